"""The library exports every dct-sim mode calls, in order, at tiny tile constants: evidence that a change to the Python that drives
the kernels left the launches alone.

    python tools/dct_sim_trace.py OUT.json

``similarity._launch`` is wrapped and the export names are recorded per mode.  Two pairs of files: ``walk`` = the two random ragged
files of tests/test_rect_walk_gpu.py (37 and 53 proteins, 0-4 fingerprints each; random rows lie beyond L1 17 000 of each other,
so cut-offs above 0 keep nothing) and ``planted`` = 36 proteins of tools/tree_bench.planted (families within L1 1 920) and the
same proteins reversed and moved a little (so the pair paths run).  COL_ROWS = 16, TILE_INTS = 60, STRIPE_ROWS = 24 and TEXT_BYTES = 400
on every class that has them.  Run it on two trees and compare the files: the sequences are deterministic (the host decides every
launch from counts, never from timing)."""

from __future__ import annotations

import json
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from tree_bench import planted  # noqa: E402

CONSTANTS = {'COL_ROWS': 16, 'TILE_INTS': 60, 'STRIPE_ROWS': 24, 'TEXT_BYTES': 400}
CLASSES = ('Blocks', 'AllPairs', 'FilteredPairs', 'ProteinSearch', 'ReciprocalBest', 'Assignment', 'DomainClusters')


def walk_files(width: int = 480):
    rng = np.random.default_rng(5)
    idx = [np.concatenate([[0], np.cumsum(rng.integers(0, 5, n))]).astype(np.int64) for n in (37, 53)]
    fps = [rng.integers(-128, 128, (int(i[-1]), width), dtype=np.int8) for i in idx]
    return [(np.array([f'{tag}{k:02d}' for k in range(len(i) - 1)]), i, f) for tag, i, f in zip('ab', idx, fps)]


def planted_files():
    """36 proteins in six families, and the same proteins in reverse order with every byte moved by at most 1."""
    sid, idx, dct, _ = planted(6, 6, seed=1)
    prots = [dct[p0:p1] for p0, p1 in zip(idx[:-1], idx[1:])][::-1]
    back = np.concatenate(prots).astype(np.int64)
    back = np.clip(back + np.random.default_rng(2).integers(-1, 2, size=back.shape), -127, 127).astype(np.int8)
    back_idx = np.concatenate([[0], np.cumsum([len(p) for p in prots])]).astype(np.int64)
    return [(sid, idx, dct), (np.array([f'rev_{s}' for s in sid[::-1]]), back_idx, back)]


def modes(a: str, b: str, out: str):
    """(function of dct_sim, arguments, keywords) of every traced mode; ``a`` / ``b`` = the two npz paths, ``out`` = where the text goes."""
    cuts = ({'min_domain': 0.5}, {'min_global': 0.3}, {'min_domain': 0.5, 'min_global': 0.3})
    yield from (('db_search', (a, b, 3, 0.25, out), {'rank': r}) for r in ('global', 'domain'))
    yield from (('rbh_sim', (a, b, out), {'score': s}) for s in ('domain', 'global'))
    yield from (('all_sim', (a, out), kw) for kw in (cuts[0], cuts[2], {'domains': True}))
    yield from (('cluster_sim', (a, out), {'linkage': k, **c}) for k in ('single', 'greedy') for c in cuts)
    yield 'cluster_sim', (a, out), {'min_domain': 0.5, 'level': 'domain'}
    yield from (('assign_sim', (a, b, out), c) for c in (cuts[0], cuts[2]))
    yield from (('tree_sim', (a, out), {'score': s}) for s in ('domain', 'global'))


def main(argv=None):
    target, = argv if argv is not None else sys.argv[1:]
    from dctdomain_amd import dct_sim, similarity
    for name in CLASSES:
        for const, value in CONSTANTS.items():
            if hasattr(getattr(dct_sim, name), const):
                setattr(getattr(dct_sim, name), const, value)
    calls, real = [], similarity._launch
    similarity._launch = lambda device, name, *args: (calls.append(name), real(device, name, *args))[1]
    trace = {}
    with tempfile.TemporaryDirectory() as tmp:
        for data, files in (('walk', walk_files()), ('planted', planted_files())):
            paths = [os.path.join(tmp, f'{data}{k}-dct.npz') for k in (0, 1)]
            for path, (sid, idx, fps) in zip(paths, files):
                np.savez(path, sid=np.asarray(sid), idx=idx, dct=fps)
            for fn, args, kw in modes(*paths, os.path.join(tmp, 'out.txt')):
                calls.clear()
                getattr(dct_sim, fn)(*args, **kw)
                trace[f'{data}: {fn} ' + ' '.join(f'{k}={v}' for k, v in kw.items())] = list(calls)
    os.makedirs(os.path.dirname(os.path.abspath(target)), exist_ok=True)
    with open(target, 'w') as fh:
        json.dump(trace, fh, indent=0)
    print(f'{len(trace)} modes, {sum(len(v) for v in trace.values())} launches -> {target}')


if __name__ == '__main__':
    main()
