"""dct-sim --tree on one GPU: rounds, time per round split into tile and scan, and the total, beside one --cluster pass.

    python tools/tree_bench.py [--families 500] [--size 100] [--repeats 2] [--out profiles/tree/result.json]

Input: families x size proteins (1-8 uniform int8 fingerprints in [-48, 48] each, tools/all_sim_bench.synth's proteins); the
members of a family are copies of its first member's rows within +-2 each (L1 <= 1 920 inside a family, 15 500 +- 500 between
strangers), shuffled over the file.  Timed, alternating, in one process after a warm-up of every shape:
  tree            dct_sim.Tree(...).edges() at the default bound (every pair of similarity above 0);
  tree@0.5        the same with min_cut = 0.5;
  cluster@0.5     dct_sim.Clusters(min_domain=0.5).labels() -- the code of the parent commit, unchanged by --tree.
Times are host clocks around work that ends in a device synchronise; the split comes from device events around the calls that
fill a tile (protein_min), scan it (tri_nearest) and end a round (tree_hook + cluster_labels), summed per build.  The labels of
the tree cut at 0.5 are compared with the cluster pass before anything is reported."""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def planted(families: int, size: int, seed: int = 7):
    """(sid, idx, dct, family of every protein)."""
    rng = np.random.default_rng(seed)
    n = families * size
    fam = rng.permutation(np.repeat(np.arange(families), size))
    rows_of = rng.integers(1, 9, size=families)
    base = [rng.integers(-48, 49, size=(int(r), 480), dtype=np.int8) for r in rows_of]
    counts = rows_of[fam]
    idx = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts, out=idx[1:])
    dct = np.concatenate([base[f] for f in fam.tolist()]).astype(np.int64)
    dct = np.clip(dct + rng.integers(-2, 3, size=dct.shape), -127, 127).astype(np.int8)
    sid = np.array([f'UniRef50_{k:08d}' for k in range(n)])
    return sid, idx, dct, fam


class Split:
    """Device events around the named functions of dct_sim, summed per key after a synchronise."""

    def __init__(self, dct_sim, names: dict):
        import torch
        self.torch, self.mod, self.names, self.events, self.saved = torch, dct_sim, names, [], {}

    def __enter__(self):
        for name, key in self.names.items():
            fn = self.saved[name] = getattr(self.mod, name)

            def timed(*a, _fn=fn, _key=key, **kw):
                e0, e1 = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
                e0.record()
                out = _fn(*a, **kw)
                e1.record()
                self.events.append((_key, e0, e1))
                return out
            setattr(self.mod, name, timed)
        return self

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(self.mod, name, fn)

    def totals(self) -> dict:
        self.torch.cuda.synchronize()
        out = {}
        for key, e0, e1 in self.events:
            out[key] = out.get(key, 0.0) + e0.elapsed_time(e1) / 1e3
        return {k: round(v, 4) for k, v in out.items()}


STEPS = {'protein_min': 'tile', 'l1_matrix': 'tile', 'tri_nearest': 'scan', 'tri_link': 'link', 'tree_hook': 'hook', 'cluster_labels': 'labels'}


def run(dct_sim, what: str, sid, idx, dct):
    import torch
    torch.cuda.synchronize()
    with Split(dct_sim, STEPS) as split:
        t0 = time.perf_counter()
        if what == 'cluster@0.5':
            job = dct_sim.Clusters(sid, idx, dct, min_domain=0.5)
            labels, rounds, edges = job.labels(), 1, None
        else:
            job = dct_sim.Tree(sid, idx, dct, min_cut=0.5 if what == 'tree@0.5' else None)
            edges = job.edges()
            labels, rounds = None, job.rounds
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        parts = split.totals()
    row = {'what': what, 'seconds': round(seconds, 3), 'rounds': rounds, 'stripes': len(list(job.stripes())), 'device_seconds': parts}
    if rounds:
        row['per_round'] = {k: round(v / rounds, 4) for k, v in parts.items()}
    if edges is not None:
        row['edges'] = int(len(edges[0]))
    return row, job, labels


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--families', type=int, default=500)
    ap.add_argument('--size', type=int, default=100)
    ap.add_argument('--repeats', type=int, default=2)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    import torch
    from dctdomain_amd import dct_sim
    if not torch.cuda.is_available():
        raise SystemExit('tree_bench measures on a GPU: none found')
    sid, idx, dct, fam = planted(args.families, args.size)
    n = len(sid)
    small = planted(20, 10)
    for what in ('tree', 'tree@0.5', 'cluster@0.5'):           # warm-up: code objects loaded, the allocator primed
        run(dct_sim, what, *small[:3])
    rows = []
    want = None
    for _ in range(args.repeats):
        for what in ('cluster@0.5', 'tree@0.5', 'tree'):
            row, job, labels = run(dct_sim, what, sid, idx, dct)
            if what == 'cluster@0.5':
                want = labels
                first = np.full(args.families, n)
                np.minimum.at(first, fam, np.arange(n))
                assert np.array_equal(labels, first[fam]), 'the cluster pass does not return the planted families'
            else:
                assert np.array_equal(job.labels(0.5), want), f'{what}: cut at 0.5 the tree does not give the clusters'
                assert row['edges'] == (n - args.families if what == 'tree@0.5' else n - 1), row
            rows.append(row)
            print(json.dumps(row), flush=True)
    result = {'proteins': n, 'families': args.families, 'fingerprints': int(idx[-1]), 'device': torch.cuda.get_device_name(0), 'runs': rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(result, fh, indent=1)
    return result


if __name__ == '__main__':
    main()
