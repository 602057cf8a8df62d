"""dct-sim --db --rbh on one GPU: wall time after the load, split into tile and scan, beside the one-directional search pass.

    python tools/rbh_bench.py [--families 1000] [--size 100] [--queries 10000] [--repeats 3] [--out profiles/rbh/result.json]

Input: file B = families x size proteins in planted families (tools/tree_bench.planted: 1-8 int8 fingerprints each, members of a
family within L1 1 920 of each other, strangers at 15 500 +- 500, shuffled); file A = `queries` proteins of B drawn at random,
each row moved by a further +-2.  Timed, alternating, in one process after a warm-up of every shape:
  rbh domain      dct_sim.ReciprocalBest(score='domain'): best() (the pass) and lines() (both scores of the pairs, the text);
  rbh global      the same with score='global';
  search domain   dct_sim.ProteinSearch(B).search(A, top=1, threshold=2, rank='domain') -- `--db --rank domain --top 1
                  --threshold 2`, the code of the parent commit: the same protein_min pass, one direction, its own selection.
Times are host clocks around work that ends in a device synchronise; the split comes from device events around the calls that
fill a tile (protein_min / l1_matrix), scan it (rect_best) or select from it (threshold_select).  Before a time is reported the
result is checked: every protein of A finds a protein of its own family, and best_b of `rbh domain` is the search's only hit."""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from tree_bench import Split, planted  # noqa: E402

STEPS = {'protein_min': 'tile', 'l1_matrix': 'tile', 'rect_best': 'scan', 'threshold_select': 'select'}


def two_files(families: int, size: int, queries: int, seed: int = 11):
    """((sid, idx, dct, family) of A, the same of B)."""
    sid, idx, dct, fam = planted(families, size)
    rng = np.random.default_rng(seed)
    pick = rng.choice(len(sid), size=min(queries, len(sid)), replace=False)
    counts = idx[pick + 1] - idx[pick]
    a_idx = np.zeros(len(pick) + 1, dtype=np.int64)
    np.cumsum(counts, out=a_idx[1:])
    rows = np.repeat(idx[pick] - a_idx[:-1], counts) + np.arange(a_idx[-1])
    a_dct = np.clip(dct[rows].astype(np.int64) + rng.integers(-2, 3, size=(len(rows), dct.shape[1])), -127, 127).astype(np.int8)
    a_sid = np.array([f'query_{k:08d}' for k in range(len(pick))])
    return (a_sid, a_idx, a_dct, fam[pick]), (sid, idx, dct, fam)


def run(dct_sim, what: str, a, b):
    import torch
    torch.cuda.synchronize()
    with Split(dct_sim, STEPS) as split:
        t0 = time.perf_counter()
        if what == 'search domain':
            hits = dct_sim.ProteinSearch(b[2], b[1]).search(a[2], a[1], 1, 2.0, rank='domain')
            torch.cuda.synchronize()
            t1 = t2 = time.perf_counter()
            best_b, lines = np.array([int(h[0][0]) if len(h[0]) else -1 for h in hits]), len(hits)
        else:
            job = dct_sim.ReciprocalBest(a[0], a[1], a[2], b[0], b[1], b[2], score=what.split()[1])
            (best_b, _), _ = job.best()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            lines = len(job.lines())
            t2 = time.perf_counter()
        parts = split.totals()
    row = {'what': what, 'seconds': round(t2 - t0, 3), 'pass_seconds': round(t1 - t0, 3), 'text_seconds': round(t2 - t1, 3), 'lines': lines,
           'device_seconds': parts}
    return row, best_b


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--families', type=int, default=1000)
    ap.add_argument('--size', type=int, default=100)
    ap.add_argument('--queries', type=int, default=10000)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    import torch
    from dctdomain_amd import dct_sim
    if not torch.cuda.is_available():
        raise SystemExit('rbh_bench measures on a GPU: none found')
    a, b = two_files(args.families, args.size, args.queries)
    small = two_files(20, 10, 50)
    jobs = ('search domain', 'rbh domain', 'rbh global')
    for what in jobs:                                           # warm-up: code objects loaded, the allocator primed
        run(dct_sim, what, *small)
    rows, want = [], None
    for _ in range(args.repeats):
        for what in jobs:
            row, best_b = run(dct_sim, what, a, b)
            assert (best_b >= 0).all() and np.array_equal(b[3][best_b], a[3]), f'{what}: a protein of A does not find its family'
            if what == 'search domain':
                want = best_b
            elif what == 'rbh domain':
                assert np.array_equal(best_b, want), 'best_b of the reciprocal pass is not the hit of the search'
            rows.append(row)
            print(json.dumps(row), flush=True)
    result = {'proteins_a': len(a[0]), 'proteins_b': len(b[0]), 'fingerprints_a': int(a[1][-1]), 'fingerprints_b': int(b[1][-1]),
              'device': torch.cuda.get_device_name(0), 'runs': rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(result, fh, indent=1)
    return result


if __name__ == '__main__':
    main()
