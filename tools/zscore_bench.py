"""dct-sim --db --zscore on one GPU: the scan alone beside rect_best, and the searches with and without it.

    python tools/zscore_bench.py --part scan [--repeats 7]
    python tools/zscore_bench.py --part run [--families 1000] [--size 100] [--queries 10000] [--repeats 5] [--out FILE]

scan: one int32 tile of 8192 x 16384 entries of L1s around 15 500 (every entry counts).  hipEvents around one call, after one untimed
call: `rect_best` (bound 16999, settled arrays), a plain read of the tile (`torch.max`), and `rect_moments` with rows only, columns
only and both.  The moments are compared with torch's own sums before anything is timed.
run: the files of tools/rbh_bench.py (B = families x size planted proteins, A = `queries` of them, moved a little).  Timed,
alternating, in one process after a warm-up of every shape: `--db --rank global`, `--db --rank domain` (top 5, threshold 0.25) and
`--db --rbh domain`, each without and with z-scores.  Host clocks around work that ends in a device synchronise; device events
around the calls that fill a tile (protein_min / l1_matrix), scan it (rect_moments, rect_best) or select from it (threshold_select).
Before a time is reported the z-scores of one query are compared with numpy's on that query's row of the tile.
A build without the feature (the parent commit) runs the jobs it has: the flagless ones."""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from rbh_bench import two_files  # noqa: E402
from tree_bench import Split  # noqa: E402

STEPS = {'protein_min': 'tile', 'l1_matrix': 'tile', 'rect_moments': 'moments', 'rect_best': 'best', 'threshold_select': 'select'}


def _timed(torch, fn, repeats: int):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return sorted(out)


def scan(repeats: int):
    import torch
    from dctdomain_amd import similarity
    n_rows, n_cols, limit = 8192, 16384, 255 * 480 + 1
    g = torch.Generator(device='cuda').manual_seed(5)
    tile = torch.randint(15000, 16000, (n_rows, n_cols), dtype=torch.int32, device='cuda', generator=g)
    has = hasattr(similarity, 'rect_moments')
    rows = []
    if has:
        state = similarity.MomentState(n_rows, n_cols)
        similarity.rect_moments(tile, 0, 0, state, limit=limit)
        wide = tile.to(torch.int64)
        for got, axis, n in ((state.row, 1, n_cols), (state.col, 0, n_rows)):
            assert bool((got[0] == n).all()) and torch.equal(got[1], wide.sum(axis)) and torch.equal(got[2], (wide * wide).sum(axis))
        del wide
    best = similarity.BestState(n_rows, n_cols)
    jobs = [('rect_best', lambda: similarity.rect_best(tile, 0, 0, 16999, best)), ('read (torch.max)', lambda: tile.max())]
    if has:
        for name, r, c in (('rect_moments rows', True, False), ('rect_moments cols', False, True), ('rect_moments both', True, True)):
            st = similarity.MomentState(n_rows, n_cols, rows=r, cols=c)
            jobs.append((name, lambda st=st: similarity.rect_moments(tile, 0, 0, st, limit=limit)))
    for name, fn in jobs:
        ms = _timed(torch, fn, repeats)
        row = {'what': name, 'median_ms': round(ms[len(ms) // 2], 4), 'min_ms': round(ms[0], 4), 'max_ms': round(ms[-1], 4),
               'tb_per_s': round(tile.numel() * 4 / ms[len(ms) // 2] / 1e9, 3)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def run(dct_sim, what: str, a, b):
    import torch
    mode, score, z = what.split()[0], what.split()[1], what.endswith('+z')
    kw = {'zscore': True} if z else {}
    torch.cuda.synchronize()
    with Split(dct_sim, {k: v for k, v in STEPS.items() if hasattr(dct_sim, k)}) as split:
        t0 = time.perf_counter()
        if mode == 'search':
            out = dct_sim.ProteinSearch(b[2], b[1]).search(a[2], a[1], 5, 0.25, rank=score, **kw)
            torch.cuda.synchronize()
            t1 = t2 = time.perf_counter()
            lines = sum(len(h[0]) for h in out)
        else:
            job = dct_sim.ReciprocalBest(a[0], a[1], a[2], b[0], b[1], b[2], score=score)
            if z:
                job.with_zscore()
            job.best()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            out = job.lines()
            lines = len(out)
            t2 = time.perf_counter()
        parts = split.totals()
    return {'what': what, 'seconds': round(t2 - t0, 4), 'pass_seconds': round(t1 - t0, 4), 'text_seconds': round(t2 - t1, 4), 'lines': lines,
            'device_seconds': parts}, out


def check(dct_sim, a, b, out, score: str):
    """The z-scores of query 0 against numpy on its own row of L1s (every protein of these files has fingerprints)."""
    from dctdomain_amd import similarity
    q = 0
    if score == 'global':
        row = similarity.l1_matrix(a[2][a[1][1] - 1:a[1][1]], b[2][b[1][1:] - 1]).cpu().numpy()[0].astype(np.float64)
    else:
        row = similarity.protein_min(similarity.to_device_int8(a[2][:a[1][1]]), a[1][:2], similarity.to_device_int8(b[2]), b[1]).cpu().numpy()[0].astype(np.float64)
    d = out[q][1 if score == 'domain' else 2].astype(np.float64)
    assert np.allclose(out[q][-1], (row.mean() - d) / row.std(), rtol=1e-9), 'z of query 0 is not numpy\'s'


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--part', choices=('scan', 'run'), required=True)
    ap.add_argument('--families', type=int, default=1000)
    ap.add_argument('--size', type=int, default=100)
    ap.add_argument('--queries', type=int, default=10000)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    import torch
    from dctdomain_amd import dct_sim
    if not torch.cuda.is_available():
        raise SystemExit('zscore_bench measures on a GPU: none found')
    if args.part == 'scan':
        result = {'device': torch.cuda.get_device_name(0), 'runs': scan(args.repeats)}
    else:
        has = hasattr(dct_sim, 'zscore_of')
        a, b = two_files(args.families, args.size, args.queries)
        small = two_files(20, 10, 50)
        jobs = [j for j in ('search global', 'search global +z', 'search domain', 'search domain +z', 'rbh domain', 'rbh domain +z')
                if has or not j.endswith('+z')]
        for what in jobs:                                           # warm-up: code objects loaded, the allocator primed
            run(dct_sim, what, *small)
        rows = []
        for k in range(args.repeats):
            for what in jobs:
                row, out = run(dct_sim, what, a, b)
                if k == 0 and what.startswith('search') and what.endswith('+z'):
                    check(dct_sim, a, b, out, what.split()[1])
                rows.append(row)
                print(json.dumps(row), flush=True)
        result = {'proteins_a': len(a[0]), 'proteins_b': len(b[0]), 'fingerprints_a': int(a[1][-1]), 'fingerprints_b': int(b[1][-1]),
                  'device': torch.cuda.get_device_name(0), 'feature': has, 'runs': rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(result, fh, indent=1)
    return result


if __name__ == '__main__':
    main()
