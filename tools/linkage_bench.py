"""dct-sim --hac on one GPU: the scan kernel beside rect_best, one round of the merge kernel, and whole runs beside --cluster.

    python tools/linkage_bench.py --part scan  [--n 16000] [--repeats 5] [--out F.jsonl]
    python tools/linkage_bench.py --part merge [--n 16000] [--repeats 3] [--out F.jsonl]
    python tools/linkage_bench.py --part run   [--families 160] [--size 100] [--repeats 2] [--out F.jsonl]

`scan`: linkage_nearest alone on an all-live n x n matrix of random keys -- int32 (complete) and int64 (average) -- beside
dctfp_rect_best on the same int32 matrix (its row side does the same reduction, and a column side on top), device events, the
median of `--repeats` after one warm-up, and the bytes of the matrix per second beside them.  nn is checked against rect_best's
best_row before anything is timed.
`merge`: one round of linkage_merge in which n / 3 disjoint random pairs merge (what a first round does), per element type, with
the bytes it touches: per merged row 2 coalesced reads and 1 write of a row, the gathers (x, p_y), (p_x, p_y) for the paired
columns and the mirror store for the others -- each gather and mirror store counted as the 4 or 8 bytes it asks for.
`run`: tools/tree_bench.planted -- families x size proteins, the members of a family near copies of its first member, shuffled --
through dct_sim.Clusters(min_domain=0.5) and dct_sim.Dendrogram(min_cut=0.5) with both methods, in one process after a warm-up on
a small file: seconds, rounds, and the build's own split (matrix / scan / merge, host clocks around a device synchronise, which
`Dendrogram.timed` turns on) in a second, timed pass, and the --flat text to /dev/null.  The clusters are checked against the
planted families before a time is reported."""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _median_ms(call, repeats: int, reset=None):
    import torch
    times = []
    for _ in range(repeats + 1):
        if reset is not None:
            reset()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return sorted(times[1:])[len(times[1:]) // 2], [round(t, 4) for t in times[1:]]


def _matrix(n: int, wide: bool, seed: int = 3):
    """A symmetric n x n matrix of random keys 0 .. 16999 on the device, rows padded to 16 bytes, the diagonal at the sentinel."""
    import torch
    from dctdomain_amd.similarity import LINKAGE_NONE
    gen = torch.Generator(device='cuda').manual_seed(seed)
    ld = (n + 3) // 4 * 4
    store = torch.randint(0, 17000, (n, ld), dtype=torch.int32, device='cuda', generator=gen)
    mat = store[:, :n]
    mat.copy_(torch.minimum(mat, mat.T.contiguous()))
    if wide:
        store = store.long()
        mat = store[:, :n]
    mat.diagonal().fill_(LINKAGE_NONE[mat.dtype])
    return mat


def part_scan(args):
    import torch
    from dctdomain_amd.similarity import BestState, linkage_nearest, rect_best
    n, bound = args.n, 16999
    size = torch.ones(n, dtype=torch.int32, device='cuda')
    live = torch.arange(n, dtype=torch.int32, device='cuda')
    rows = []
    mat = _matrix(n, False)
    state = BestState(n, n)
    rect_best(mat, 0, 0, bound, state)
    nn = linkage_nearest(mat, size, live, bound)
    assert torch.equal(nn.long(), state.best_row & 0xffffffff), 'linkage_nearest and rect_best disagree'

    def fresh():
        state.best_row.fill_(-1)
        state.best_col.fill_(-1)
    cases = [('linkage_nearest', 'int32', mat, lambda: linkage_nearest(mat, size, live, bound, nn), None),
             ('rect_best', 'int32', mat, lambda: rect_best(mat, 0, 0, bound, state), fresh)]
    for name, kind, m, call, reset in cases:
        ms, every = _median_ms(call, args.repeats, reset)
        rows.append({'what': 'scan', 'kernel': name, 'entries': kind, 'n': n, 'matrix_bytes': m.element_size() * n * n, 'ms_all': every,
                     'ms_median': round(ms, 4), 'matrix_GB_per_s': round(m.element_size() * n * n / ms / 1e6, 1)})
    del mat, state
    wide = _matrix(n, True)
    ms, every = _median_ms(lambda: linkage_nearest(wide, size, live, bound, nn), args.repeats)
    rows.append({'what': 'scan', 'kernel': 'linkage_nearest', 'entries': 'int64', 'n': n, 'matrix_bytes': 8 * n * n, 'ms_all': every,
                 'ms_median': round(ms, 4), 'matrix_GB_per_s': round(8 * n * n / ms / 1e6, 1)})
    for row in rows:
        row['device'] = torch.cuda.get_device_name(0)
        print(json.dumps(row), flush=True)
    return rows


def part_merge(args):
    import torch
    from dctdomain_amd.similarity import linkage_merge
    n = args.n
    gen = torch.Generator(device='cuda').manual_seed(9)
    pick = torch.randperm(n, device='cuda', generator=gen)[:2 * (n // 3)].view(-1, 2)
    lo, hi = pick.min(dim=1).values, pick.max(dim=1).values
    partner = torch.full((n,), -1, dtype=torch.int32, device='cuda')
    partner[lo] = hi.int()
    partner[hi] = lo.int()
    keep = lo.int().contiguous()
    size = torch.ones(n, dtype=torch.int32, device='cuda')
    m = keep.numel()
    rows = []
    for wide in (False, True):
        mat = _matrix(n, wide)
        b = mat.element_size()
        ms, every = _median_ms(lambda: linkage_merge(mat, size, partner, keep), args.repeats)   # (repeated on its own output: the same traffic)
        survivors = n - m                                        # columns a merged row updates; m of them have a pair of their own
        touched = m * (2 * n * b + survivors * b + 2 * m * b + (survivors - m) * b)
        rows.append({'what': 'merge', 'entries': 'int64' if wide else 'int32', 'n': n, 'pairs': m, 'ms_all': every, 'ms_median': round(ms, 4),
                     'bytes_touched': touched, 'gather_bytes': 2 * m * m * b, 'mirror_store_bytes': m * (survivors - m) * b,
                     'GB_per_s': round(touched / ms / 1e6, 1), 'device': torch.cuda.get_device_name(0)})
        print(json.dumps(rows[-1]), flush=True)
        del mat
    return rows


def part_run(args):
    import torch
    from dctdomain_amd import dct_sim
    from tools.tree_bench import planted
    sid, idx, dct, fam = planted(args.families, args.size)
    n = len(sid)
    first = np.full(args.families, n)
    np.minimum.at(first, fam, np.arange(n))
    want = first[fam]
    small = planted(20, 10)

    def cluster(s, i, d):
        job = dct_sim.Clusters(s, i, d, min_domain=0.5)
        labels = job.labels()
        with open(os.devnull, 'wb') as null:
            job.write(null.write, labels)
        return labels, {}

    def hac(method, timed):
        def go(s, i, d):
            tree = dct_sim.Dendrogram(s, i, d, method=method, score='domain', min_cut=0.5)
            tree.timed = timed
            labels = tree.labels()
            t0 = time.perf_counter()
            with open(os.devnull, 'wb') as null:
                for part in dct_sim.cluster_lines(s, labels):
                    null.write(memoryview(part))
            return labels, {'rounds': tree.rounds, 'merges': len(tree.merges()[0]), 'matrix_bytes': tree.matrix_bytes(),
                            'text_seconds': round(time.perf_counter() - t0, 4),
                            **({'split_seconds': {k: round(v, 4) for k, v in tree.seconds.items()}} if timed else {})}
        return go
    jobs = [('cluster', cluster), ('hac_complete', hac('complete', False)), ('hac_complete_split', hac('complete', True)),
            ('hac_average', hac('average', False)), ('hac_average_split', hac('average', True))]
    for _, job in jobs:                                          # warm-up: code objects loaded, the allocator primed
        job(*small[:3])
    rows = []
    for _ in range(args.repeats):
        for what, job in jobs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            labels, extra = job(sid, idx, dct)
            torch.cuda.synchronize()
            seconds = time.perf_counter() - t0
            assert np.array_equal(labels, want), f'{what}: not the planted families'
            rows.append({'what': what, 'seconds': round(seconds, 4), 'proteins': n, 'fingerprints': int(idx[-1]), **extra,
                         'device': torch.cuda.get_device_name(0)})
            print(json.dumps(rows[-1]), flush=True)
            torch.cuda.empty_cache()
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--part', choices=('scan', 'merge', 'run'), default='scan')
    ap.add_argument('--n', type=int, default=16000)
    ap.add_argument('--families', type=int, default=160)
    ap.add_argument('--size', type=int, default=100)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('linkage_bench measures on a GPU: none found')
    rows = {'scan': part_scan, 'merge': part_merge, 'run': part_run}[args.part](args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as fh:
            for row in rows:
                fh.write(json.dumps(row) + '\n')


if __name__ == '__main__':
    main()
