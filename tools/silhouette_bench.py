"""python -m dctdomain_amd.cluster_quality on one GPU: the scan kernel beside rect_moments, and whole runs beside --cluster.

    python tools/silhouette_bench.py --part scan [--rows 8192] [--cols 50000] [--repeats 5] [--variant-lib LIB.so] [--out F.jsonl]
    python tools/silhouette_bench.py --part run  [--families 160] [--size 100] [--repeats 2] [--out F.jsonl]

`scan`: dctfp_silhouette_rows alone on one rows x cols int32 tile of random keys 0 .. 16999 (the rows are the first proteins of a
file of `cols`), per label layout -- one cluster; cols / 100 contiguous clusters of 100; the same interleaved; cols / 2 clusters of
2 (7 passes at 50 000); all singletons -- beside dctfp_rect_moments' row side on the same tile (both read every entry once and
reduce per row): device events, the median of `--repeats` after one warm-up, the ratio and the TB/s of tile.  `--variant-lib`: a
second build of the library (build_ext.build_library(extra_flags=['-DDCTFP_SIL_SHARED_ADD=0'], flag_units=['k_silhouette.hip'],
lib_path=...)) in which every lane adds its own key to LDS: what the wave's shared-key step is worth, in the same process, the
two builds taking turns.  The results of the two builds are compared before anything is timed.
`run`: tools/tree_bench.planted -- families x size proteins -- through dct_sim.Clusters(min_domain=0.5), whose labels are the
clustering judged; then cluster_quality.Silhouette (sums and the text to /dev/null) beside Clusters itself (the triangle, once)
and beside the matrix build of --hac (Dendrogram._matrix: the full square, as here), in one process after a warm-up on a small file."""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _median_ms(call, repeats: int):
    import torch
    times = []
    for _ in range(repeats + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return sorted(times[1:])[len(times[1:]) // 2], [round(t, 4) for t in times[1:]]


def layouts(n: int):
    """{name: one label per protein}."""
    per = max(1, n // 100)
    return {'one_cluster': np.zeros(n, dtype=np.int64), 'contiguous_x100': np.arange(n) // 100, 'interleaved_x100': np.arange(n) % per,
            'pairs': np.arange(n) // 2, 'all_singletons': np.arange(n)}


def part_scan(args):
    import torch
    from dctdomain_amd import _lib
    from dctdomain_amd.cluster_quality import Silhouette
    from dctdomain_amd.similarity import MomentState, rect_moments
    n_rows, n = min(args.rows, args.cols), args.cols
    gen = torch.Generator(device='cuda').manual_seed(5)
    tile = torch.randint(0, 17000, (n_rows, n), dtype=torch.int32, device='cuda', generator=gen)
    tile_bytes = 4 * n_rows * n
    builds = {'product': _lib.get_context(0)}
    if args.variant_lib:
        builds['own_adds'] = _lib.Context(0, _lib.load(os.path.abspath(args.variant_lib)))
    state = MomentState(n, n, rows=True, cols=False)
    base_ms, base_all = _median_ms(lambda: rect_moments(tile, 0, 0, state), args.repeats)
    rows = [{'what': 'scan', 'kernel': 'rect_moments_rows', 'rows': n_rows, 'cols': n, 'tile_bytes': tile_bytes, 'ms_all': base_all,
             'ms_median': round(base_ms, 4), 'tile_TB_per_s': round(tile_bytes / base_ms / 1e9, 3)}]
    for name, labels in layouts(n).items():
        cid, size, first = (torch.as_tensor(a, device='cuda') for a in Silhouette([''] * n, None, None, labels.tolist()).device_clusters())
        outs = {b: (torch.zeros(n, dtype=torch.int64, device='cuda'), torch.zeros(n, dtype=torch.int64, device='cuda'),
                    torch.zeros(n, dtype=torch.int32, device='cuda'), torch.zeros(n, dtype=torch.int32, device='cuda')) for b in builds}

        def call(b):
            builds[b].call('dctfp_silhouette_rows', tile.data_ptr(), n_rows, n, n, 0, 0, None, None, 17000, cid.data_ptr(),
                           size.data_ptr() if size.numel() else None, first.data_ptr() if first.numel() else None, size.numel(), args.pass_clusters,
                           *(t.data_ptr() for t in outs[b]), n)
        for b in builds:
            call(b)
        torch.cuda.synchronize()
        for b in builds:
            assert all(torch.equal(x, y) for x, y in zip(outs[b], outs['product'])), f'{name}: the builds disagree'
        timed = {b: [] for b in builds}
        for _ in range(args.rounds):                                # (the builds take turns: one process, one device, interleaved)
            for b in builds:
                timed[b].append(_median_ms(lambda: call(b), args.repeats))
        for b in builds:
            ms = sorted(m for m, _ in timed[b])[len(timed[b]) // 2]
            rows.append({'what': 'scan', 'kernel': 'silhouette_rows', 'build': b, 'layout': name, 'clusters': int(size.numel()),
                         'passes': max(1, -(-int(size.numel()) // args.pass_clusters)), 'rows': n_rows, 'cols': n, 'tile_bytes': tile_bytes,
                         'ms_all': [every for _, every in timed[b]], 'ms_median': round(ms, 4), 'tile_TB_per_s': round(tile_bytes / ms / 1e9, 3),
                         'ratio_to_rect_moments': round(ms / base_ms, 3)})
    for row in rows:
        row['device'] = torch.cuda.get_device_name(0)
        print(json.dumps(row), flush=True)
    return rows


def part_run(args):
    import torch
    from dctdomain_amd import dct_sim
    from dctdomain_amd.cluster_quality import Silhouette
    from tools.tree_bench import planted
    sid, idx, dct, _fam = planted(args.families, args.size)
    n = len(sid)
    small = planted(20, 10)
    dev = torch.device('cuda', torch.cuda.current_device())
    found = {}

    def cluster(s, i, d):
        job = dct_sim.Clusters(s, i, d, min_domain=0.5)
        labels = job.labels()
        with open(os.devnull, 'wb') as null:
            job.write(null.write, labels)
        found[len(s)] = labels
        return {'clusters': int(len(np.unique(labels)))}

    def quality(s, i, d):
        job = Silhouette(s, i, d, found[len(s)].tolist(), score='domain')
        job.sums()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with open(os.devnull, 'wb') as null:
            job.write(null.write)
        summary = job.summary()
        return {'stripes': len(job._stripes()), 'text_seconds': round(time.perf_counter() - t0, 4), 'mean_silhouette': summary['mean'],
                'negative': summary['negative']}

    def matrix(s, i, d):
        mat = dct_sim.Dendrogram(s, i, d, method='complete', score='domain', min_cut=0.5)._matrix(dev)
        return {'matrix_bytes': int(mat.numel() * 4)}
    jobs = [('cluster', cluster), ('cluster_quality', quality), ('hac_matrix_build', matrix)]
    for _, job in jobs:                                          # warm-up: code objects loaded, the allocator primed
        job(*small[:3])
    rows = []
    for _ in range(args.repeats):
        for what, job in jobs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            extra = job(sid, idx, dct)
            torch.cuda.synchronize()
            rows.append({'what': what, 'seconds': round(time.perf_counter() - t0, 4), 'proteins': n, 'fingerprints': int(idx[-1]), **extra,
                         'device': torch.cuda.get_device_name(0)})
            print(json.dumps(rows[-1]), flush=True)
            torch.cuda.empty_cache()
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--part', choices=('scan', 'run'), default='scan')
    ap.add_argument('--rows', type=int, default=8192)
    ap.add_argument('--cols', type=int, default=50000)
    ap.add_argument('--pass-clusters', type=int, default=4096)
    ap.add_argument('--variant-lib', default=None)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--families', type=int, default=160)
    ap.add_argument('--size', type=int, default=100)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('silhouette_bench measures on a GPU: none found')
    rows = {'scan': part_scan, 'run': part_run}[args.part](args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as fh:
            for row in rows:
                fh.write(json.dumps(row) + '\n')


if __name__ == '__main__':
    main()
