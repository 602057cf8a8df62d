#!/usr/bin/env python3
"""dct-sim --min-coverage, measured (profiles/coverage/README.md).  One process, one GPU:

1. ``Clusters.labels()`` at ``--min-domain`` with and without ``--min-coverage`` (``--cov-unit domains``) on the planted-family file
   of profiles/cluster/ (``all_sim_bench.synth`` + ``plant_families``), the two alternating, ``--repeat`` runs each after a warm-up of
   both on a small file; wall time with a synchronise, and the device time of the tile step (``protein_min`` / ``protein_cover``)
   from events around each call;
2. ``dctfp_protein_cover`` beside ``dctfp_protein_min`` on one tile (the first ``--stripe`` proteins against the whole file), events
   around each call, the kernels alternating; with ``--parent-lib`` also ``dctfp_protein_min`` of that build of the library (the
   parent commit's), to show that this tree's is the same kernel.

    python tools/coverage_bench.py [--n 50000 --families 500 --family-size 100 --min-domain 0.5 --min-coverage 0.8]
                                   [--parent-lib PATH] [--out FILE.jsonl]
"""

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.all_sim_bench import plant_families, synth  # noqa: E402


def _file(n, families, size, seed, tmp):
    from dctdomain_amd import dct_sim
    path = os.path.join(tmp, f'f{n}-dct.npz')
    synth(path, n, seed)
    sid, idx, fps = dct_sim._load_npz(path)
    os.remove(path)
    if families:
        idx, fps = plant_families(idx, fps, families, size)
    return sid, idx, fps


def _med(v):
    return sorted(v)[len(v) // 2]


def part_cluster(args, tmp):
    import torch
    from dctdomain_amd import dct_sim
    spans = []

    def timed(name):
        fn = getattr(dct_sim, name)

        def run(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **k)
            e1.record()
            spans.append((e0, e1))
            return out
        setattr(dct_sim, name, run)

    def job(sid, idx, fps, cover):
        c = dct_sim.Clusters(sid, idx, fps, min_domain=args.min_domain)
        return c.with_coverage(args.min_coverage, dct_sim.coverage_weights(sid, idx, None, 'domains')) if cover else c

    small = _file(2000, 10, 10, 5, tmp)
    sid, idx, fps = _file(args.n, args.families, args.family_size, 7, tmp)
    for cover in (False, True):
        job(*small, cover).labels()
    timed('protein_min')
    timed('protein_cover')
    wall, tile, clusters = {False: [], True: []}, {False: [], True: []}, {}
    for _ in range(args.repeat):
        for cover in (False, True):
            spans.clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            labels = job(sid, idx, fps, cover).labels()
            torch.cuda.synchronize()
            wall[cover].append(time.perf_counter() - t0)
            tile[cover].append(sum(a.elapsed_time(b) for a, b in spans))
            clusters[cover] = int(len(np.unique(labels)))
    return {'part': 'cluster', 'n': len(sid), 'fingerprints': int(idx[-1]), 'families': args.families, 'family_size': args.family_size,
            'min_domain': args.min_domain, 'min_coverage': args.min_coverage, 'cov_unit': 'domains',
            'plain_s': [round(t, 4) for t in wall[False]], 'coverage_s': [round(t, 4) for t in wall[True]],
            'plain_median_s': round(_med(wall[False]), 4), 'coverage_median_s': round(_med(wall[True]), 4),
            'plain_tile_ms': [round(t, 2) for t in tile[False]], 'coverage_tile_ms': [round(t, 2) for t in tile[True]],
            'coverage_over_plain': round(_med(wall[True]) / _med(wall[False]), 4),
            'coverage_over_plain_tile': round(_med(tile[True]) / _med(tile[False]), 4),
            'clusters_plain': clusters[False], 'clusters_coverage': clusters[True]}, (sid, idx, fps)


def part_kernel(args, data):
    import torch
    from dctdomain_amd import _lib, dct_sim
    from dctdomain_amd.similarity import protein_cover, protein_min
    sid, idx, fps = data
    dev = torch.device('cuda', torch.cuda.current_device())
    p1 = min(args.stripe, len(sid))
    b = torch.as_tensor(fps[:int(idx[-1])], device=dev)
    a, ia = b[:int(idx[p1])], idx[:p1 + 1]
    w = dct_sim.coverage_weights(sid, idx, None, 'domains')
    need = dct_sim.coverage_need(w[np.maximum(idx[1:], 1) - 1], args.min_coverage)
    w_dev, need_dev = torch.as_tensor(w.astype(np.int32), device=dev), torch.as_tensor(need.astype(np.int32), device=dev)
    bound = dct_sim.sim_bound(args.min_domain)
    out = torch.empty((p1, len(sid)), dtype=torch.int32, device=dev)
    runs = {'protein_min': lambda: protein_min(a, ia, b, idx, out=out),
            'protein_cover': lambda: protein_cover(a, ia, w_dev[:int(idx[p1])], need_dev[:p1], b, idx, w_dev, need_dev, bound, out=out),
            'protein_cover_no_need': lambda: protein_cover(a, ia, w_dev[:int(idx[p1])], torch.zeros_like(need_dev[:p1]), b, idx, w_dev,
                                                           torch.zeros_like(need_dev), bound, out=out)}
    if args.parent_lib:
        lib = C.CDLL(args.parent_lib)
        lib.dctfp_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        lib.dctfp_protein_min.argtypes = _lib.load().dctfp_protein_min.argtypes
        ctx = C.c_void_p()
        assert lib.dctfp_create(dev.index, C.byref(ctx)) == 0
        ia_dev, ib_dev = torch.as_tensor(ia, device=dev), torch.as_tensor(idx, device=dev)

        def parent():
            rc = lib.dctfp_protein_min(ctx, a.data_ptr(), a.stride(0), ia_dev.data_ptr(), p1, b.data_ptr(), b.stride(0), ib_dev.data_ptr(),
                                       len(sid), a.shape[1], out.data_ptr(), out.stride(0), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
            assert rc == 0
        runs['protein_min_parent_build'] = parent
    results = {}
    for name, fn in runs.items():                               # warm-up, and the outputs compared
        fn()
        results[name] = out.clone()
    same = {name: bool(torch.equal(t, results['protein_min'])) for name, t in results.items()}
    dropped = int((results['protein_cover'] != results['protein_min']).sum())
    ms = {name: [] for name in runs}
    for _ in range(args.kernel_repeat):
        for name, fn in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    med = {name: _med(v) for name, v in ms.items()}
    return {'part': 'kernel', 'proteins_a': p1, 'rows_a': int(idx[p1]), 'proteins_b': len(sid), 'rows_b': int(idx[-1]), 'bound': bound,
            'entries_within_bound': int((results['protein_min'] <= bound).sum()), 'entries_dropped_by_coverage': dropped,
            'equal_to_protein_min': same, 'ms': {name: [round(t, 3) for t in v] for name, v in ms.items()},
            'median_ms': {name: round(t, 3) for name, t in med.items()},
            'over_protein_min': {name: round(t / med['protein_min'], 4) for name, t in med.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=50000)
    ap.add_argument('--families', type=int, default=500)
    ap.add_argument('--family-size', type=int, default=100)
    ap.add_argument('--min-domain', type=float, default=0.5)
    ap.add_argument('--min-coverage', type=float, default=0.8)
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--stripe', type=int, default=8192, help='kernel part: proteins of the row side')
    ap.add_argument('--kernel-repeat', type=int, default=7)
    ap.add_argument('--parent-lib', help='another build of libdctfp.so whose dctfp_protein_min is timed beside this one')
    ap.add_argument('--dir', default=None)
    ap.add_argument('--out')
    args = ap.parse_args()
    import tempfile
    with tempfile.TemporaryDirectory(dir=args.dir) as tmp:
        first, data = part_cluster(args, tmp)
    lines = [first, part_kernel(args, data)]
    for line in lines:
        print(json.dumps(line))
    if args.out:
        with open(args.out, 'a') as fh:
            for line in lines:
                fh.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
