"""Protein-level search at database scale (dct-sim --db / --pair without the block matrix): times and memory on synthetic data.

    python tools/protein_search_bench.py --part search  [--db 1000000 --queries 10000]   # db_search, end to end after the load
    python tools/protein_search_bench.py --part kernels [--db 1000000]                    # selection kernels, dctfp_pair_min
    python tools/protein_search_bench.py --part blocks  [--old-db 100000 --old-queries 2000]  # the block-matrix path, and the new one
    python tools/protein_search_bench.py --part argmin  [--db 1000000 --repeat 5]         # dctfp_pair_argmin beside dctfp_pair_min
    python tools/protein_search_bench.py --part rowbest [--db 1000000 --repeat 5]         # dctfp_pair_row_best beside dctfp_pair_argmin

Each part is its own process (run each under its own time limit).  Data: random int8 fingerprints, 1-12 domains + the whole
protein per protein, values in [-48, 48] (unrelated proteins at L1 ~ 15 000: similarity 0.1, below the 0.25 threshold) and
a planted fraction of near-duplicates (last rows within a few units per byte of a query's) so that threshold hits exist.
Prints one JSON line per part; --out appends it to a file."""

from __future__ import annotations

import argparse
import json
import os
import resource
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12        # B/s, MI355X spec (MI355X_MICROARCH: 6.3 TB/s achievable)


def synth(n_prot: int, seed: int, max_dom: int = 12):
    rng = np.random.default_rng(seed)
    counts = rng.integers(1, max_dom + 1, size=n_prot) + 1           # domains + the whole protein
    idx = np.zeros(n_prot + 1, dtype=np.int64)
    np.cumsum(counts, out=idx[1:])
    dct = rng.integers(-48, 49, size=(int(idx[-1]), 480), dtype=np.int8)
    return idx, dct


def plant(q_idx, q_dct, idx, dct, frac: float, seed: int):
    """Near-duplicates of a fraction of the queries: 1-8 database proteins each get a last row within +-9 per byte."""
    rng = np.random.default_rng(seed)
    nq = len(q_idx) - 1
    chosen = rng.choice(nq, size=max(1, int(frac * nq)), replace=False)
    for q in chosen:
        base = q_dct[q_idx[q + 1] - 1].astype(np.int16)
        for t in rng.choice(len(idx) - 1, size=int(rng.integers(1, 9)), replace=False):
            dct[idx[t + 1] - 1] = np.clip(base + rng.integers(-9, 10, size=480), -128, 127)
    return len(chosen)


def peak_rss_gb() -> float:
    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2 ** 20


def sync():
    import torch
    torch.cuda.synchronize()


def part_search(a):
    from dctdomain_amd import dct_sim
    t0 = time.time()
    idx, dct = synth(a.db, 1)
    q_idx, q_dct = synth(a.queries, 2)
    n_planted = plant(q_idx, q_dct, idx, dct, a.planted, 3)
    t_gen = time.time() - t0
    rss_data = peak_rss_gb()
    res = {}
    for rep in ('warm', 'timed'):
        sync()
        t0 = time.time()
        search = dct_sim.ProteinSearch(dct, idx)
        hits = search.search(q_dct, q_idx, a.top, a.threshold)
        t_search = time.time() - t0
        n_lines = 0
        with open(os.devnull, 'w') as null:       # the printing of db_search: the same f-strings, to nowhere
            for qi, (cols, mn, last) in enumerate(hits):
                for q, m, l in zip(cols, mn, last):
                    maxs, s = dct_sim._scores(m, l)
                    null.write(f'q{qi} d{q} {maxs} {s}\n')
                    n_lines += 1
        t_total = time.time() - t0
        res[rep] = (t_search, t_total, n_lines)
        del search, hits
    t_search, t_total, n_lines = res['timed']
    return {'part': 'search', 'db_proteins': a.db, 'db_fingerprints': int(idx[-1]), 'queries': a.queries,
            'query_fingerprints': int(q_idx[-1]), 'planted_queries': n_planted, 'top': a.top, 'threshold': a.threshold,
            'groups': len(dct_sim.ProteinSearch(dct, idx).groups), 'search_s': round(t_search, 3),
            'db_search_s': round(t_total, 3), 'lines': n_lines, 'whole_protein_pairs_per_s': a.db * a.queries / t_search,
            'peak_rss_gb_after_data': round(rss_data, 2), 'peak_rss_gb': round(peak_rss_gb(), 2),
            'data_bytes_gb': round((dct.nbytes + q_dct.nbytes) / 2 ** 30, 2), 'generate_s': round(t_gen, 1)}


def _events_ms(fn, reps: int):
    import torch
    fn()
    sync()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    sync()
    return e0.elapsed_time(e1) / reps


def part_kernels(a):
    import ctypes as C
    import torch
    from dctdomain_amd import _lib, dct_sim
    from dctdomain_amd.similarity import l1_matrix, pair_min, to_device_int8
    idx, dct = synth(a.db, 1)
    q_idx, q_dct = synth(a.queries, 2)
    plant(q_idx, q_dct, idx, dct, a.planted, 3)
    last, empty = dct_sim._last_rows(dct, idx)
    q_last, _ = dct_sim._last_rows(q_dct, q_idx)
    dev = torch.device('cuda')
    rows = min(len(q_last), dct_sim.ProteinSearch.TILE_INTS // a.db)
    last_d = to_device_int8(last)
    tile = l1_matrix(q_last[:rows], last_d)
    ctx = _lib.get_context(0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    bound = dct_sim.sim_bound(a.threshold)
    empty_d = torch.as_tensor(empty, device=dev)
    count = torch.empty(rows, dtype=torch.int32, device=dev)
    cut = torch.empty((rows, 2), dtype=torch.int32, device=dev)

    def run_count():
        _lib.check(ctx._lib.dctfp_select_count(ctx.handle, tile.data_ptr(), rows, a.db, a.db, None, empty_d.data_ptr(), 17000, bound,
                                               a.top, count.data_ptr(), cut.data_ptr(), stream))
    ms_count = _events_ms(run_count, 5)
    m = count.cpu().numpy().astype(np.int64)
    off = np.concatenate([[0], np.cumsum(m)])
    off_d = torch.as_tensor(off, device=dev)
    key = torch.empty(int(off[-1]), dtype=torch.int32, device=dev)
    col = torch.empty_like(key)

    def run_fill():
        _lib.check(ctx._lib.dctfp_select_fill(ctx.handle, tile.data_ptr(), rows, a.db, a.db, None, empty_d.data_ptr(), 17000, cut.data_ptr(),
                                              off_d.data_ptr(), int(m.max()), key.data_ptr(), col.data_ptr(), stream))
    ms_fill = _events_ms(run_fill, 5)
    q_last_d = to_device_int8(q_last[:rows])
    ms_l1 = _events_ms(lambda: l1_matrix(q_last_d, last_d), 3)
    tile_bytes = rows * a.db * 4
    # dctfp_pair_min: random (query, database protein) pairs, gathered reads of both proteins' fingerprints
    rng = np.random.default_rng(7)
    n_pairs = a.pairs
    pairs = np.stack([rng.integers(0, len(q_idx) - 1, size=n_pairs), rng.integers(0, a.db, size=n_pairs)], axis=1)
    da, db = to_device_int8(q_dct), to_device_int8(dct)
    ia_d, ib_d = torch.as_tensor(q_idx, device=dev), torch.as_tensor(idx, device=dev)
    pairs_d = torch.as_tensor(pairs.astype(np.int32), device=dev)
    mn = torch.empty(n_pairs, dtype=torch.int32, device=dev)
    lst = torch.empty_like(mn)

    def run_pairs():
        _lib.check(ctx._lib.dctfp_pair_min(ctx.handle, pairs_d.data_ptr(), n_pairs, da.data_ptr(), 480, ia_d.data_ptr(), len(q_idx) - 1,
                                           db.data_ptr(), 480, ib_d.data_ptr(), a.db, 480, mn.data_ptr(), lst.data_ptr(), stream))
    ms_pairs = _events_ms(run_pairs, 5)
    na = (q_idx[pairs[:, 0] + 1] - q_idx[pairs[:, 0]])
    nb = (idx[pairs[:, 1] + 1] - idx[pairs[:, 1]])
    pair_bytes = int(((na + nb) * 480).sum())                 # each fingerprint of both proteins read once per pair
    sad_bytes = int((na * nb * 480).sum())                    # bytes through v_sad_u8 (per operand)
    # spot check against numpy
    k = rng.integers(0, n_pairs, size=20)
    got_mn, got_last = pair_min(da, q_idx, db, idx, pairs[k])
    for t, (i, j) in enumerate(pairs[k]):
        blk = np.abs(q_dct[q_idx[i]:q_idx[i + 1]].astype(np.int16)[:, None] - dct[idx[j]:idx[j + 1]].astype(np.int16)[None]).sum(-1)
        assert got_mn[t] == blk.min() and got_last[t] == blk[-1, -1]
    return {'part': 'kernels', 'tile_rows': rows, 'tile_cols': a.db, 'tile_gib': round(tile_bytes / 2 ** 30, 3),
            'l1_tile_ms': round(ms_l1, 3), 'select_count_ms': round(ms_count, 3), 'select_fill_ms': round(ms_fill, 3),
            'select_count_tb_s': tile_bytes / ms_count / 1e9, 'select_fill_tb_s': tile_bytes / ms_fill / 1e9,
            'hits_in_tile': int(off[-1]), 'pairs': n_pairs, 'pair_min_ms': round(ms_pairs, 3),
            'pair_min_pairs_per_s': n_pairs / ms_pairs * 1e3, 'pair_min_bytes_per_pair': pair_bytes / n_pairs,
            'pair_min_tb_s': pair_bytes / ms_pairs / 1e9, 'pair_min_share_of_hbm_peak': pair_bytes / ms_pairs / 1e9 / (HBM_PEAK / 1e12),
            'pair_min_sad_gb_s': sad_bytes / ms_pairs / 1e6}


def part_argmin(a):
    """dctfp_pair_argmin beside dctfp_pair_min on the 1 M random pairs of `kernels` (the same data, seeds and launch arguments), in
    one process: --repeat rounds of (pair_min x 5, pair_argmin x 5), so that each list shows the run-to-run spread of its kernel
    under the same conditions; every pair's outputs compared between the two, a sample against numpy."""
    import ctypes as C
    import torch
    from dctdomain_amd import _lib
    from dctdomain_amd.similarity import to_device_int8
    idx, dct = synth(a.db, 1)
    q_idx, q_dct = synth(a.queries, 2)
    plant(q_idx, q_dct, idx, dct, a.planted, 3)
    dev = torch.device('cuda')
    ctx = _lib.get_context(0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(7)
    n_pairs = a.pairs
    pairs = np.stack([rng.integers(0, len(q_idx) - 1, size=n_pairs), rng.integers(0, a.db, size=n_pairs)], axis=1)
    da, db = to_device_int8(q_dct), to_device_int8(dct)
    ia_d, ib_d = torch.as_tensor(q_idx, device=dev), torch.as_tensor(idx, device=dev)
    pairs_d = torch.as_tensor(pairs.astype(np.int32), device=dev)
    out = [torch.empty(n_pairs, dtype=torch.int32, device=dev) for _ in range(6)]
    head = (ctx.handle, pairs_d.data_ptr(), n_pairs, da.data_ptr(), 480, ia_d.data_ptr(), len(q_idx) - 1, db.data_ptr(), 480, ib_d.data_ptr(),
            a.db, 480)

    def run_min():
        _lib.check(ctx._lib.dctfp_pair_min(*head, out[0].data_ptr(), out[1].data_ptr(), stream))

    def run_argmin():
        _lib.check(ctx._lib.dctfp_pair_argmin(*head, out[2].data_ptr(), out[3].data_ptr(), out[4].data_ptr(), out[5].data_ptr(), stream))
    ms_min, ms_arg = [], []
    for _ in range(a.repeat):
        ms_min.append(round(_events_ms(run_min, 5), 4))
        ms_arg.append(round(_events_ms(run_argmin, 5), 4))
    mn, last, mn2, last2, arg_a, arg_b = (t.cpu().numpy().astype(np.int64) for t in out)
    assert np.array_equal(mn, mn2) and np.array_equal(last, last2)
    assert np.array_equal(arg_a < 0, mn >= 17000) and np.array_equal(arg_b < 0, mn >= 17000)
    for t in rng.integers(0, n_pairs, size=50).tolist() + np.flatnonzero(mn < 17000)[:50].tolist():
        i, j = pairs[t]
        blk = np.abs(q_dct[q_idx[i]:q_idx[i + 1]].astype(np.int16)[:, None] - dct[idx[j]:idx[j + 1]].astype(np.int16)[None]).sum(-1)
        want = divmod(int(np.argmin(blk)), blk.shape[1]) if blk.min() < 17000 else (-1, -1)
        assert mn[t] == blk.min() and (arg_a[t], arg_b[t]) == want
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    return {'part': 'argmin', 'pairs': n_pairs, 'db': a.db, 'pairs_with_a_domain_pair': int((arg_a >= 0).sum()), 'pair_min_ms': ms_min,
            'pair_argmin_ms': ms_arg, 'pair_min_median_ms': med(ms_min), 'pair_argmin_median_ms': med(ms_arg),
            'pair_min_spread_ms': round(max(ms_min) - min(ms_min), 4), 'argmin_over_min': round(med(ms_arg) / med(ms_min), 4),
            'argmin_within_pair_min_spread': med(ms_arg) <= med(ms_min) + (max(ms_min) - min(ms_min))}


def part_rowbest(a):
    """dctfp_pair_row_best beside dctfp_pair_argmin on the 1 M random pairs of `argmin` (the same data, seeds and launch arguments),
    in one process: --repeat rounds of (pair_argmin x 5, pair_row_best x 5) after a warm-up of both; the best first-side entry of
    every pair compared with pair_argmin's, a sample against numpy.  Under `rocprofv3 --kernel-trace --stats` the kernel times are
    the profiler's; the times printed here are hipEvents around five launches."""
    import ctypes as C
    import torch
    from dctdomain_amd import _lib
    from dctdomain_amd.similarity import pair_row_offsets, to_device_int8
    idx, dct = synth(a.db, 1)
    q_idx, q_dct = synth(a.queries, 2)
    plant(q_idx, q_dct, idx, dct, a.planted, 3)
    dev = torch.device('cuda')
    ctx = _lib.get_context(0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(7)
    n_pairs = a.pairs
    pairs = np.stack([rng.integers(0, len(q_idx) - 1, size=n_pairs), rng.integers(0, a.db, size=n_pairs)], axis=1)
    off = pair_row_offsets(q_idx, idx, pairs)
    rows = int(off[-1])
    da, db = to_device_int8(q_dct), to_device_int8(dct)
    ia_d, ib_d, off_d = (torch.as_tensor(v, device=dev) for v in (q_idx, idx, off))
    pairs_d = torch.as_tensor(pairs.astype(np.int32), device=dev)
    out = [torch.empty(n_pairs, dtype=torch.int32, device=dev) for _ in range(4)]
    l1_d, arg_d = (torch.full((rows,), -7, dtype=torch.int32, device=dev) for _ in range(2))
    head = (ctx.handle, pairs_d.data_ptr(), n_pairs, da.data_ptr(), 480, ia_d.data_ptr(), len(q_idx) - 1, db.data_ptr(), 480, ib_d.data_ptr(),
            a.db, 480)

    def run_argmin():
        _lib.check(ctx._lib.dctfp_pair_argmin(*head, *(t.data_ptr() for t in out), stream))

    def run_best():
        _lib.check(ctx._lib.dctfp_pair_row_best(*head, off_d.data_ptr(), rows, l1_d.data_ptr(), arg_d.data_ptr(), stream))
    run_argmin()
    run_best()
    sync()
    ms_arg, ms_best = [], []
    for _ in range(a.repeat):
        ms_arg.append(round(_events_ms(run_argmin, 5), 4))
        ms_best.append(round(_events_ms(run_best, 5), 4))
    mn, _, arg_a, arg_b = (t.cpu().numpy().astype(np.int64) for t in out)
    l1, arg = l1_d.cpu().numpy().astype(np.int64), arg_d.cpu().numpy().astype(np.int64)
    assert (l1 >= 0).all() and (arg >= 0).all()                 # (every protein has rows: every entry was written)
    k = q_idx[pairs[:, 0] + 1] - q_idx[pairs[:, 0]]
    assert np.array_equal(np.minimum.reduceat(l1, off[:-1]), mn)      # (the smallest entry of a pair, on either side, is its minimum)
    for t in rng.integers(0, n_pairs, size=200).tolist():
        i, j = pairs[t]
        blk = np.abs(q_dct[q_idx[i]:q_idx[i + 1]].astype(np.int16)[:, None] - dct[idx[j]:idx[j + 1]].astype(np.int16)[None]).sum(-1)
        assert l1[off[t]:off[t] + k[t]].tolist() == blk.min(1).tolist() and arg[off[t]:off[t] + k[t]].tolist() == blk.argmin(1).tolist()
        assert l1[off[t] + k[t]:off[t + 1]].tolist() == blk.min(0).tolist() and arg[off[t] + k[t]:off[t + 1]].tolist() == blk.argmin(0).tolist()
        r = int(np.argmin(l1[off[t]:off[t] + k[t]]))
        assert mn[t] == blk.min() and (mn[t] >= 17000 or (arg_a[t], arg_b[t]) == (r, arg[off[t] + r]))
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    return {'part': 'rowbest', 'pairs': n_pairs, 'db': a.db, 'rows_written': rows, 'pair_argmin_ms': ms_arg, 'pair_row_best_ms': ms_best,
            'pair_argmin_median_ms': med(ms_arg), 'pair_row_best_median_ms': med(ms_best),
            'pair_argmin_spread_ms': round(max(ms_arg) - min(ms_arg), 4), 'row_best_over_argmin': round(med(ms_best) / med(ms_arg), 4)}


def part_blocks(a):
    import torch
    from dctdomain_amd import dct_sim
    idx, dct = synth(a.old_db, 1)
    q_idx, q_dct = synth(a.old_queries, 2)
    plant(q_idx, q_dct, idx, dct, a.planted, 3)
    out = {'part': 'blocks', 'db_proteins': a.old_db, 'queries': a.old_queries}
    with tempfile.TemporaryDirectory() as tmp:
        qf, dbf = os.path.join(tmp, 'q-dct.npz'), os.path.join(tmp, 'db-dct.npz')
        np.savez(qf, sid=np.array([f'q{i}' for i in range(a.old_queries)]), idx=q_idx, dom=np.array(['1-9']), dct=q_dct)
        np.savez(dbf, sid=np.array([f'd{i}' for i in range(a.old_db)]), idx=idx, dom=np.array(['1-9']), dct=dct)
        dct_sim.ProteinSearch(dct, idx).search(q_dct[:q_idx[8]], q_idx[:9], a.top, a.threshold)     # (warm-up of every kernel)
        blk = dct_sim.Blocks(qf, dbf)
        del blk
        torch.cuda.synchronize()
        outs = {}
        for name in ('new', 'old'):
            t0 = time.time()
            path = os.path.join(tmp, f'{name}.txt')
            if name == 'new':
                dct_sim.db_search(qf, dbf, a.top, a.threshold, path)
            else:
                blk = dct_sim.Blocks(qf, dbf)
                t_blocks = time.time() - t0
                glob = dct_sim._sim(blk.last)
                with open(path, 'w') as fh:
                    fh.write(dct_sim.HEADER + '\n')
                    for i, query in enumerate(blk.rows):
                        order = np.argsort(-glob[i], kind='stable')
                        for rank, q in enumerate(order):
                            if rank >= a.top and glob[i, q] < a.threshold:
                                break
                            maxs, s = blk.scores(i, q)
                            fh.write(f'{query} {blk.cols[q]} {maxs} {s}\n')
                out['blocks_init_s'] = round(t_blocks, 3)
                del blk, glob
            out[f'{name}_db_search_s'] = round(time.time() - t0, 3)
            outs[name] = open(path).read()
        out['identical_output'] = outs['new'] == outs['old']
        out['lines'] = outs['new'].count('\n') - 1
    out['peak_rss_gb'] = round(peak_rss_gb(), 2)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--part', choices=('search', 'kernels', 'blocks', 'argmin', 'rowbest'), required=True)
    ap.add_argument('--repeat', type=int, default=5, help='argmin / rowbest: rounds of both kernels')
    ap.add_argument('--db', type=int, default=1_000_000)
    ap.add_argument('--queries', type=int, default=10_000)
    ap.add_argument('--old-db', type=int, default=100_000)
    ap.add_argument('--old-queries', type=int, default=2_000)
    ap.add_argument('--pairs', type=int, default=1_000_000)
    ap.add_argument('--planted', type=float, default=0.05, help='fraction of queries with near-duplicates in the database')
    ap.add_argument('--top', type=int, default=5)
    ap.add_argument('--threshold', type=float, default=0.25)
    ap.add_argument('--out', help='append the JSON line here too')
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('protein_search_bench needs the GPU')
    res = {'search': part_search, 'kernels': part_kernels, 'blocks': part_blocks, 'argmin': part_argmin, 'rowbest': part_rowbest}[a.part](a)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, 'a') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
