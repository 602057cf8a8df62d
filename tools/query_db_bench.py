"""query_db at database scale (QuerySearch: dctfp_l1_knn + dctfp_query_rank + dctfp_query_lines): times on synthetic data.

    python tools/query_db_bench.py --part kernels [--db 200000 --queries 2000]        # l1_knn vs l1_matrix + row_select
    python tools/query_db_bench.py --part search  [--db 1000000 --queries 10000]      # end to end after the load, text to /dev/null
    python tools/query_db_bench.py --part old     [--old-db 100000 --old-queries 1000]  # query_db.search() vs QuerySearch, bytes compared

Each part is its own process (run each under its own time limit).  Data: tools/protein_search_bench.py's synth / plant (1-12
domains + the whole protein per protein, planted near-duplicates).  Prints one JSON line per part; --out appends it to a file.
Kernel fractions are taken against the v_sad_u8 peak: 157e12 byte differences per second."""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.protein_search_bench import _events_ms, peak_rss_gb, plant, synth, sync  # noqa: E402

SAD_PEAK = 157e12        # byte differences per second


def _tables(n_q, n_db, seed):
    from dctdomain_amd.query_db import Table
    q_idx, q_dct = synth(n_q, seed)
    idx, dct = synth(n_db, seed + 1)
    plant(q_idx, q_dct, idx, dct, 0.05, seed + 2)

    def table(pidx, fps, tag):
        counts = np.diff(pidx)
        pids = [f'{tag}{p}' for p in range(len(counts)) for _ in range(counts[p])]
        doms = [f'1-{j + 10}' for p in range(len(counts)) for j in range(counts[p])]
        return Table(pids, doms, fps)
    return table(q_idx, q_dct, 'Q'), table(idx, dct, 'D')


def part_kernels(a):
    """Both routes of QuerySearch on the same shapes, interleaved: dctfp_l1_knn, and l1_matrix + row_select on tiles of at most
    query_db.TILE_INTS distances (what QuerySearch(knn='matrix') runs; the selected pairs come back to the host there)."""
    import torch
    from dctdomain_amd import query_db
    from dctdomain_amd.similarity import l1_knn_device
    rng = np.random.default_rng(1)
    res = {'part': 'kernels', 'configs': []}
    b = torch.from_numpy(rng.integers(-48, 49, size=(a.db, 480), dtype=np.int8)).cuda()
    qs = query_db.QuerySearch.__new__(query_db.QuerySearch)          # (only its two routes: no tables)
    qs.dev, qs.knn = b.device, 'matrix'
    for nq in (5, 640, 2000, 8000, 20000):
        q = torch.from_numpy(rng.integers(-48, 49, size=(nq, 480), dtype=np.int8)).cuda()
        for k in (100, 1024):
            knn = lambda: l1_knn_device(q, b, k)
            old = lambda: qs._block_knn(q, b, k, 0)
            t_new, t_old = [], []
            for _ in range(2):                                      # interleaved
                t_new.append(_events_ms(knn, 1))
                t_old.append(_events_ms(old, 1))
            ms_new, ms_old = min(t_new), min(t_old)
            res['configs'].append({'nq': nq, 'nb': a.db, 'k': k, 'l1_knn_ms': round(ms_new, 3), 'matrix_route_ms': round(ms_old, 3),
                                   'l1_knn_sad_fraction': round(nq * a.db * 480 / (ms_new * 1e-3) / SAD_PEAK, 3)})
            print(json.dumps(res['configs'][-1]), flush=True)
    return res


def part_search(a):
    from dctdomain_amd.query_db import QuerySearch
    t0 = time.perf_counter()
    qt, dt = _tables(a.queries, a.db, 5)      # (synthetic arrays + Table: the per-row Python of the loader, not the .db read)
    t_tables = time.perf_counter() - t0
    t0 = time.perf_counter()
    qs = QuerySearch(dt, knn=a.knn)
    sync()
    t_load = time.perf_counter() - t0
    stats = {'bytes': 0}
    with open(os.devnull, 'wb') as sink:
        def write(data):
            stats['bytes'] += len(data)
            sink.write(data)
        t0 = time.perf_counter()
        qs.search(qt, a.khits, write)
        t_search = time.perf_counter() - t0
    return {'part': 'search', 'knn': a.knn, 'queries': a.queries, 'db': a.db, 'query_fps': qt.n, 'db_fps': dt.n, 'khits': a.khits,
            'tables_s': round(t_tables, 3), 'upload_s': round(t_load, 3), 'search_s': round(t_search, 3), 'bytes': stats['bytes'], 'peak_rss_gb': round(peak_rss_gb(), 2)}


def part_old(a):
    from dctdomain_amd import query_db
    qt, dt = _tables(a.old_queries, a.old_db, 7)

    def rows(t):
        p = [t.pid[t.pid_off[i]:t.pid_off[i + 1]].decode() for i in range(t.n)]
        d = [t.dom[t.dom_off[i]:t.dom_off[i + 1]].decode() for i in range(t.n)]
        return [(i, p[i], d[i]) for i in range(t.n)]
    qrows, drows = rows(qt), rows(dt)
    t0 = time.perf_counter()
    old = ''.join(line + '\n' for line in query_db.search(qrows, qt.fps, drows, dt.fps, a.khits)).encode('utf8')
    t_old = time.perf_counter() - t0
    out = []
    t0 = time.perf_counter()
    query_db.QuerySearch(dt).search(qt, a.khits, out.append)
    new = b''.join(out)
    t_new = time.perf_counter() - t0
    return {'part': 'old', 'queries': a.old_queries, 'db': a.old_db, 'khits': a.khits, 'old_s': round(t_old, 3), 'new_s': round(t_new, 3),
            'lines': old.count(b'\n'), 'bytes': len(old), 'identical': old == new}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--part', choices=('kernels', 'search', 'old'), required=True)
    ap.add_argument('--db', type=int, default=1_000_000, help='database proteins (kernels: database fingerprints)')
    ap.add_argument('--queries', type=int, default=10_000)
    ap.add_argument('--old-db', type=int, default=100_000)
    ap.add_argument('--old-queries', type=int, default=1_000)
    ap.add_argument('--khits', type=int, default=100)
    ap.add_argument('--knn', choices=('auto', 'fused', 'matrix'), default='auto', help='search: the k-nearest route of QuerySearch')
    ap.add_argument('--out', help='append the JSON line here too')
    a = ap.parse_args(argv)
    res = {'kernels': part_kernels, 'search': part_search, 'old': part_old}[a.part](a)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, 'a') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
