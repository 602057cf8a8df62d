"""Times dct-sim --db --rank domain's hot path on one GPU.

1. ``dctfp_protein_min`` against ``dctfp_l1_matrix`` + ``dctfp_block_min`` on identical inputs (default 45 000 x 450 000
   fingerprint rows, 4-5 per protein, 480 bytes each).  The composition runs in column groups whose distance matrix holds
   at most 2^28 int32 (1 GiB), as ``Blocks`` tiles it; the fused kernel in one call.  Both outputs are compared.
2. ``ProteinSearch.search`` with rank='domain' against rank='global' at 10 000 query proteins x 1 M database proteins of
   synthetic fingerprints, after the load (the arrays are in memory; no npz is read).

    python tools/protein_min_bench.py [--rows-a 45000 --rows-b 450000] [--queries 10000 --db 1000000] [--skip-search]

Prints one JSON line per measurement.  Rates: byte differences per second against the v_sad_u8 peak (256 CUs x 64 lanes x
4 per clock at 2.4 GHz = 157 x 10^12/s)."""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SAD_PEAK = 256 * 64 * 4 * 2.4e9


def _ragged(rng, n_rows_target, d=480):
    counts = rng.integers(4, 6, size=int(n_rows_target / 4.5) + 1)
    idx = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    keep = int(np.searchsorted(idx, n_rows_target, 'right')) - 1
    idx = idx[:keep + 1]
    return rng.integers(-48, 49, size=(int(idx[-1]), d), dtype=np.int8), idx


def _timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), times


def kernel_vs_composition(rows_a, rows_b, reps):
    import torch
    from dctdomain_amd.dct_sim import _protein_groups
    from dctdomain_amd.similarity import block_min_device, l1_matrix, protein_min, to_device_int8
    rng = np.random.default_rng(1)
    a, ia = _ragged(rng, rows_a)
    b, ib = _ragged(rng, rows_b)
    ta, tb = to_device_int8(a), to_device_int8(b)
    npa, npb = len(ia) - 1, len(ib) - 1
    fused = torch.empty((npa, npb), dtype=torch.int32, device=ta.device)
    comp = torch.empty_like(fused)
    groups = list(_protein_groups(ib, max(1, (1 << 28) // len(a))))

    def run_fused():
        protein_min(ta, ia, tb, ib, out=fused)

    def run_comp():
        for q0, q1 in groups:
            comp[:, q0:q1] = block_min_device(l1_matrix(ta, tb[ib[q0]:ib[q1]]), ia, ib[q0:q1 + 1] - ib[q0])[0]

    t_f, all_f = _timed(run_fused, reps)
    t_c, all_c = _timed(run_comp, reps)
    equal = bool(torch.equal(fused, comp))
    diffs = float(len(a)) * len(b) * a.shape[1]
    return {'what': 'protein_min_vs_l1_matrix_block_min', 'rows_a': len(a), 'rows_b': len(b), 'proteins_a': npa, 'proteins_b': npb,
            'd': a.shape[1], 'fused_s': t_f, 'composed_s': t_c, 'fused_over_composed': t_f / t_c,
            'fused_diffs_per_s': diffs / t_f, 'fused_of_sad_peak': diffs / t_f / SAD_PEAK, 'composed_groups': len(groups),
            'identical': equal, 'fused_runs_s': all_f, 'composed_runs_s': all_c}


def search_modes(n_q, n_db, reps):
    from dctdomain_amd.dct_sim import ProteinSearch
    rng = np.random.default_rng(2)
    q, qi = _ragged(rng, int(n_q * 4.5))
    db, di = _ragged(rng, int(n_db * 4.5))
    out = {'what': 'dct_sim_db_search_after_load', 'query_proteins': len(qi) - 1, 'db_proteins': len(di) - 1,
           'query_rows': len(q), 'db_rows': len(db), 'top': 5, 'threshold': 0.25}
    for rank in ('global', 'domain'):
        search = ProteinSearch(db, di)
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            hits = search.search(q, qi, 5, 0.25, rank=rank)
            times.append(time.perf_counter() - t0)
        out[f'{rank}_s'] = float(np.median(times))
        out[f'{rank}_runs_s'] = times
        out[f'{rank}_lines'] = int(sum(len(h[0]) for h in hits))
    out['domain_over_global'] = out['domain_s'] / out['global_s']
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rows-a', type=int, default=45_000)
    ap.add_argument('--rows-b', type=int, default=450_000)
    ap.add_argument('--queries', type=int, default=10_000)
    ap.add_argument('--db', type=int, default=1_000_000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--skip-search', action='store_true')
    ap.add_argument('--skip-kernel', action='store_true')
    args = ap.parse_args(argv)
    if not args.skip_kernel:
        print(json.dumps(kernel_vs_composition(args.rows_a, args.rows_b, args.reps)), flush=True)
    if not args.skip_search:
        print(json.dumps(search_modes(args.queries, args.db, args.reps)), flush=True)


if __name__ == '__main__':
    main()
