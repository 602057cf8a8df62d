"""dct-sim --hist on one GPU: the scan alone on spread, crowded and equal keys, and the whole run beside the plain cluster run.

    python tools/hist_bench.py --part scan [--rows 8192] [--cols 50000] [--out F.jsonl]
    python tools/hist_bench.py --part run [--families 500] [--size 100] [--what cluster,hist_domain,hist_global] [--out F.jsonl]

`scan` times tri_hist alone on one int32 tile right of the diagonal, beside tri_degree on the same tile from the same build -- it
reads the same bytes and is the yardstick --, at a bound of 16999 (what --hist asks for), on three inputs:
  spread    keys uniform over 0 .. 16999: every entry is counted, the lanes of a wave hit 64 different counters;
  crowded   keys uniform over a band of 500 values (8000 .. 8499): what the scores of unrelated proteins look like;
  equal     every key 4242: a tile of one planted family -- every lane of every wave adds to one counter;
each with one class (no fam) and with two (families of 100 over the nodes), against the bytes of the tile.  The counts are checked
against torch.bincount on the tile before anything is timed.

Input of `run`: tools/tree_bench.planted -- families x size proteins of 1-8 fingerprints, the members of a family near copies of
its first member, shuffled over the file (500 x 100: the 50 000-protein file of profiles/cluster/), the planted family as the
label.  Timed in one process after a warm-up on a small file, alternating, `--repeats` times:
  cluster       dct_sim.Clusters(min_domain=0.5).labels() and the text to /dev/null;
  hist_domain   dct_sim.Histogram(families, score='domain').counts() and the text to /dev/null;
  hist_global   the same with score='global'.
Times are host clocks around work that ends in a device synchronise; the split comes from device events around the calls that fill
a tile (protein_min, l1_matrix) and scan it (tri_hist, tri_link), summed per run.  Before a time is reported the result is checked:
the pairs of a planted family are nearer than any pair of two, so the ROC AUC is 1 and the best F1 is 1."""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = {'protein_min': 'tile', 'l1_matrix': 'tile', 'tri_link': 'link', 'tri_hist': 'hist', 'cluster_labels': 'labels'}
CAP = 17000


def run(dct_sim, split_cls, what: str, sid, idx, dct, fam):
    import torch
    torch.cuda.synchronize()
    with split_cls(dct_sim, STEPS) as split, open(os.devnull, 'wb') as null:
        t0 = time.perf_counter()
        if what == 'cluster':
            job = dct_sim.Clusters(sid, idx, dct, min_domain=0.5)
            result = job.labels()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            job.write(null.write, result)
        else:
            job = dct_sim.Histogram(sid, idx, dct, fam.tolist(), score=what[len('hist_'):])
            result = job.counts()
            t1 = time.perf_counter()                            # (counts() ends in the copy of the bins: the host has waited)
            job.write(null.write)
        seconds = time.perf_counter() - t0
        parts = split.totals()
    row = {'what': what, 'seconds': round(seconds, 4), 'before_text': round(t1 - t0, 4), 'stripes': len(list(job.stripes())),
           'device_seconds': parts}
    if what != 'cluster':
        s = job.summary()
        row.update(pairs=s['pairs'], same=s['same'], scored=int(result[0].sum()), roc_auc=round(s['roc_auc'], 6), best_f1=round(s['best_f1'], 6),
                   at=s['at'])
    return row, result


def part_run(args):
    import torch
    from dctdomain_amd import dct_sim
    from tools.tree_bench import Split, planted
    if not torch.cuda.is_available():
        raise SystemExit('hist_bench measures on a GPU: none found')
    whats = args.what.split(',')
    sid, idx, dct, fam = planted(args.families, args.size)
    n = len(sid)
    small = planted(20, 10)
    for what in whats:                                           # warm-up: code objects loaded, the allocator primed
        run(dct_sim, Split, what, *small)
    first = np.full(args.families, n)
    np.minimum.at(first, fam, np.arange(n))
    rows = []
    for _ in range(args.repeats):
        for what in whats:
            row, result = run(dct_sim, Split, what, sid, idx, dct, fam)
            if what == 'cluster':
                assert np.array_equal(result, first[fam]), 'cluster: not the planted families'
            else:
                assert row['roc_auc'] == 1.0 and row['best_f1'] == 1.0, f'{what}: a pair of two families scores above a pair of one'
                assert row['same'] == args.families * args.size * (args.size - 1) // 2 and int(result[1][0]) == 0
            row.update(proteins=n, fingerprints=int(idx[-1]), device=torch.cuda.get_device_name(0))
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def _median_ms(call, reset, repeats: int):
    import torch
    times = []
    for _ in range(repeats + 1):
        reset()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return sorted(times[1:])[len(times[1:]) // 2], [round(t, 4) for t in times[1:]]


def part_scan(args):
    import torch
    from dctdomain_amd.similarity import tri_degree, tri_hist
    if not torch.cuda.is_available():
        raise SystemExit('hist_bench measures on a GPU: none found')
    n_rows, n_cols, bound = args.rows, args.cols, CAP - 1
    n = n_rows + n_cols
    gen = torch.Generator(device='cuda').manual_seed(5)
    fam = (torch.randperm(n, device='cuda', generator=gen) // 100).to(torch.int32)
    deg = torch.zeros(n, dtype=torch.int32, device='cuda')
    hists = {1: torch.zeros((1, CAP + 1), dtype=torch.int64, device='cuda'), 2: torch.zeros((2, CAP + 1), dtype=torch.int64, device='cuda')}
    tile = torch.empty((n_rows, n_cols), dtype=torch.int32, device='cuda')
    place = (tile, 0, n_rows)                                    # (the whole tile is right of the diagonal)
    fills = {'spread': lambda: tile.random_(0, CAP, generator=gen), 'crowded': lambda: tile.random_(8000, 8500, generator=gen),
             'equal': lambda: tile.fill_(4242)}
    rows = []
    for case, fill in fills.items():
        fill()
        # checked before anything is timed: both class rows against torch.bincount on the tile
        other = (fam[:n_rows, None] != fam[None, n_rows:]).reshape(-1)
        want = torch.bincount(tile.reshape(-1).to(torch.int64) + other * (CAP + 1), minlength=2 * (CAP + 1)).reshape(2, CAP + 1)
        del other
        for classes, hist in hists.items():
            hist.zero_()
            tri_hist(*place, bound, hist, fam if classes == 2 else None)
            assert torch.equal(hist, want if classes == 2 else want.sum(dim=0, keepdim=True)), f'tri_hist: not the counts of the {case} tile'
        scans = [('tri_degree', 0, lambda: tri_degree(*place, bound, deg), deg.zero_),
                 ('tri_hist', 1, lambda: tri_hist(*place, bound, hists[1]), hists[1].zero_),
                 ('tri_hist', 2, lambda: tri_hist(*place, bound, hists[2], fam), hists[2].zero_)]
        for name, classes, call, reset in scans:
            ms, every = _median_ms(call, reset, args.repeats)
            row = {'what': 'scan', 'kernel': name, 'case': case, 'classes': classes, 'rows': n_rows, 'cols': n_cols,
                   'tile_bytes': 4 * n_rows * n_cols, 'distinct_keys': int((want.sum(dim=0) > 0).sum().item()), 'ms_all': every,
                   'ms_median': round(ms, 4), 'tile_GB_per_s': round(4 * n_rows * n_cols / ms / 1e6, 1),
                   'device': torch.cuda.get_device_name(0)}
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--part', choices=('run', 'scan'), default='scan')
    ap.add_argument('--families', type=int, default=500)
    ap.add_argument('--size', type=int, default=100)
    ap.add_argument('--what', default='cluster,hist_domain,hist_global')
    ap.add_argument('--rows', type=int, default=8192)
    ap.add_argument('--cols', type=int, default=50000)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    rows = part_run(args) if args.part == 'run' else part_scan(args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as fh:
            for row in rows:
                fh.write(json.dumps(row) + '\n')


if __name__ == '__main__':
    main()
