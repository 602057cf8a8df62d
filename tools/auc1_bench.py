"""dct-sim --auc1 on one GPU: the AUC1 run beside the plain cluster run, its device steps, and the two scans alone.

    python tools/auc1_bench.py --part run [--families 500] [--size 100] [--what cluster,auc1_domain,auc1_global] [--package DIR]
                               [--out F.jsonl]
    python tools/auc1_bench.py --part scan [--rows 8192] [--cols 50000] [--out F.jsonl]

Input of `run`: tools/tree_bench.planted -- families x size proteins of 1-8 fingerprints, the members of a family near copies of
its first member, shuffled over the file (500 x 100: the 50 000-protein file of profiles/cluster/), the planted family as the
label.  Timed in one process after a warm-up on a small file, alternating, `--repeats` times:
  cluster       dct_sim.Clusters(min_domain=0.5).labels() and the text to /dev/null;
  auc1_domain   dct_sim.Auc1(score='domain').counts() and the text to /dev/null;
  auc1_global   the same with score='global'.
`--package DIR` takes `dctdomain_amd` from DIR instead of this tree -- another commit's build, for `cluster` only: run the two
alternately, one process each.  Times are host clocks around work that ends in a device synchronise; the split comes from device
events around the calls that fill a tile (protein_min, l1_matrix) and scan it (tri_first_fp, tri_tp_before, tri_link), summed per
run.  Before a time is reported the result is checked: the members of a planted family are nearer to each other than to anybody
else, so every protein has size - 1 true positives before its first false positive -- a mean AUC1 and a Qraw of 1, which the line
records as a sanity number.

`scan` times tri_first_fp and tri_tp_before alone on one int32 tile right of the diagonal, beside tri_degree on the same tile, with
families of 100 over the nodes: `sparse` -- two entries in a thousand within the bound, about what a cut-off leaves of a file of
families -- and `every_entry` (a bound of 17000: every entry is a hit, the case of --auc1 without a cut-off), against the bytes of
the tile.  The results are checked against torch on the tile before anything is timed."""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = {'protein_min': 'tile', 'l1_matrix': 'tile', 'tri_link': 'link', 'tri_first_fp': 'first_fp', 'tri_tp_before': 'tp_before',
         'cluster_labels': 'labels'}


def run(dct_sim, split_cls, what: str, sid, idx, dct, fam):
    import torch
    torch.cuda.synchronize()
    names = {k: v for k, v in STEPS.items() if hasattr(dct_sim, k)}
    with split_cls(dct_sim, names) as split, open(os.devnull, 'wb') as null:
        t0 = time.perf_counter()
        if what == 'cluster':
            job = dct_sim.Clusters(sid, idx, dct, min_domain=0.5)
            result = job.labels()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            job.write(null.write, result)
        else:
            job = dct_sim.Auc1(sid, idx, dct, fam, score=what[len('auc1_'):])
            result = job.counts()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            job.write(null.write)
        seconds = time.perf_counter() - t0
        parts = split.totals()
    row = {'what': what, 'seconds': round(seconds, 4), 'before_text': round(t1 - t0, 4), 'stripes': len(list(job.stripes())),
           'device_seconds': parts}
    if what != 'cluster':
        s = job.summary()
        row.update(mean_auc1=round(s['mean_auc1'], 4), top1_raw=round(s['top1_raw'], 4), top1_norm=round(s['top1_norm'], 4),
                   with_false_positive=int((result[1] >= 0).sum()))
    return row, result


def part_run(args):
    if args.package:
        sys.path.insert(0, os.path.abspath(args.package))
    import torch
    from dctdomain_amd import dct_sim
    from tools.tree_bench import Split, planted
    if not torch.cuda.is_available():
        raise SystemExit('auc1_bench measures on a GPU: none found')
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
                assert (result[0] == args.size - 1).all(), f'{what}: a member of a planted family ranks behind a stranger'
            row.update(package=os.path.dirname(os.path.dirname(os.path.abspath(dct_sim.__file__))), proteins=n, fingerprints=int(idx[-1]),
                       device=torch.cuda.get_device_name(0))
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
    from dctdomain_amd.similarity import BEST_NONE, tri_degree, tri_first_fp, tri_tp_before
    if not torch.cuda.is_available():
        raise SystemExit('auc1_bench measures on a GPU: none found')
    n_rows, n_cols, bound = args.rows, args.cols, 8500
    n = n_rows + n_cols
    gen = torch.Generator(device='cuda').manual_seed(5)
    tile = torch.randint(bound + 1, 17001, (n_rows, n_cols), dtype=torch.int32, device='cuda', generator=gen)
    near = torch.rand((n_rows, n_cols), device='cuda', generator=gen) < 0.002
    tile[near] = torch.randint(0, bound + 1, (int(near.sum().item()),), dtype=torch.int32, device='cuda', generator=gen)
    del near
    place = (tile, 0, n_rows)                                    # (the whole tile is right of the diagonal)
    fam = (torch.randperm(n, device='cuda', generator=gen) // 100).to(torch.int32)
    first = torch.full((n,), BEST_NONE, dtype=torch.int64, device='cuda')
    tp = torch.zeros(n, dtype=torch.int32, device='cuda')
    deg = torch.zeros(n, dtype=torch.int32, device='cuda')
    # checked before anything is timed, on the first rows of the tile: the row ends of both passes against torch
    tri_first_fp(*place, bound, fam, first)
    tri_tp_before(*place, bound, fam, first, tp)
    some = min(n_rows, 256)
    part = tile[:some].to(torch.int64).clamp(max=17000)
    cols = torch.arange(n_rows, n, device='cuda')
    word = part << 32 | cols[None, :]
    hit = part <= bound
    other = fam[:some, None] != fam[None, n_rows:]
    want = torch.where(hit & other, word, torch.full_like(word, 1 << 62)).min(dim=1).values
    got = torch.where(first[:some] == BEST_NONE, torch.full_like(want, 1 << 62), first[:some])
    assert torch.equal(got, want), 'tri_first_fp: not the first false positive of a row'
    assert torch.equal((hit & ~other & (word < got[:, None])).sum(dim=1).to(torch.int32), tp[:some]), 'tri_tp_before: not the count of a row'
    del part, word, hit, other
    with_fp = int((first != BEST_NONE).sum().item())

    def fresh_first():
        first.fill_(BEST_NONE)

    scans = [('tri_degree', 'sparse', lambda: tri_degree(*place, bound, deg), deg.zero_),
             ('tri_first_fp', 'sparse', lambda: tri_first_fp(*place, bound, fam, first), fresh_first),
             ('tri_tp_before', 'sparse', lambda: tri_tp_before(*place, bound, fam, first, tp), tp.zero_),
             ('tri_first_fp', 'every_entry', lambda: tri_first_fp(*place, 17000, fam, first), fresh_first),
             ('tri_tp_before', 'every_entry', lambda: tri_tp_before(*place, 17000, fam, first, tp), tp.zero_)]
    rows = []
    for name, case, call, reset in scans:
        ms, every = _median_ms(call, reset, args.repeats)
        row = {'what': 'scan', 'kernel': name, 'case': case, 'rows': n_rows, 'cols': n_cols, 'tile_bytes': 4 * n_rows * n_cols,
               'families_of': 100, 'with_false_positive': with_fp, 'ms_all': every, 'ms_median': round(ms, 4),
               'tile_GB_per_s': round(4 * n_rows * n_cols / ms / 1e6, 1), 'device': torch.cuda.get_device_name(0)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--part', choices=('run', 'scan'), default='run')
    ap.add_argument('--families', type=int, default=500)
    ap.add_argument('--size', type=int, default=100)
    ap.add_argument('--what', default='cluster,auc1_domain,auc1_global')
    ap.add_argument('--package', default=None)
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
