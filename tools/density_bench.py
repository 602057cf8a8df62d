"""dct-sim --cluster --min-neighbors on one GPU: the density run beside the plain cluster run, its device steps, and the two scans alone.

    python tools/density_bench.py --part run [--families 500] [--size 100] [--what cluster,density] [--neighbors 5] [--package DIR]
                                  [--out F.jsonl]
    python tools/density_bench.py --part scan [--rows 8192] [--cols 50000] [--out F.jsonl]

Input of `run`: tools/tree_bench.planted -- families x size proteins of 1-8 fingerprints, the members of a family near copies of
its first member, shuffled over the file (500 x 100: the 50 000-protein file of profiles/cluster/).  Timed in one process after a
warm-up on a small file, alternating, `--repeats` times:
  cluster   dct_sim.Clusters(min_domain=0.5).labels() and the text to /dev/null;
  density   dct_sim.DensityClusters(min_domain=0.5, min_neighbors=N).labels() and the same text.
`--package DIR` takes `dctdomain_amd` from DIR instead of this tree -- another commit's build, for `cluster` only: run the two
alternately, one process each.  Times are host clocks around work that ends in a device synchronise; the split comes from device
events around the calls that fill a tile (protein_min), link it (tri_link / tri_link_core) and count it (tri_degree), summed per
run.  Before a time is reported the labels are checked: every member of a planted family has size - 1 neighbours, so with
N <= size - 1 every protein is a core and the clusters are the families.

`scan` times tri_degree and tri_link_core alone on one int32 tile right of the diagonal, beside label_sums and tri_link on the same
tile: `sparse` -- two entries in a thousand within the bound, about what a file of families gives -- and, for tri_degree,
`every_entry` (a bound of 17000: every entry is counted), against the bytes of the tile."""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = {'protein_min': 'tile', 'l1_matrix': 'tile', 'tri_link': 'link', 'tri_degree': 'degree', 'tri_link_core': 'link_core',
         'cluster_labels': 'labels'}


def run(dct_sim, split_cls, what: str, neighbors: int, sid, idx, dct):
    import torch
    torch.cuda.synchronize()
    names = {k: v for k, v in STEPS.items() if hasattr(dct_sim, k)}
    with split_cls(dct_sim, names) as split, open(os.devnull, 'wb') as null:
        t0 = time.perf_counter()
        if what == 'density':
            job = dct_sim.DensityClusters(sid, idx, dct, min_domain=0.5, min_neighbors=neighbors)
        else:
            job = dct_sim.Clusters(sid, idx, dct, min_domain=0.5)
        labels = job.labels()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        job.write(null.write, labels)
        seconds = time.perf_counter() - t0
        parts = split.totals()
    row = {'what': what, 'seconds': round(seconds, 4), 'before_text': round(t1 - t0, 4), 'stripes': len(list(job.stripes())),
           'device_seconds': parts}
    if what == 'density':
        kinds = job.kinds()
        row.update(min_neighbors=neighbors, cores=int((kinds == 2).sum()), borders=int((kinds == 1).sum()), noise=int((kinds == 0).sum()))
    return row, labels


def part_run(args):
    if args.package:
        sys.path.insert(0, os.path.abspath(args.package))
    import torch
    from dctdomain_amd import dct_sim
    from tools.tree_bench import Split, planted
    if not torch.cuda.is_available():
        raise SystemExit('density_bench measures on a GPU: none found')
    whats = args.what.split(',')
    if args.neighbors > args.size - 1:
        raise SystemExit('with more neighbours asked than a family has members the clusters are not the families: nothing to check against')
    sid, idx, dct, fam = planted(args.families, args.size)
    n = len(sid)
    small = planted(20, 10)
    for what in whats:                                           # warm-up: code objects loaded, the allocator primed
        run(dct_sim, Split, what, min(args.neighbors, 9), *small[:3])
    first = np.full(args.families, n)
    np.minimum.at(first, fam, np.arange(n))
    rows = []
    for _ in range(args.repeats):
        for what in whats:
            row, labels = run(dct_sim, Split, what, args.neighbors, sid, idx, dct)
            assert np.array_equal(labels, first[fam]), f'{what}: not the planted families'
            if what == 'density':
                assert row['cores'] == n, 'a member of a planted family is not a core'
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
    from dctdomain_amd.similarity import NEAREST_NONE, cluster_labels, label_sums, tri_degree, tri_filter_count, tri_link, tri_link_core
    if not torch.cuda.is_available():
        raise SystemExit('density_bench measures on a GPU: none found')
    n_rows, n_cols, bound = args.rows, args.cols, 8500
    n = n_rows + n_cols
    gen = torch.Generator(device='cuda').manual_seed(5)
    tile = torch.randint(bound + 1, 17001, (n_rows, n_cols), dtype=torch.int32, device='cuda', generator=gen)
    near = torch.rand((n_rows, n_cols), device='cuda', generator=gen) < 0.002
    tile[near] = torch.randint(0, bound + 1, (int(near.sum().item()),), dtype=torch.int32, device='cuda', generator=gen)
    del near
    place = (tile, 0, n_rows)                                    # (the whole tile is right of the diagonal)
    deg = torch.zeros(n, dtype=torch.int32, device='cuda')
    parent = torch.arange(n, dtype=torch.int32, device='cuda')
    nearest = torch.full((n,), NEAREST_NONE, dtype=torch.int32, device='cuda')
    sums = torch.zeros(n, dtype=torch.int64, device='cuda')
    labels = (torch.randperm(n, device='cuda', generator=gen) // 100).to(torch.int32)
    # checked before anything is timed: the degrees against tri_filter_count, the forest of all cores against tri_link's
    tri_degree(*place, bound, deg)
    count = tri_filter_count(*place, bound)
    assert torch.equal(deg[:n_rows], count) and int(deg[n_rows:].sum().item()) == int(count.sum().item())
    edges = int(count.sum().item())
    core = (deg >= args.neighbors).to(torch.uint8)
    tri_link_core(*place, bound, torch.ones_like(core), parent, nearest)
    linked = cluster_labels(parent)
    parent.copy_(torch.arange(n, dtype=torch.int32, device='cuda'))
    tri_link(*place, bound, parent)
    assert torch.equal(cluster_labels(parent), linked) and bool((nearest == NEAREST_NONE).all().item())

    def fresh_forest():
        parent.copy_(torch.arange(n, dtype=torch.int32, device='cuda'))
        nearest.fill_(NEAREST_NONE)

    scans = [('tri_degree', 'sparse', lambda: tri_degree(*place, bound, deg), deg.zero_),
             ('tri_degree', 'every_entry', lambda: tri_degree(*place, 17000, deg), deg.zero_),
             ('tri_link_core', 'sparse', lambda: tri_link_core(*place, bound, core, parent, nearest), fresh_forest),
             ('tri_link', 'sparse', lambda: tri_link(*place, bound, parent), fresh_forest),
             ('label_sums', 'labels_of_100', lambda: label_sums(*place, labels, sums), sums.zero_)]
    rows = []
    for name, case, call, reset in scans:
        ms, every = _median_ms(call, reset, args.repeats)
        row = {'what': 'scan', 'kernel': name, 'case': case, 'rows': n_rows, 'cols': n_cols, 'tile_bytes': 4 * n_rows * n_cols,
               'entries_within_bound': edges, 'cores': int(core.sum().item()), 'ms_all': every, 'ms_median': round(ms, 4),
               'tile_GB_per_s': round(4 * n_rows * n_cols / ms / 1e6, 1), 'device': torch.cuda.get_device_name(0)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--part', choices=('run', 'scan'), default='run')
    ap.add_argument('--families', type=int, default=500)
    ap.add_argument('--size', type=int, default=100)
    ap.add_argument('--what', default='cluster,density')
    ap.add_argument('--neighbors', type=int, default=5)
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
