"""dct-sim --cluster --rep medoid on one GPU: the medoid run beside the plain cluster run, its device steps, and the scan alone.

    python tools/medoid_bench.py --part run [--families 500] [--size 100] [--what cluster,medoid] [--package DIR] [--out F.jsonl]
    python tools/medoid_bench.py --part scan [--rows 8192] [--cols 50000] [--out F.jsonl]

Input of `run`: tools/tree_bench.planted -- families x size proteins of 1-8 fingerprints, the members of a family near copies of
its first member, shuffled over the file (500 x 100: the 50 000-protein file of profiles/cluster/).  Timed in one process after a
warm-up on a small file, alternating, `--repeats` times:
  cluster   dct_sim.Clusters(min_domain=0.5).labels() and the text to /dev/null;
  medoid    .medoids() and the text with the medoids in the first field.
`--package DIR` takes `dctdomain_amd` from DIR instead of this tree -- another commit's build, for `cluster` only: run the two
alternately, one process each.  Times are host clocks around work that ends in a device synchronise; the split comes from device
events around the calls that fill a tile (protein_min), link it (tri_link) and sum it (label_sums), summed per run.  Before a time
is reported the medoids are checked: one per family, inside it, and equal to numpy's on three whole families.

`scan` times label_sums alone on one random int32 tile right of the diagonal, with every protein under one label (every entry is
loaded and added: the tile read) and with labels of 100 members each (most entries are skipped before the load), against the
bytes of the tile."""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = {'protein_min': 'tile', 'l1_matrix': 'tile', 'tri_link': 'link', 'label_sums': 'sums', 'cluster_labels': 'labels'}


def family_medoid(idx, dct, members):
    """The medoid of one family by numpy: min(L1, 17000) of the protein minimum, summed over the other members."""
    rows = [dct[idx[p]:idx[p + 1]].astype(np.int64) for p in members]
    key = np.zeros((len(members), len(members)), dtype=np.int64)
    for a in range(len(members)):
        for b in range(a + 1, len(members)):
            key[a, b] = key[b, a] = min(int(np.abs(rows[a][:, None, :] - rows[b][None, :, :]).sum(axis=2).min()), 17000)
    return int(members[np.argmin(key.sum(axis=1))])


def run(dct_sim, split_cls, what: str, sid, idx, dct):
    import torch
    torch.cuda.synchronize()
    names = {k: v for k, v in STEPS.items() if hasattr(dct_sim, k)}
    with split_cls(dct_sim, names) as split, open(os.devnull, 'wb') as null:
        t0 = time.perf_counter()
        job = dct_sim.Clusters(sid, idx, dct, min_domain=0.5)
        if what == 'medoid':
            rep = job.medoids()
            labels = job.last_labels
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            job.write(null.write, labels, rep=rep)
        else:
            rep, labels = None, job.labels()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            job.write(null.write, labels)
        seconds = time.perf_counter() - t0
        parts = split.totals()
    row = {'what': what, 'seconds': round(seconds, 4), 'before_text': round(t1 - t0, 4), 'stripes': len(list(job.stripes())),
           'device_seconds': parts}
    return row, labels, rep


def part_run(args):
    if args.package:
        sys.path.insert(0, os.path.abspath(args.package))
    import torch
    from dctdomain_amd import dct_sim
    from tools.tree_bench import Split, planted
    if not torch.cuda.is_available():
        raise SystemExit('medoid_bench measures on a GPU: none found')
    whats = args.what.split(',')
    sid, idx, dct, fam = planted(args.families, args.size)
    n = len(sid)
    small = planted(20, 10)
    for what in whats:                                           # warm-up: code objects loaded, the allocator primed
        run(dct_sim, Split, what, *small[:3])
    first = np.full(args.families, n)
    np.minimum.at(first, fam, np.arange(n))
    rows = []
    for _ in range(args.repeats):
        for what in whats:
            row, labels, rep = run(dct_sim, Split, what, sid, idx, dct)
            assert np.array_equal(labels, first[fam]), 'the cluster pass does not return the planted families'
            if rep is not None:
                assert np.array_equal(fam[rep], fam) and np.array_equal(rep, rep[first[fam]]), 'a medoid outside its family, or two in one'
                for f in (0, args.families // 2, args.families - 1):
                    members = np.flatnonzero(fam == f)
                    assert int(rep[members[0]]) == family_medoid(idx, dct, members), f'family {f}: not numpy\'s medoid'
                row['medoids_other_than_first'] = int((rep[first] != first).sum())
            row.update(package=os.path.dirname(os.path.dirname(os.path.abspath(dct_sim.__file__))), proteins=n, fingerprints=int(idx[-1]),
                       device=torch.cuda.get_device_name(0))
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def part_scan(args):
    import torch
    from dctdomain_amd.similarity import label_sums
    if not torch.cuda.is_available():
        raise SystemExit('medoid_bench measures on a GPU: none found')
    n_rows, n_cols = args.rows, args.cols
    n = n_rows + n_cols
    gen = torch.Generator(device='cuda').manual_seed(5)
    tile = torch.randint(0, 17001, (n_rows, n_cols), dtype=torch.int32, device='cuda', generator=gen)
    rows = []
    for name, labels in (('one_label', torch.zeros(n, dtype=torch.int32, device='cuda')),
                         ('labels_of_100', (torch.randperm(n, device='cuda', generator=gen) // 100).to(torch.int32))):
        sums = torch.zeros(n, dtype=torch.int64, device='cuda')
        label_sums(tile, 0, n_rows, labels, sums)                # (the whole tile is right of the diagonal)
        torch.cuda.synchronize()
        same = labels[:n_rows, None] == labels[None, n_rows:]
        want_total = 2 * int((tile.to(torch.int64) * same).sum().item())
        assert int(sums.sum().item()) == want_total, name
        counted = int(same.sum().item())
        del same
        times = []
        for _ in range(args.repeats + 1):
            sums.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            label_sums(tile, 0, n_rows, labels, sums)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        ms = sorted(times[1:])[len(times[1:]) // 2]
        row = {'what': 'scan', 'labels': name, 'rows': n_rows, 'cols': n_cols, 'tile_bytes': 4 * n_rows * n_cols, 'entries_counted': counted,
               'ms_all': [round(t, 4) for t in times[1:]], 'ms_median': round(ms, 4), 'tile_GB_per_s': round(4 * n_rows * n_cols / ms / 1e6, 1),
               'device': torch.cuda.get_device_name(0)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--part', choices=('run', 'scan'), default='run')
    ap.add_argument('--families', type=int, default=500)
    ap.add_argument('--size', type=int, default=100)
    ap.add_argument('--what', default='cluster,medoid')
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
