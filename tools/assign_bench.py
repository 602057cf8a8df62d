"""dct-sim --assign beside the routes it replaces (profiles/assign/README.md has the commands and what they print).

    python tools/assign_bench.py --part cover --reps 200000 --new 20000 --min-domain 0.5 [--repeat 3] [--out FILE.jsonl]
    python tools/assign_bench.py --part run   --reps 200000 --new 20000 --min-domain 0.5 [--repeat 3] [--out FILE.jsonl]

Both load two synthetic files of the database-build mix (tools/all_sim_bench.synth: 1-8 uniform int8 fingerprints in [-48, 48]
per protein, 4.5 on average, d = 480) and warm every route up on small files first.
`cover`: the cover pass alone, --repeat times each in one process, device time by events with a synchronize around each run:
the fused route (dctfp_rows_assign over all rows, as Assignment._cover_rows) and the tile route made of calls that were there
before it -- dctfp_protein_min into a rectangular int32 tile per stripe of representatives, then dctfp_greedy_tri_mark with the
representatives' state preset to "new representative".  The tile route is the yardstick.  The two assign arrays must be equal.
`run`: Assignment.labels() + text to /dev/null beside Representatives.labels() + text on the concatenated file, wall time."""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.all_sim_bench import synth                         # noqa: E402

SAD_PEAK = 157e12                                             # byte differences per second (256 CUs x 64 lanes x 4 per clock)


def _load(path):
    with np.load(path) as data:
        return data['sid'], np.asarray(data['idx'], dtype=np.int64), data['dct']


def _files(tmp, m, n):
    rep, new = os.path.join(tmp, f'r{m}-dct.npz'), os.path.join(tmp, f'n{n}-dct.npz')
    synth(rep, m, 11)
    synth(new, n, 12)
    return _load(rep), _load(new)


def _spread(v):
    return {'runs': [round(x, 4) for x in v], 'median': round(statistics.median(v), 4), 'min': round(min(v), 4), 'max': round(max(v), 4)}


def _cover_fused(job, torch):
    assign = torch.full((job.m + job.n,), 0x7fffffff, dtype=torch.int32, device='cuda')
    job._cover_rows(assign)
    return assign


def _cover_tile(job, torch, rep_dev, new_dev):
    """protein_min into a rectangular tile per stripe of representatives + greedy_tri_mark, the representatives preset."""
    from dctdomain_amd import dct_sim
    from dctdomain_amd.similarity import GreedyState, greedy_tri_mark, protein_min
    m, n = job.m, job.n
    gs = GreedyState(m + n)
    gs.state[:m] = 2                                          # new representative: marks all its columns
    gs.state[m:] = 1                                          # (any state that neither marks nor stamps)
    per = max(1, dct_sim.FilteredPairs.TILE_INTS // n)
    ib = job.idx
    for p0 in range(0, m, per):
        p1 = min(m, p0 + per)
        ia = job.rep_idx[p0:p1 + 1] - job.rep_idx[p0]
        tile = protein_min(rep_dev[job.rep_idx[p0]:job.rep_idx[p1]], ia, new_dev, ib)
        greedy_tri_mark(tile, p0, m, job.bound_domain, gs, m + n, 1)
        del tile
    return gs.assign


def part_cover(args):
    import torch
    from dctdomain_amd import dct_sim
    from dctdomain_amd.similarity import to_device_int8
    with tempfile.TemporaryDirectory() as tmp:
        (wr, wn) = _files(tmp, 2000, 500)
        (rep, new) = _files(tmp, args.reps, args.new)

    def both(rep, new, repeat):
        job = dct_sim.Assignment(*rep, *new, min_domain=args.min_domain)
        rep_dev, new_dev = to_device_int8(rep[2]), to_device_int8(new[2])
        ms = {'fused': [], 'tile': []}
        out = {}
        for _ in range(repeat):
            for name, fn in (('fused', lambda: _cover_fused(job, torch)), ('tile', lambda: _cover_tile(job, torch, rep_dev, new_dev))):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                out[name] = fn()
                e1.record()
                torch.cuda.synchronize()
                ms[name].append(e0.elapsed_time(e1))
        return ms, bool(torch.equal(out['fused'], out['tile'])), int((out['fused'][job.m:] != 0x7fffffff).sum())

    both(wr, wn, 2)                                           # warm-up: both routes on small files
    ms, same, covered = both(rep, new, args.repeat)
    row_pairs = int(rep[1][-1]) * int(new[1][-1])
    fused, tile = statistics.median(ms['fused']), statistics.median(ms['tile'])
    spread = max(max(v) - min(v) for v in ms.values())
    return {'part': 'cover', 'reps': args.reps, 'new': args.new, 'rep_rows': int(rep[1][-1]), 'new_rows': int(new[1][-1]), 'min_domain': args.min_domain,
            'fused_ms': _spread(ms['fused']), 'tile_ms': _spread(ms['tile']), 'assign_equal': same, 'covered': covered,
            'fused_over_tile': round(fused / tile, 4), 'fused_not_slower_beyond_spread': bool(fused <= tile + spread),
            'fused_share_of_sad_peak': round(row_pairs * 480 / (fused * 1e-3) / SAD_PEAK, 4),
            'tile_share_of_sad_peak': round(row_pairs * 480 / (tile * 1e-3) / SAD_PEAK, 4)}


def part_run(args):
    import torch
    from dctdomain_amd import dct_sim
    with tempfile.TemporaryDirectory() as tmp:
        (wr, wn) = _files(tmp, 2000, 500)
        (rep, new) = _files(tmp, args.reps, args.new)

    def both(rep, new, repeat):
        whole = (np.concatenate([rep[0], np.char.add('n', new[0])]), np.concatenate([rep[1], rep[1][-1] + new[1][1:]]), np.concatenate([rep[2], new[2]]))
        s = {'assign': [], 'greedy_whole': []}
        with open(os.devnull, 'wb', buffering=0) as fh:
            for _ in range(repeat):
                for name, make in (('assign', lambda: dct_sim.Assignment(*rep, *new, min_domain=args.min_domain)),
                                   ('greedy_whole', lambda: dct_sim.Representatives(*whole, min_domain=args.min_domain))):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    make().write(lambda mv: fh.write(mv))
                    torch.cuda.synchronize()
                    s[name].append(time.perf_counter() - t0)
        return s

    both(wr, wn, 1)
    s = both(rep, new, args.repeat)
    return {'part': 'run', 'reps': args.reps, 'new': args.new, 'min_domain': args.min_domain, 'assign_s': _spread(s['assign']),
            'greedy_whole_s': _spread(s['greedy_whole'])}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--part', required=True, choices=['cover', 'run'])
    ap.add_argument('--reps', type=int, default=200000)
    ap.add_argument('--new', type=int, default=20000)
    ap.add_argument('--min-domain', type=float, default=0.5)
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--out')
    args = ap.parse_args(argv)
    res = {'cover': part_cover, 'run': part_run}[args.part](args)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'a') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
