"""dct-sim all-against-all (all_sim) streamed from the device: identity with the block-matrix path, and rates at scale.

    python tools/all_sim_bench.py --part compare [--n 2000]            # old (Blocks) and new path: sha256 of the text, times
    python tools/all_sim_bench.py --part scale --n 20000 [--dir D]     # new path to /dev/null and to a file under D
    python tools/all_sim_bench.py --part scale --n 1000000 --min-global 0.5   # the same with cut-offs (dct_sim.FilteredPairs)
    python tools/all_sim_bench.py --part filter --n 50000 [--min-domain 0.5]  # cut-offs beside the unfiltered run, one process
    python tools/all_sim_bench.py --part cluster --n 50000 --families 500 --family-size 100 --min-domain 0.5   # --cluster beside the cut-offs
    python tools/all_sim_bench.py --part domains --n 50000 --families 500 --family-size 100 --min-domain 0.5   # --domains beside the same cut-offs
    python tools/all_sim_bench.py --part map --n 50000 --families 500 --family-size 100 --min-domain 0.5       # --domain-map beside --domains
    python tools/all_sim_bench.py --part rows_link --n 50000 --families 500 --family-size 100 --min-domain 0.5 # --cluster --level domain

`rows_link` loads one synthetic file with planted families and runs, after a warm-up of both on a small file, --repeat times each:
the domain families (DomainClusters.labels: dctfp_rows_link, no distance stored) and the materialising route over the same row
pairs in the same process -- stripes of rows against the rows from the stripe's start onward, l1_matrix into int32 tiles of at
most 1 GiB and tri_link over them (no owner exclusion there: the same contraction, other edges).  Events around rows_link and around
l1_matrix give both kernels' rates in row pairs per second and the share of the one in the other.
`filter` loads one synthetic file and runs, after the load and a warm-up on a small file, the unfiltered path (AllPairs, to
/dev/null as `scale` does) and the path with cut-offs; events around the device steps of the second (the tile: protein_min or
l1_matrix; the filter; pair_min; the lines) say where its device time goes.  --planted fingerprints are overwritten with near
copies of others first: random proteins alone leave nothing above a cut-off.
`cluster` loads one synthetic file (--families x --family-size proteins overwritten with near copies of a family's first member)
and runs, after a warm-up of both on a small file, --repeat times each: the path with cut-offs (FilteredPairs, to /dev/null) and
the clustering at the same cut-offs (Clusters); events around the device steps of the latter (tile / link / labels), the host
text timed apart.  Then the greedy linkage (Representatives) on the same file in the same way: its device steps (tile / decide /
mark), its rounds, and how many proteins its labels move away from single linkage's.
`domains` is `cluster`'s procedure for --domains: the path with cut-offs without the flag, then with it (labels = the 1-based index
of a fingerprint within its protein), --repeat times each in that order, events around the device steps of the second.
`scale` writes a synthetic -dct.npz (about 4.5 fingerprints per protein, 17-character ids) and runs the new path in a child
process per sink (and one that only initialises the GPU: the RSS floor), so that the child's peak RSS (ru_maxrss of RUSAGE_CHILDREN, as tools/run_with_rss.py) is that of the run
alone.  The child also measures the pinned device-to-host copy rate of one TEXT_BYTES buffer.  The file run is skipped when
the disk under D has less room than the text.  Prints one JSON line per part; --out appends it to a file."""

from __future__ import annotations

import argparse
import hashlib
import json
import os
import resource
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synth(path: str, n: int, seed: int):
    rng = np.random.default_rng(seed)
    counts = rng.integers(1, 9, size=n)                       # 1 .. 8 fingerprints, 4.5 on average
    idx = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts, out=idx[1:])
    dct = rng.integers(-48, 49, size=(int(idx[-1]), 480), dtype=np.int8)
    sid = np.array([f'UniRef50_{k:08d}' for k in range(n)])
    np.savez(path, sid=sid, idx=idx, dom=np.array(['1-9'] * len(dct)), dct=dct)
    return int(idx[-1])


def _old_text(path: str) -> bytes:
    """all_sim as it printed through dct_sim.Blocks (header and result lines)."""
    from dctdomain_amd import dct_sim
    blk = dct_sim.Blocks(path)
    lines = [dct_sim.HEADER]
    for i, j in zip(*np.triu_indices(len(blk.rows), k=1)):
        maxs, s = blk.scores(i, j)
        lines.append(f'{blk.rows[i]} {blk.rows[j]} {maxs:.3f} {s:.3f}')
    return ('\n'.join(lines) + '\n').encode('utf8')


def part_compare(args):
    import torch
    from dctdomain_amd import dct_sim
    with tempfile.TemporaryDirectory(dir=args.dir) as tmp:
        path = os.path.join(tmp, 'c-dct.npz')
        synth(path, args.n, 5)
        dct_sim.main(['--dct', path, '--output', os.path.join(tmp, 'warm.txt')])     # (context, kernels loaded)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        old = _old_text(path)
        t_old = time.perf_counter() - t0
        out = os.path.join(tmp, 'new.txt')
        t0 = time.perf_counter()
        dct_sim.main(['--dct', path, '--output', out])
        t_new = time.perf_counter() - t0
        new = open(out, 'rb').read()
    return {'part': 'compare', 'n': args.n, 'lines': new.count(b'\n') - 1, 'sha256_old': hashlib.sha256(old).hexdigest(),
            'sha256_new': hashlib.sha256(new).hexdigest(), 'identical': old == new, 'old_s': round(t_old, 3), 'new_s': round(t_new, 3)}


def part_run(args):
    """(child) one streamed run of the new path from --npz to --sink, after the load."""
    import torch
    from dctdomain_amd import dct_sim
    sid, idx, fps = dct_sim._load_npz(args.npz)
    n = len(sid)
    cut = args.min_domain is not None or args.min_global is not None
    ap = dct_sim.FilteredPairs(sid, idx, fps, args.min_domain, args.min_global) if cut else dct_sim.AllPairs(sid, idx, fps)
    written, kept = [0], [0]
    with open(args.sink, 'wb', buffering=0) as fh:
        def sink(mv):
            fh.write(mv)
            written[0] += len(mv)
            if cut:
                kept[0] += bytes(mv).count(b'\n')
        t0 = time.perf_counter()
        ap.write(sink)
        torch.cuda.synchronize()
        os.fsync(fh.fileno()) if args.sink != os.devnull else None
        dt = time.perf_counter() - t0
    dev = torch.device('cuda', 0)
    # pinned device-to-host rate of one text buffer, in this process (after the run: its buffers come from the same cache)
    size = int(min(ap.TEXT_BYTES, 1 << 28))
    src = torch.empty(size, dtype=torch.uint8, device=dev)
    pin = torch.empty(size, dtype=torch.uint8, pin_memory=True)
    pin.copy_(src, non_blocking=True)
    torch.cuda.synchronize()
    reps = 10
    t0 = time.perf_counter()
    for _ in range(reps):
        pin.copy_(src, non_blocking=True)
    torch.cuda.synchronize()
    d2h = reps * size / (time.perf_counter() - t0)
    del src, pin
    lines = n * (n - 1) // 2
    if cut:
        return {'n': n, 'fingerprints': int(idx[-1]), 'pairs': lines, 'min_domain': args.min_domain, 'min_global': args.min_global,
                'route': ap.route, 'lines': kept[0], 'text_bytes': written[0], 'seconds': round(dt, 3), 'pairs_per_s': round(lines / dt)}
    return {'n': n, 'fingerprints': int(idx[-1]), 'lines': lines, 'text_bytes': written[0], 'seconds': round(dt, 3),
            'lines_per_s': round(lines / dt), 'text_GBps': round(written[0] / dt / 1e9, 2), 'd2h_pinned_GBps': round(d2h / 1e9, 2),
            'text_over_d2h': round(written[0] / dt / d2h, 3)}


def part_filter(args):
    """One process: the unfiltered run (AllPairs, /dev/null) and the run with cut-offs on the same loaded file, after a warm-up
    of both on a small one; device time of the second by step."""
    import torch
    from dctdomain_amd import dct_sim
    min_domain = args.min_domain if args.min_domain is not None or args.min_global is not None else 0.5
    with tempfile.TemporaryDirectory(dir=args.dir) as tmp:
        small, path = os.path.join(tmp, 'w-dct.npz'), os.path.join(tmp, 'f-dct.npz')
        synth(small, 2000, 5)
        synth(path, args.n, 7)
        warm = dct_sim._load_npz(small)
        sid, idx, fps = dct_sim._load_npz(path)
    # (random proteins lie far above any cut-off: some near copies of single fingerprints, so that pair_min and the lines run)
    rng = np.random.default_rng(11)
    for rows_of, k in ((warm[2], min(args.planted, 100)), (fps, args.planted)):     # (the warm-up takes every step too)
        rows = rng.choice(len(rows_of), size=2 * k, replace=False)
        rows_of[rows[:k]] = np.clip(rows_of[rows[k:]].astype(np.int64) + rng.integers(-2, 3, size=(k, rows_of.shape[1])), -127, 127)
    spans = {}

    def timed(name, label):
        fn = getattr(dct_sim, name)

        def run(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **k)
            e1.record()
            spans.setdefault(label, []).append((e0, e1))
            return out
        setattr(dct_sim, name, run)
        return fn
    written, kept = [0], [0]
    with open(os.devnull, 'wb', buffering=0) as fh:
        def sink(mv):
            fh.write(mv)
            written[0] += len(mv)

        def sink_counting(mv):
            sink(mv)
            kept[0] += bytes(mv).count(b'\n')
        dct_sim.AllPairs(*warm).write(sink)
        dct_sim.FilteredPairs(*warm, min_domain, args.min_global).write(sink)
        torch.cuda.synchronize()
        written[0] = 0
        t0 = time.perf_counter()
        dct_sim.AllPairs(sid, idx, fps).write(sink)
        torch.cuda.synchronize()
        t_all, text_all = time.perf_counter() - t0, written[0]
        steps = (('protein_min', 'tile'), ('l1_matrix', 'tile'), ('tri_filter_count', 'filter'), ('tri_filter_fill', 'filter'),
                 ('pair_min_device', 'pair_min'), ('pair_line_offsets', 'lines'), ('pair_lines', 'lines'))
        real = [(name, timed(name, label)) for name, label in steps]
        written[0] = 0
        fp = dct_sim.FilteredPairs(sid, idx, fps, min_domain, args.min_global)
        t0 = time.perf_counter()
        fp.write(sink_counting)
        torch.cuda.synchronize()
        t_cut = time.perf_counter() - t0
        for name, fn in real:
            setattr(dct_sim, name, fn)
    ms = {label: round(sum(a.elapsed_time(b) for a, b in ev), 3) for label, ev in spans.items()}
    device = sum(ms.values())
    n = len(sid)
    return {'part': 'filter', 'n': n, 'fingerprints': int(idx[-1]), 'pairs': n * (n - 1) // 2, 'planted_rows': args.planted, 'min_domain': min_domain,
            'min_global': args.min_global, 'route': fp.route, 'stripes': len(list(fp.stripes())),
            'unfiltered_s': round(t_all, 3), 'unfiltered_text_bytes': text_all, 'filtered_s': round(t_cut, 3), 'filtered_lines': kept[0],
            'filtered_text_bytes': written[0], 'speedup': round(t_all / t_cut, 2), 'filtered_faster': t_cut < t_all, 'device_ms': ms,
            'share_outside_tile_of_run': round(1 - ms.get('tile', 0.0) / (1e3 * t_cut), 4),
            'share_outside_tile_of_device_steps': round(1 - ms.get('tile', 0.0) / device, 4) if device else None}


def plant_families(idx, fps, families: int, size: int, seed: int = 13):
    """Overwrites `families` x `size` proteins with near copies (+-2) of the first member of their family.  Returns (idx, fps)."""
    n = len(idx) - 1
    rng = np.random.default_rng(seed)
    chosen = rng.choice(n, size=families * size, replace=False).reshape(families, size)
    counts = np.diff(idx)
    new_counts = counts.copy()
    new_counts[chosen[:, 1:]] = counts[chosen[:, :1]]
    new_idx = np.concatenate([[0], np.cumsum(new_counts)]).astype(np.int64)
    out = np.empty((int(new_idx[-1]), fps.shape[1]), dtype=np.int8)
    same = np.ones(n, dtype=bool)
    same[chosen[:, 1:].ravel()] = False
    out[np.repeat(same, new_counts)] = fps[np.repeat(same, counts)]
    for fam in chosen:
        src = fps[idx[fam[0]]:idx[fam[0] + 1]].astype(np.int64)
        for p in fam[1:]:
            out[new_idx[p]:new_idx[p + 1]] = np.clip(src + rng.integers(-2, 3, size=src.shape), -127, 127)
    return new_idx, out


def part_cluster(args):
    """One process: FilteredPairs to /dev/null, Clusters and Representatives at the same cut-offs on the same loaded file, --repeat
    times each after a warm-up of all three on a small one; device time of the two clusterings by step."""
    import torch
    from dctdomain_amd import dct_sim
    min_domain = args.min_domain if args.min_domain is not None or args.min_global is not None else 0.5
    with tempfile.TemporaryDirectory(dir=args.dir) as tmp:
        small, path = os.path.join(tmp, 'w-dct.npz'), os.path.join(tmp, 'f-dct.npz')
        synth(small, 2000, 5)
        synth(path, args.n, 7)
        wsid, widx, wfps = dct_sim._load_npz(small)
        sid, idx, fps = dct_sim._load_npz(path)
    widx, wfps = plant_families(widx, wfps, 10, 10)
    if args.families:
        idx, fps = plant_families(idx, fps, args.families, args.family_size)
    spans = {}

    def timed(name, label):
        fn = getattr(dct_sim, name)

        def run(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **k)
            e1.record()
            spans.setdefault(label, []).append((e0, e1))
            return out
        setattr(dct_sim, name, run)
        return fn
    written, kept = [0], [0]
    with open(os.devnull, 'wb', buffering=0) as fh:
        def sink(mv):
            fh.write(mv)
            written[0] += len(mv)
            kept[0] += bytes(mv).count(b'\n')
        dct_sim.FilteredPairs(wsid, widx, wfps, min_domain, args.min_global).write(sink)
        dct_sim.Clusters(wsid, widx, wfps, min_domain, args.min_global).write(sink)
        dct_sim.Representatives(wsid, widx, wfps, min_domain, args.min_global).write(sink)
        torch.cuda.synchronize()
        t_filter, t_cluster, t_text, device_ms = [], [], [], []
        t_greedy, greedy_ms, rounds = [], [], []
        for _ in range(args.repeat):
            written[0] = kept[0] = 0
            fp = dct_sim.FilteredPairs(sid, idx, fps, min_domain, args.min_global)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fp.write(sink)
            torch.cuda.synchronize()
            t_filter.append(time.perf_counter() - t0)
            edges, edge_bytes = kept[0], written[0]
        steps = (('protein_min', 'tile'), ('l1_matrix', 'tile'), ('tri_link', 'link'), ('link_pairs', 'link'), ('cluster_labels', 'labels'),
                 ('tri_filter_count', 'filter'), ('tri_filter_fill', 'filter'), ('pair_min_device', 'pair_min'))
        real = [(name, timed(name, label)) for name, label in steps]
        for _ in range(args.repeat):
            spans.clear()
            written[0] = kept[0] = 0
            cl = dct_sim.Clusters(sid, idx, fps, min_domain, args.min_global)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            labels = cl.labels()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for text in dct_sim.cluster_lines(sid, labels):
                sink(memoryview(text))
            t2 = time.perf_counter()
            t_cluster.append(t2 - t0)
            t_text.append(t2 - t1)
            device_ms.append({label: round(sum(a.elapsed_time(b) for a, b in ev), 3) for label, ev in spans.items()})
        for name, fn in real:
            setattr(dct_sim, name, fn)
        cluster_bytes, cluster_lines = written[0], kept[0]
        steps = (('protein_min', 'tile'), ('l1_matrix', 'tile'), ('greedy_decide', 'decide'), ('greedy_tri_mark', 'mark'),
                 ('greedy_pairs_mark', 'mark'), ('tri_filter_count', 'filter'), ('tri_filter_fill', 'filter'), ('pair_min_device', 'pair_min'))
        real = [(name, timed(name, label)) for name, label in steps]
        for _ in range(args.repeat):
            spans.clear()
            rp = dct_sim.Representatives(sid, idx, fps, min_domain, args.min_global)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            greedy = rp.labels()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for text in dct_sim.cluster_lines(sid, greedy):
                sink(memoryview(text))
            t_greedy.append(time.perf_counter() - t0)
            rounds.append(rp.rounds)
            greedy_ms.append({label: round(sum(a.elapsed_time(b) for a, b in ev), 3) for label, ev in spans.items()})
        for name, fn in real:
            setattr(dct_sim, name, fn)
    n = len(sid)
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    ms = device_ms[t_cluster.index(med(t_cluster))]
    gms = greedy_ms[t_greedy.index(med(t_greedy))]
    is_rep = greedy == np.arange(n)
    res_greedy = {'greedy_s': [round(t, 3) for t in t_greedy], 'greedy_median_s': round(med(t_greedy), 3), 'greedy_rounds': rounds,
                  'greedy_over_cluster': round(med(t_greedy) / med(t_cluster), 4), 'greedy_within_10_percent': med(t_greedy) <= 1.1 * med(t_cluster),
                  'greedy_clusters': int(is_rep.sum()), 'greedy_largest': int(np.bincount(greedy).max()),
                  'greedy_labels_other_than_single': int((greedy != labels).sum()),
                  'greedy_device_ms_of_median_run': gms, 'greedy_device_ms_all': greedy_ms}
    return {'part': 'cluster', 'n': n, 'fingerprints': int(idx[-1]), 'pairs': n * (n - 1) // 2, 'families': args.families,
            'family_size': args.family_size, 'min_domain': min_domain, 'min_global': args.min_global, 'route': cl.route,
            'stripes': len(list(cl.stripes())), 'edges': edges, 'edge_text_bytes': edge_bytes, 'clusters': int(len(np.unique(labels))),
            'largest': int(np.bincount(labels).max()), 'cluster_text_bytes': cluster_bytes, 'cluster_lines': cluster_lines,
            'filtered_s': [round(t, 3) for t in t_filter], 'cluster_s': [round(t, 3) for t in t_cluster],
            'cluster_host_text_s': [round(t, 3) for t in t_text], 'filtered_median_s': round(med(t_filter), 3),
            'cluster_median_s': round(med(t_cluster), 3), 'filtered_spread_s': round(max(t_filter) - min(t_filter), 3),
            'cluster_faster': med(t_cluster) < med(t_filter),
            'cluster_within_filtered_spread': med(t_cluster) <= med(t_filter) + (max(t_filter) - min(t_filter)),
            'device_ms_of_median_run': ms, 'device_ms_all': device_ms,
            'link_over_tile': round(ms.get('link', 0.0) / ms['tile'], 4) if ms.get('tile') else None, **res_greedy}


def _live_pairs(a0: int, na: int, b0: int, nb: int) -> int:
    """Row pairs in the 128 x 128 blocks dctfp_rows_link contracts: those not wholly on or left of the diagonal."""
    r_first = a0 + 128 * np.arange((na + 127) // 128, dtype=np.int64)
    c_last = b0 + np.minimum(nb, 128 * (np.arange((nb + 127) // 128, dtype=np.int64) + 1)) - 1
    return int((c_last[None, :] > r_first[:, None]).sum()) * 128 * 128


def part_rows_link(args):
    """One process: DomainClusters.labels and the materialising route (l1_matrix into 1 GiB tiles + tri_link) on the same loaded
    file, --repeat times each after a warm-up of both on a small one; device time of rows_link and of l1_matrix by events."""
    import torch
    from dctdomain_amd import dct_sim, similarity
    min_domain = args.min_domain if args.min_domain is not None else 0.5
    with tempfile.TemporaryDirectory(dir=args.dir) as tmp:
        small, path = os.path.join(tmp, 'w-dct.npz'), os.path.join(tmp, 'f-dct.npz')
        synth(small, 2000, 5)
        synth(path, args.n, 7)
        wsid, widx, wfps = dct_sim._load_npz(small)
        sid, idx, fps = dct_sim._load_npz(path)
    widx, wfps = plant_families(widx, wfps, 10, 10)
    if args.families:
        idx, fps = plant_families(idx, fps, args.families, args.family_size)
    bound = dct_sim.sim_bound(min_domain)
    tile_ints = dct_sim.FilteredPairs.TILE_INTS
    spans, pairs = {}, {}

    def timed(module, name, count):
        fn = getattr(module, name)

        def run(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **k)
            e1.record()
            spans.setdefault(name, []).append((e0, e1))
            pairs[name] = pairs.get(name, 0) + count(*a)
            return out
        setattr(module, name, run)
        return fn

    def materialised(rows_dev):
        """Stripes x the rows from the stripe's start onward: l1_matrix into a tile, tri_link over it."""
        total = rows_dev.shape[0]
        parent = torch.arange(total, dtype=torch.int32, device=rows_dev.device)
        s0 = 0
        while s0 < total:
            s1 = min(total, s0 + max(1, tile_ints // (total - s0)))
            tile = similarity.l1_matrix(rows_dev[s0:s1], rows_dev[s0:])
            similarity.tri_link(tile, s0, s0, bound, parent)
            del tile
            s0 = s1
        return similarity.cluster_labels(parent).cpu().numpy()

    dct_sim.DomainClusters(wsid, widx, wfps, min_domain).labels()
    materialised(similarity.to_device_int8(wfps))
    torch.cuda.synchronize()
    real = [(dct_sim, 'rows_link', timed(dct_sim, 'rows_link', lambda a, a0, b, b0, *_: _live_pairs(a0, a.shape[0], b0, b.shape[0]))),
            (similarity, 'l1_matrix', timed(similarity, 'l1_matrix', lambda a, b, *_: a.shape[0] * b.shape[0]))]
    t_fused, t_mat, ms_fused, ms_l1 = [], [], [], []
    for _ in range(args.repeat):
        spans.clear()
        pairs.clear()
        dc = dct_sim.DomainClusters(sid, idx, fps, min_domain)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        labels = dc.labels()
        torch.cuda.synchronize()
        t_fused.append(time.perf_counter() - t0)
        ms_fused.append(sum(a.elapsed_time(b) for a, b in spans['rows_link']))
        fused_pairs = pairs['rows_link']
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows_dev = similarity.to_device_int8(fps[:int(idx[-1])])          # (the upload is inside both times)
        mat_labels = materialised(rows_dev)
        torch.cuda.synchronize()
        t_mat.append(time.perf_counter() - t0)
        ms_l1.append(sum(a.elapsed_time(b) for a, b in spans['l1_matrix']))
        l1_pairs = pairs['l1_matrix']
        del rows_dev
    for module, name, fn in real:
        setattr(module, name, fn)
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    rate_fused, rate_l1 = fused_pairs / (1e-3 * med(ms_fused)), l1_pairs / (1e-3 * med(ms_l1))
    nodes = labels >= 0
    return {'part': 'rows_link', 'n': len(sid), 'fingerprints': int(idx[-1]), 'families': args.families, 'family_size': args.family_size,
            'min_domain': min_domain, 'bound': bound, 'clusters': int(len(np.unique(labels[nodes]))), 'largest': int(np.bincount(labels[nodes]).max()),
            'clusters_without_owner_exclusion': int(len(np.unique(mat_labels))),
            'fused_s': [round(t, 3) for t in t_fused], 'materialised_s': [round(t, 3) for t in t_mat],
            'fused_median_s': round(med(t_fused), 3), 'materialised_median_s': round(med(t_mat), 3),
            'fused_spread_s': round(max(t_fused) - min(t_fused), 3), 'materialised_spread_s': round(max(t_mat) - min(t_mat), 3),
            'fused_not_slower_beyond_spread': med(t_fused) <= med(t_mat) + (max(t_fused) - min(t_fused)) + (max(t_mat) - min(t_mat)),
            'rows_link_ms': [round(v, 3) for v in ms_fused], 'l1_matrix_ms': [round(v, 3) for v in ms_l1],
            'rows_link_pairs': fused_pairs, 'l1_matrix_pairs': l1_pairs,
            'rows_link_pairs_per_s': round(rate_fused, 1), 'l1_matrix_pairs_per_s': round(rate_l1, 1),
            'rows_link_share_of_l1_matrix_rate': round(rate_fused / rate_l1, 4)}


def part_domains(args):
    """One process: FilteredPairs to /dev/null without and with the domain pair on the same loaded file, --repeat times each after
    a warm-up of both on a small one; device time of the second by step."""
    import torch
    from dctdomain_amd import dct_sim
    min_domain = args.min_domain if args.min_domain is not None or args.min_global is not None else 0.5
    with tempfile.TemporaryDirectory(dir=args.dir) as tmp:
        small, path = os.path.join(tmp, 'w-dct.npz'), os.path.join(tmp, 'f-dct.npz')
        synth(small, 2000, 5)
        synth(path, args.n, 7)
        wsid, widx, wfps = dct_sim._load_npz(small)
        sid, idx, fps = dct_sim._load_npz(path)
    widx, wfps = plant_families(widx, wfps, 10, 10)
    if args.families:
        idx, fps = plant_families(idx, fps, args.families, args.family_size)
    t0 = time.perf_counter()
    labels = dct_sim.fingerprint_labels(sid, idx)
    t_labels = time.perf_counter() - t0
    spans = {}

    def timed(name, label):
        fn = getattr(dct_sim, name)

        def run(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **k)
            e1.record()
            spans.setdefault(label, []).append((e0, e1))
            return out
        setattr(dct_sim, name, run)
        return fn
    written, kept = [0], [0]
    with open(os.devnull, 'wb', buffering=0) as fh:
        def sink(mv):
            fh.write(mv)
            written[0] += len(mv)
            kept[0] += bytes(mv).count(b'\n')
        dct_sim.FilteredPairs(wsid, widx, wfps, min_domain, args.min_global).write(sink)
        dct_sim.FilteredPairs(wsid, widx, wfps, min_domain, args.min_global, labels=dct_sim.fingerprint_labels(wsid, widx)).write(sink)
        torch.cuda.synchronize()
        t_plain, t_dom, device_ms, sizes = [], [], [], {}
        for flagged in (False, True):
            if flagged:
                steps = (('protein_min', 'tile'), ('l1_matrix', 'tile'), ('tri_filter_count', 'filter'), ('tri_filter_fill', 'filter'),
                         ('pair_argmin_device', 'pair_argmin'), ('pair_line_offsets', 'lines'), ('pair_lines', 'lines'))
                real = [(name, timed(name, label)) for name, label in steps]
            for _ in range(args.repeat):
                spans.clear()
                written[0] = kept[0] = 0
                fp = dct_sim.FilteredPairs(sid, idx, fps, min_domain, args.min_global, labels=labels if flagged else None)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fp.write(sink)
                torch.cuda.synchronize()
                (t_dom if flagged else t_plain).append(time.perf_counter() - t0)
                sizes[flagged] = (kept[0], written[0])
                if flagged:
                    device_ms.append({label: round(sum(a.elapsed_time(b) for a, b in ev), 3) for label, ev in spans.items()})
        for name, fn in real:
            setattr(dct_sim, name, fn)
    n = len(sid)
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    return {'part': 'domains', 'n': n, 'fingerprints': int(idx[-1]), 'pairs': n * (n - 1) // 2, 'families': args.families,
            'family_size': args.family_size, 'min_domain': min_domain, 'min_global': args.min_global, 'route': fp.route,
            'lines': sizes[False][0], 'text_bytes': sizes[False][1], 'domain_lines': sizes[True][0], 'domain_text_bytes': sizes[True][1],
            'labels_host_s': round(t_labels, 3), 'plain_s': [round(t, 3) for t in t_plain], 'domains_s': [round(t, 3) for t in t_dom],
            'plain_median_s': round(med(t_plain), 3), 'domains_median_s': round(med(t_dom), 3),
            'plain_spread_s': round(max(t_plain) - min(t_plain), 3), 'domains_over_plain': round(med(t_dom) / med(t_plain), 3),
            'device_ms_of_median_run': device_ms[t_dom.index(med(t_dom))], 'device_ms_all': device_ms}


def part_map(args):
    """One process: FilteredPairs to /dev/null with the domain pair (--domains) and with the domain map (--domain-map at the
    cut-off of --min-domain) on the same loaded file, --repeat times each after a warm-up of both on a small one; the bytes of
    text each wrote, and the device time of the map runs by step."""
    import torch
    from dctdomain_amd import dct_sim
    min_domain = args.min_domain if args.min_domain is not None else 0.5
    with tempfile.TemporaryDirectory(dir=args.dir) as tmp:
        small, path = os.path.join(tmp, 'w-dct.npz'), os.path.join(tmp, 'f-dct.npz')
        synth(small, 2000, 5)
        synth(path, args.n, 7)
        wsid, widx, wfps = dct_sim._load_npz(small)
        sid, idx, fps = dct_sim._load_npz(path)
    widx, wfps = plant_families(widx, wfps, 10, 10)
    if args.families:
        idx, fps = plant_families(idx, fps, args.families, args.family_size)
    labels = dct_sim.fingerprint_labels(sid, idx)
    bound = dct_sim.map_bound(None, min_domain)
    spans = {}

    def timed(name, label):
        fn = getattr(dct_sim, name)

        def run(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **k)
            e1.record()
            spans.setdefault(label, []).append((e0, e1))
            return out
        setattr(dct_sim, name, run)
        return fn

    def job(s, i, f, names, mapped):
        fp = dct_sim.FilteredPairs(s, i, f, min_domain, args.min_global, labels=names)
        return fp.with_map(bound) if mapped else fp
    written, kept = [0], [0]
    with open(os.devnull, 'wb', buffering=0) as fh:
        def sink(mv):
            fh.write(mv)
            written[0] += len(mv)
            kept[0] += bytes(mv).count(b'\n')
        for mapped in (False, True):
            job(wsid, widx, wfps, dct_sim.fingerprint_labels(wsid, widx), mapped).write(sink)
        torch.cuda.synchronize()
        times, device_ms, sizes = {False: [], True: []}, [], {}
        for mapped in (False, True):
            if mapped:
                steps = (('protein_min', 'tile'), ('l1_matrix', 'tile'), ('tri_filter_count', 'filter'), ('tri_filter_fill', 'filter'),
                         ('pair_argmin_device', 'pair_argmin'), ('pair_row_best_device', 'pair_row_best'),
                         ('pair_map_line_lengths', 'line lengths'), ('pair_map_lines', 'lines'))
                real = [(name, timed(name, label)) for name, label in steps]
            for _ in range(args.repeat):
                spans.clear()
                written[0] = kept[0] = 0
                fp = job(sid, idx, fps, labels, mapped)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fp.write(sink)
                torch.cuda.synchronize()
                times[mapped].append(time.perf_counter() - t0)
                sizes[mapped] = (kept[0], written[0])
                if mapped:
                    device_ms.append({label: round(sum(a.elapsed_time(b) for a, b in ev), 3) for label, ev in spans.items()})
        for name, fn in real:
            setattr(dct_sim, name, fn)
    n = len(sid)
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    t_dom, t_map = times[False], times[True]
    return {'part': 'map', 'n': n, 'fingerprints': int(idx[-1]), 'families': args.families, 'family_size': args.family_size,
            'min_domain': min_domain, 'min_global': args.min_global, 'map_bound': bound, 'route': fp.route,
            'domain_lines': sizes[False][0], 'domain_text_bytes': sizes[False][1], 'map_lines': sizes[True][0], 'map_text_bytes': sizes[True][1],
            'domains_s': [round(t, 3) for t in t_dom], 'map_s': [round(t, 3) for t in t_map],
            'domains_median_s': round(med(t_dom), 3), 'map_median_s': round(med(t_map), 3),
            'domains_spread_s': round(max(t_dom) - min(t_dom), 3), 'map_over_domains': round(med(t_map) / med(t_dom), 3),
            'domains_ns_per_byte': round(1e9 * med(t_dom) / sizes[False][1], 3), 'map_ns_per_byte': round(1e9 * med(t_map) / sizes[True][1], 3),
            'device_ms_of_median_run': device_ms[t_map.index(med(t_map))], 'device_ms_all': device_ms}


def part_base(args):
    """(child) a process that has only initialised the GPU and run one small distance tile: the RSS floor of the run."""
    import torch
    from dctdomain_amd.similarity import l1_matrix
    l1_matrix(np.zeros((4, 480), dtype=np.int8), np.zeros((4, 480), dtype=np.int8))
    torch.cuda.synchronize()
    return {'part': 'base'}


def _child_rss(cmd, timeout):
    """(completed process, its peak RSS in MiB): one fresh process per measurement.  ru_maxrss of RUSAGE_CHILDREN is the
    largest over every child so far, so None means "not above an earlier child's"."""
    before = resource.getrusage(resource.RUSAGE_CHILDREN).ru_maxrss
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    peak = resource.getrusage(resource.RUSAGE_CHILDREN).ru_maxrss
    return p, (round(peak / 1024) if peak > before else None)


def part_scale(args):
    from dctdomain_amd import dct_sim
    res = {'part': 'scale', 'n': args.n}
    with tempfile.TemporaryDirectory(dir=args.dir) as tmp:
        path = os.path.join(tmp, 's-dct.npz')
        rows = synth(path, args.n, 7)
        res['npz_MB'] = round(os.path.getsize(path) / 2 ** 20)
        res['data_MB'] = round(rows * 480 / 2 ** 20)
        res['two_buffers_MB'] = round(2 * dct_sim.AllPairs.TEXT_BYTES / 2 ** 20)
        text = int(dct_sim.row_text_bytes(np.full(args.n, 17)).sum())
        p, res['base_rss_MB'] = _child_rss([sys.executable, os.path.abspath(__file__), '--part', 'base'], args.timeout)
        cut = []
        for opt, v in (('--min-domain', args.min_domain), ('--min-global', args.min_global)):
            if v is not None:
                cut += [opt, str(v)]
        for name, sink in (('devnull', os.devnull), ('file', os.path.join(tmp, 'all.txt'))):
            if name == 'file' and not cut and shutil.disk_usage(tmp).free < text + (1 << 30):
                res[name] = {'skipped': f'{shutil.disk_usage(tmp).free / 1e9:.0f} GB free, {text / 1e9:.0f} GB of text'}
                continue
            cmd = [sys.executable, os.path.abspath(__file__), '--part', 'run', '--npz', path, '--sink', sink] + cut
            p, peak = _child_rss(cmd, args.timeout)
            if p.returncode != 0:
                res[name] = {'rc': p.returncode, 'stderr': p.stderr[-2000:]}
                break
            r = json.loads(p.stdout.strip().splitlines()[-1])
            r['peak_rss_MB'] = peak
            res[name] = r
            if name == 'file':
                os.unlink(sink)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', required=True, choices=['compare', 'scale', 'filter', 'cluster', 'domains', 'map', 'rows_link', 'run', 'base'])
    ap.add_argument('--n', type=int, default=2000)
    ap.add_argument('--dir', default=None, help='where the npz and the text file go (local disk)')
    ap.add_argument('--npz')
    ap.add_argument('--sink')
    ap.add_argument('--timeout', type=float, default=1200)
    ap.add_argument('--planted', type=int, default=1000, help='filter: fingerprints overwritten with near copies of others')
    ap.add_argument('--families', type=int, default=0, help='cluster / domains: families of near copies planted in the file')
    ap.add_argument('--family-size', type=int, default=100, help='cluster: proteins per planted family')
    ap.add_argument('--repeat', type=int, default=3, help='cluster / domains: runs of each path')
    ap.add_argument('--min-domain', type=float, default=None, help='scale / filter: print the pairs whose DCTdomain is not below this')
    ap.add_argument('--min-global', type=float, default=None, help='scale / filter: print the pairs whose DCTglobal is not below this')
    ap.add_argument('--out')
    args = ap.parse_args()
    res = {'compare': part_compare, 'scale': part_scale, 'filter': part_filter, 'cluster': part_cluster, 'domains': part_domains, 'map': part_map, 'rows_link': part_rows_link, 'run': part_run, 'base': part_base}[args.part](args)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'a') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
