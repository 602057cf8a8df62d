"""dct-sim --cluster (dct_sim.Clusters; dctfp_tri_link / dctfp_link_pairs / dctfp_cluster_labels) against the numpy oracle of
cluster_rule.py (pinned on the CPU in test_cluster_host.py): the reference golden, the filtered mode's own edges on random ragged
files, independence from the partition, the kernels on hand-made tiles, pair lists, a chain of 2 000 proteins end to end and
200 000 proteins with planted families."""

import os
import time

import numpy as np
import pytest

import all_sim_filter_rule as rule
import cluster_rule as crule
import golden_util as gu

pytestmark = pytest.mark.gpu
NPZ = os.path.join(gu.GOLD, 'all_sim', 'all-dct.npz')
CUTS = [{'min_domain': x} for x in (0.1, 0.5, 0.9, 1.0)] + [{'min_global': y} for y in (0.1, 0.5, 0.9, 1.0)] + \
       [{'min_domain': 0.25, 'min_global': 0.1}, {'min_domain': 0.9, 'min_global': 0.5}, {'min_domain': 0.5, 'min_global': 0.9}]


def _run(path, out, min_domain=None, min_global=None) -> bytes:
    from dctdomain_amd import dct_sim
    argv = ['--dct', path, '--output', out, '--cluster']
    for name, v in (('--min-domain', min_domain), ('--min-global', min_global)):
        if v is not None:
            argv += [name, str(v)]
    dct_sim.main(argv)
    with open(out, 'rb') as fh:
        return fh.read()


def _load(path):
    with np.load(path) as data:
        return [str(s) for s in data['sid']], np.asarray(data['idx'], dtype=np.int64), data['dct']


# ---- 1. the reference golden

@pytest.mark.parametrize('kw', CUTS, ids=lambda kw: ','.join(f'{k[4:]}={v}' for k, v in kw.items()))
def test_reference_golden(tmp_path, kw):
    from dctdomain_amd import dct_sim
    sid, idx, dct = _load(NPZ)
    want, _ = crule.labels(dct, idx, **kw)
    got = dct_sim.Clusters(sid, idx, dct, **kw).labels()
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert _run(NPZ, str(tmp_path / 'out.txt'), **kw) == crule.HEADER + crule.text(sid, want)


def test_stdout_keeps_its_closing_lines(capfd):
    from dctdomain_amd import dct_sim
    sid, idx, dct = _load(NPZ)
    want = crule.text(sid, crule.labels(dct, idx, min_domain=0.9)[0]).decode('utf8').split('\n')[:-1]
    dct_sim.main(['--dct', NPZ, '--cluster', '--min-domain', '0.9'])
    got = capfd.readouterr().out.split('\n')
    assert got[0] == '#representative member' and len(want) == 139
    assert got[1].startswith('dct loaded for 139 sequences, time used: ')
    assert got[2:141] == want
    assert got[141].startswith('total time used ') and got[142].startswith('distance calculation used ') and got[143:] == ['']


def test_the_other_modes_print_what_they_printed(tmp_path):
    from dctdomain_amd import dct_sim
    lines = rule.read_lines(os.path.join(gu.GOLD, 'all_sim', 'expected.txt.gz'))
    _, idx, dct = _load(NPZ)
    _, _, mn, last = rule.triangle_l1(dct, idx)
    out = str(tmp_path / 'out.txt')
    dct_sim.main(['--dct', NPZ, '--output', out, '--min-domain', '0.5'])
    assert open(out, 'rb').read() == rule.filtered_text(lines, rule.kept(mn, last, 0.5))


# ---- 2. the components of the filtered mode's own edges, on random ragged files

_ALPHABET = list('abcdefghijklmnopqrstuvwxyz0123456789_|.-') + ['é', 'ß', 'α', '蛋', '😀']


def _ragged(seed, n):
    """Proteins of 0-3 fingerprints (15 % empty) from four families at L1 ~ 6 500 (0.62) within a family, plus planted near
    copies (+-2) of single fingerprints at random places of other proteins."""
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, 4, size=n)
    counts[rng.random(n) < 0.15] = 0
    idx = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    total = int(idx[-1])
    fam = rng.integers(-60, 61, size=(4, 480))
    dct = np.clip(fam[rng.integers(0, 4, size=total)] + rng.integers(-20, 21, size=(total, 480)), -127, 127).astype(np.int8)
    for _ in range(n // 4):
        a, b = rng.integers(0, total, size=2)
        dct[b] = np.clip(dct[a].astype(np.int64) + rng.integers(-2, 3, size=480), -127, 127)
    names = [''.join(rng.choice(_ALPHABET, size=int(m))) + f'{k}' for k, m in enumerate(rng.choice([1, 5, 17, 40, 333], size=n))]
    return names, idx, dct


_RAGGED_CUTS = [(0.62, None), (None, 0.62), (0.8, None), (None, 0.8), (0.62, 0.6), (0.6, 0.62), (0.8, 0.3), (1e-9, None), (None, 1.0)]


@pytest.mark.parametrize('seed,n', [(1, 60), (2, 150), (3, 2), (4, 300)])
def test_components_of_the_filtered_pairs(seed, n):
    from dctdomain_amd import dct_sim
    sid, idx, dct = _ragged(seed, n)
    assert (np.diff(idx) == 0).any() or n < 10
    seen = set()
    for min_domain, min_global in _RAGGED_CUTS:
        i, j, _, _ = dct_sim.FilteredPairs(sid, idx, dct, min_domain, min_global).pairs()
        want = crule.components(n, i, j)
        got = dct_sim.Clusters(sid, idx, dct, min_domain, min_global).labels()
        assert np.array_equal(got, want), (min_domain, min_global)
        assert np.array_equal(want, crule.labels(dct, idx, min_domain, min_global)[0])
        seen.add(len(np.unique(want)))
    assert n < 10 or len(seen) > 2                            # (the cut-offs fall inside, between and outside the families)


def test_a_copy_that_is_not_a_last_fingerprint_links_for_domain_only():
    from dctdomain_amd import dct_sim
    rng = np.random.default_rng(9)
    rows = rng.integers(-48, 49, size=(5, 480)).astype(np.int8)
    near = np.clip(rows[0].astype(np.int64) + rng.integers(-2, 3, size=480), -127, 127).astype(np.int8)
    dct = np.stack([rows[0], rows[1], near, rows[2], rows[3], rows[4]])      # A = [x, y], B = [x', z], C = [w], D = []
    idx = np.array([0, 2, 4, 5, 5, 6], dtype=np.int64)
    sid = ['A', 'B', 'C', 'D', 'E']
    assert dct_sim.Clusters(sid, idx, dct, min_domain=0.5).labels().tolist() == [0, 0, 2, 3, 4]
    assert dct_sim.Clusters(sid, idx, dct, min_global=0.5).labels().tolist() == [0, 1, 2, 3, 4]
    assert dct_sim.Clusters(sid, idx, dct, min_domain=0.5, min_global=0.5).labels().tolist() == [0, 1, 2, 3, 4]
    assert dct_sim.Clusters(sid, idx, dct, min_domain=0.5, min_global=0.01).labels().tolist() == \
        crule.labels(dct, idx, 0.5, 0.01)[0].tolist()


# ---- 3. independence from the partition

@pytest.mark.parametrize('kw', [{'min_domain': 0.62}, {'min_global': 0.62}, {'min_domain': 0.63, 'min_global': 0.6}])   # 30 / 37 / 46 clusters
def test_labels_do_not_depend_on_stripes_groups_or_ranges(monkeypatch, kw):
    from dctdomain_amd import dct_sim
    sid, idx, dct = _ragged(7, 90)
    want = crule.labels(dct, idx, **kw)[0]
    assert 2 < len(np.unique(want)) < 80
    first = dct_sim.Clusters(sid, idx, dct, **kw)
    assert np.array_equal(first.labels(), want) and np.array_equal(first.labels(), want)       # (twice: the same)
    texts = set()
    for tile_ints, col_rows, text_bytes in [(5, 3, 41), (1, 1, 1), (300, 3, 281), (90, 7, 1 << 28), (1000, 40, 100), (1 << 28, 2, 1 << 28)]:
        for name, v in (('TILE_INTS', tile_ints), ('COL_ROWS', col_rows), ('TEXT_BYTES', text_bytes)):
            monkeypatch.setattr(dct_sim.FilteredPairs, name, v)
        c = dct_sim.Clusters(sid, idx, dct, **kw)
        stripes = list(c.stripes())
        assert len(stripes) > 1 and (tile_ints > 1 or all(b - a == 1 for a, b in stripes))      # (one-row stripes among them)
        assert np.array_equal(c.labels(), want), (tile_ints, col_rows, text_bytes)
        got = []
        c.write(lambda mv: got.append(bytes(mv)))
        texts.add(b''.join(got))
    assert texts == {crule.text(sid, want)}


# ---- 4. the kernels on hand-made tiles: 0 is an edge, 17 000 is none

def _forest(n):
    import torch
    return torch.arange(n, dtype=torch.int32, device='cuda')


def _check(parent, want, extra=None):
    """Labels equal the oracle's; parent[x] <= x; cluster_labels twice gives the same; further links still work."""
    import torch
    from dctdomain_amd.similarity import cluster_labels, link_pairs
    n = parent.numel()
    got = cluster_labels(parent)
    assert got.dtype == torch.int32 and got.data_ptr() != parent.data_ptr()
    assert np.array_equal(got.cpu().numpy(), want)
    p = parent.cpu().numpy()
    assert (p <= np.arange(n)).all() and (p >= 0).all()
    assert np.array_equal(crule.components(n, np.arange(n), p), want)      # (parent is a forest of the same components)
    assert np.array_equal(cluster_labels(parent).cpu().numpy(), want)
    if extra is None:
        roots = np.unique(want)
        extra = (int(roots[-1]), int(roots[0]))
    a, b = extra
    link_pairs(torch.tensor([a], dtype=torch.int32, device='cuda'), torch.tensor([b], dtype=torch.int32, device='cuda'), parent)
    more = want.copy()
    la, lb = want[a], want[b]
    more[(want == la) | (want == lb)] = min(la, lb)
    assert np.array_equal(cluster_labels(parent).cpu().numpy(), more)
    assert (parent.cpu().numpy() <= np.arange(n)).all()


def _edge_tile(n, ei, ej):
    """(n, n) device tile: 17 000 everywhere, 0 at (min, max) of every edge."""
    import torch
    t = torch.full((n, n), 17000, dtype=torch.int32, device='cuda')
    lo, hi = np.minimum(ei, ej), np.maximum(ei, ej)
    t[torch.as_tensor(lo, device='cuda'), torch.as_tensor(hi, device='cuda')] = 0
    return t


def _timed_link(t, n):
    import torch
    from dctdomain_amd.similarity import cluster_labels, tri_link
    parent = _forest(n)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tri_link(t, 0, 0, 0, parent)
    labels = cluster_labels(parent)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, parent, labels


def test_chains_of_twenty_thousand_within_ten_times_the_random_case():
    """A chain makes the deepest forest a union-find without shortening can make: its time is held against the same tile size
    with as many random edges, measured here on the same device (after a warm-up), times ten."""
    n = 20000
    rng = np.random.default_rng(5)
    a, b = rng.integers(0, n, size=n - 1), rng.integers(0, n, size=n - 1)
    a, b = a[a != b], b[a != b]
    t = _edge_tile(n, a, b)
    _timed_link(t, n)                                         # (warm-up: kernels loaded, the allocator primed)
    t_random, parent, _ = min((_timed_link(t, n) for _ in range(3)), key=lambda r: r[0])
    _check(parent, crule.components(n, a, b))
    del t
    perm = rng.permutation(n)
    times = {}
    for name, order in (('chain', np.arange(n)), ('permuted chain', perm)):
        t = _edge_tile(n, order[:-1], order[1:])
        seconds, parent, labels = _timed_link(t, n)
        times[name] = seconds
        assert not labels.cpu().numpy().any()
        _check(parent, np.zeros(n, dtype=np.int32))
        del t
    print(f'\ncluster timing n={n}: random {1e3 * t_random:.3f} ms, chain {1e3 * times["chain"]:.3f} ms, '
          f'permuted chain {1e3 * times["permuted chain"]:.3f} ms (tri_link + cluster_labels)')
    assert times['chain'] <= 10 * t_random and times['permuted chain'] <= 10 * t_random, (times, t_random)


def test_star_and_bridge():
    from dctdomain_amd.similarity import tri_link
    n = 4000
    t = _edge_tile(n, np.arange(n - 1), np.full(n - 1, n - 1))          # a star whose centre is the largest index
    parent = _forest(n)
    tri_link(t, 0, 0, 0, parent)
    _check(parent, np.zeros(n, dtype=np.int32))
    # A = 0 .. m - 1 and n - 1 (a chain, and an edge from 0), B = m .. n - 2 (a chain); the bridge (n - 2, n - 1) is the last row's
    m = 1500
    ei = np.concatenate([np.arange(m - 1), [0], np.arange(m, n - 2)])
    ej = np.concatenate([np.arange(1, m), [n - 1], np.arange(m + 1, n - 1)])
    want = np.zeros(n, dtype=np.int32)
    want[m:n - 1] = m
    t = _edge_tile(n, ei, ej)
    parent = _forest(n)
    tri_link(t, 0, 0, 0, parent)
    _check(parent, want)
    t[n - 2, n - 1] = 0
    parent = _forest(n)
    tri_link(t[:-1], 0, 0, 0, parent)                         # (row n - 1 has nothing right of the diagonal)
    _check(parent, np.zeros(n, dtype=np.int32), extra=(5, 7))


def _np_edges(t, row0, col0, bound, row_empty=None, col_empty=None, cap=17000):
    key = np.minimum(t.astype(np.int64) & 0xffffffff, cap)    # (a negative value counts as cap)
    if row_empty is not None:
        key[np.asarray(row_empty, dtype=bool)] = cap
    if col_empty is not None:
        key[:, np.asarray(col_empty, dtype=bool)] = cap
    i = row0 + np.arange(t.shape[0])[:, None]
    j = col0 + np.arange(t.shape[1])[None, :]
    r, c = np.nonzero((j > i) & (key <= bound))
    return row0 + r, col0 + c


@pytest.mark.parametrize('n_rows,n_cols', [(7, 3000), (1, 5000), (40, 1), (3, 1023), (5, 1025), (9, 2048), (300, 37), (64, 64)])
@pytest.mark.parametrize('bound', [0, 8500])
def test_link_kernel_against_numpy(n_rows, n_cols, bound):
    """The bound exactly (an entry at `bound` links, one at `bound + 1` does not), entries left of the diagonal and beyond n_cols
    (the padding holds 0 = an edge if it were read), views with ld > n_cols at each of the four 4-byte alignments, the flags."""
    import torch
    from dctdomain_amd.similarity import tri_link
    rng = np.random.default_rng(1000 * n_rows + n_cols + bound)
    places = [(10, 5), (n_rows + 3, 0), (0, n_rows + 20), (0, 1), (0, 0), (3, 0)]
    for k, (col0, row0) in enumerate(places):
        t = np.full((n_rows, n_cols), bound + 1, dtype=np.int32)
        u = rng.random((n_rows, n_cols))
        t[u < 0.4] = 17000
        t[u > 1 - 1.5 / max(n_cols, 2)] = bound               # (sparse: about one and a half edges per row)
        t[u < 0.02] = -5
        pad, shift = int(rng.integers(1, 9)), k % 4
        big = torch.zeros((n_rows, n_cols + pad + shift), dtype=torch.int32, device='cuda')
        view = big[:, shift:shift + n_cols]
        view.copy_(torch.as_tensor(t, device='cuda'))
        assert view.stride(0) > n_cols and (view.data_ptr() - big.data_ptr()) == 4 * shift
        flags = [(None, None), (rng.random(n_rows) < 0.3, None), (None, rng.random(n_cols) < 0.3),
                 (rng.random(n_rows) < 0.2, rng.random(n_cols) < 0.2)][(k + n_rows) % 4]
        n = max(row0 + n_rows, col0 + n_cols) + int(rng.integers(0, 3))
        ei, ej = _np_edges(t, row0, col0, bound, *flags)
        parent = _forest(n)
        tri_link(view, row0, col0, bound, parent, *flags)
        _check(parent, crule.components(n, ei, ej))
        assert n_cols < 3 or (t == bound + 1).sum() > 0.3 * t.size           # (most entries sit one above the bound: none of them links)
    assert (big.cpu().numpy()[:, shift + n_cols:] == 0).all()


def test_link_calls_reject_bad_arguments_and_take_empty_ones():
    import ctypes as C
    import torch
    from dctdomain_amd import _lib
    from dctdomain_amd.similarity import cluster_labels, link_pairs, tri_link
    t = torch.zeros((6, 100), dtype=torch.int32, device='cuda')
    parent = _forest(100)
    ctx = _lib.get_context(0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda row0=0, col0=0, bound=0, ld=100, n_nodes=100, n_rows=6: ctx._lib.dctfp_tri_link(   # noqa: E731
        ctx.handle, t.data_ptr(), n_rows, 100, ld, row0, col0, None, None, 17000, bound, parent.data_ptr(), n_nodes, stream)
    assert call(col0=1) == _lib.DCTFP_ERR_INVALID and call(row0=95) == _lib.DCTFP_ERR_INVALID      # outside parent: on the host
    assert call(bound=17001) == _lib.DCTFP_ERR_INVALID and call(bound=-2) == _lib.DCTFP_ERR_INVALID and call(ld=99) == _lib.DCTFP_ERR_INVALID
    assert call(n_nodes=2 ** 31) == _lib.DCTFP_ERR_LIMIT
    assert ctx._lib.dctfp_link_pairs(ctx.handle, parent.data_ptr(), parent.data_ptr(), 3, parent.data_ptr(), 2 ** 31, stream) == _lib.DCTFP_ERR_LIMIT
    assert ctx._lib.dctfp_cluster_labels(ctx.handle, parent.data_ptr(), 2 ** 31, parent.data_ptr(), stream) == _lib.DCTFP_ERR_LIMIT
    assert ctx._lib.dctfp_link_pairs(ctx.handle, parent.data_ptr(), parent.data_ptr(), 2 ** 31 + 1, parent.data_ptr(), 100, stream) == _lib.DCTFP_ERR_LIMIT
    assert call(n_rows=0) == 0
    assert ctx._lib.dctfp_link_pairs(ctx.handle, None, None, 0, parent.data_ptr(), 100, stream) == 0
    assert ctx._lib.dctfp_cluster_labels(ctx.handle, parent.data_ptr(), 0, parent.data_ptr(), stream) == 0
    assert parent.cpu().tolist() == list(range(100))          # nothing was linked by any of these
    with pytest.raises(IndexError):
        tri_link(t, 0, 1, 0, parent)
    with pytest.raises(ValueError):
        tri_link(t, 0, 0, 0, parent.long())
    with pytest.raises(ValueError):
        link_pairs(parent[:3], parent[:2], parent)
    assert cluster_labels(_forest(0)).numel() == 0
    assert call(bound=-1) == 0 and cluster_labels(parent).cpu().tolist() == list(range(100))      # bound -1: nothing survives
    assert call() == 0 and not cluster_labels(parent).cpu().numpy().any()


def test_labels_of_a_forest_handed_in_as_one_long_path():
    """cluster_labels on a forest no link made: parent[x] = x - 1, depth n.  Path halving by all threads keeps it short."""
    import torch
    from dctdomain_amd.similarity import cluster_labels
    n = 200000
    parent = torch.arange(-1, n - 1, dtype=torch.int32, device='cuda')
    parent[0] = 0
    parent[n // 2] = n // 2
    want = np.zeros(n, dtype=np.int32)
    want[n // 2:] = n // 2
    assert np.array_equal(cluster_labels(parent).cpu().numpy(), want)
    assert np.array_equal(parent.cpu().numpy(), want)         # (flattened: every node under its root)


# ---- 5. lists of pairs

@pytest.mark.parametrize('n,m', [(50, 30), (1000, 700), (100000, 150000), (7, 0)])
def test_link_pairs_against_the_oracle(n, m):
    import torch
    from dctdomain_amd.similarity import link_pairs
    rng = np.random.default_rng(n + m)
    pi, pj = rng.integers(0, n, size=m), rng.integers(0, n, size=m)
    if m > 20:
        pi[:5], pj[:5] = pj[5:10], pi[5:10]                   # repeats (both ways round)
        pi[10:13] = pj[10:13]                                 # self pairs
        pi[13:17] = [-1, n, 3, 2 ** 31 - 1]                   # out of range: skipped
        pj[13:17] = [4, 5, n + 7, 0]
    ok = (pi >= 0) & (pi < n) & (pj >= 0) & (pj < n)
    parent = _forest(n)
    dev = lambda a: torch.as_tensor(a.astype(np.int32), device='cuda')   # noqa: E731
    half = m // 2
    link_pairs(dev(pi[:half]), dev(pj[:half]), parent)
    link_pairs(dev(pi[half:]), dev(pj[half:]), parent)
    _check(parent, crule.components(n, pi[ok], pj[ok]))


def _thermometer(levels):
    """One int8 fingerprint per level: L1 between two of them = the difference of their levels (a path through the 480
    coordinates, 250 units along each)."""
    lv = np.asarray(levels, dtype=np.int64)[:, None]
    return (np.clip(lv - 250 * np.arange(480)[None, :], 0, 250) - 125).astype(np.int8)


def test_the_second_cut_off_removes_a_bridge():
    from dctdomain_amd import dct_sim
    levels = [0, 100, 5100, 5200, 5250, 40000]                # A-B and C-D-E close, B-C at L1 5 000 = 0.706, F alone
    dct = _thermometer(levels)
    idx = np.arange(7, dtype=np.int64)
    sid = list('ABCDEF')
    _, _, mn, last = rule.triangle_l1(dct, idx)
    assert mn[0] == 100 and mn[5] == 5000 and np.array_equal(mn, last)
    assert dct_sim.Clusters(sid, idx, dct, min_global=0.5).labels().tolist() == [0, 0, 0, 0, 0, 5]
    two = dct_sim.Clusters(sid, idx, dct, min_domain=0.9, min_global=0.5)
    assert (two.route, two.bound_domain < 17000) == ('global', True)
    assert two.labels().tolist() == [0, 0, 2, 2, 2, 5] == crule.labels(dct, idx, 0.9, 0.5)[0].tolist()


# ---- 6. end to end on a chain

def test_a_shuffled_chain_of_two_thousand_proteins(tmp_path):
    from dctdomain_amd import dct_sim
    assert dct_sim.sim_bound(0.9995) == 8
    n = 2000
    rng = np.random.default_rng(17)
    place = rng.permutation(n)                                # chain position of the protein at each file index
    for cut_at in (None, n // 2):
        keep = place != cut_at if cut_at is not None else np.ones(n, dtype=bool)
        pos = place[keep]
        dct = _thermometer(5 * pos)                           # neighbours at L1 5, the next ones at 10 > 8
        m = len(pos)
        sid = [f'chain{k:04d}' for k in range(m)]
        path = str(tmp_path / f'chain{m}-dct.npz')
        np.savez(path, sid=np.array(sid), idx=np.arange(m + 1, dtype=np.int64), dom=np.array(['1-9'] * m), dct=dct)
        got = _run(path, str(tmp_path / 'out.txt'), min_domain=0.9995)
        if cut_at is None:
            want = np.zeros(m, dtype=np.int32)                # one cluster, its representative index 0 of the file
        else:
            low = pos < cut_at
            want = np.where(low, np.flatnonzero(low)[0], np.flatnonzero(~low)[0]).astype(np.int32)
            assert len(np.unique(want)) == 2
        assert got == crule.HEADER + crule.text(sid, want)
        assert np.array_equal(dct_sim.Clusters(sid, np.arange(m + 1), dct, min_global=0.9995).labels(), want)


# ---- 7. scale

def test_two_hundred_thousand_proteins_fall_into_the_planted_families(tmp_path):
    """synth's random proteins (1-8 uniform int8 rows in [-48, 48]) lie at L1 15 500 +- 500 from each other, the minimum over at
    most 64 row pairs some 2.5 standard deviations lower: 14 standard deviations above --min-domain 0.5's bound of 8 500, so
    unrelated proteins share no edge -- a condition on the input, checked below with the oracle on a sample.  Members of a family
    are copies of its first member's rows within +-2 each (L1 <= 1 920 between any two), so the components are the families."""
    from dctdomain_amd import dct_sim
    from tools.all_sim_bench import synth
    n, n_fam = 200000, 3000
    path = str(tmp_path / 's-dct.npz')
    synth(path, n, 7)
    sid, idx, dct = _load(path)
    rng = np.random.default_rng(29)
    sizes = rng.choice([2, 3, 5, 12, 40], size=n_fam, p=[.5, .2, .15, .1, .05])
    chosen = rng.choice(n, size=int(sizes.sum()), replace=False)
    want = np.arange(n, dtype=np.int32)
    per = {}
    start = 0
    for size in sizes:
        members = chosen[start:start + size]
        start += size
        src = dct[idx[members[0]]:idx[members[0] + 1]].astype(np.int64)
        for p in members[1:]:
            per[int(p)] = np.clip(src + rng.integers(-2, 3, size=src.shape), -127, 127).astype(np.int8)
        want[members] = members.min()
    counts = np.diff(idx)
    for p, rows in per.items():
        counts[p] = len(rows)
    new_idx = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    new = np.empty((int(new_idx[-1]), 480), dtype=np.int8)
    as_it_was = np.ones(n, dtype=bool)
    as_it_was[list(per)] = False
    new[np.repeat(as_it_was, counts)] = dct[np.repeat(as_it_was, np.diff(idx))]
    for p, rows in per.items():
        new[new_idx[p]:new_idx[p + 1]] = rows
    dct, idx = new, new_idx
    # the condition on the input: 3 000 random pairs outside the families, and members against strangers
    ri, rj = rng.integers(0, n, size=3000), rng.integers(0, n, size=3000)
    rj[:1000] = chosen[rng.integers(0, len(chosen), size=1000)]
    ok = want[ri] != want[rj]
    rm, rl = rule.pair_l1(dct, idx, ri[ok], rj[ok])
    assert ok.sum() > 2900 and not rule.kept(rm, rl, min_domain=0.5).any() and rm.min() > 8500 + 3000
    fi = chosen[:sizes[0]]
    fm, _ = rule.pair_l1(dct, idx, np.repeat(fi[0], len(fi) - 1), fi[1:])
    assert fm.max() <= 1920
    got = dct_sim.Clusters(sid, idx, dct, min_domain=0.5).labels()
    assert np.array_equal(got, want)
    assert len(np.unique(got)) == n - int(sizes.sum()) + n_fam
