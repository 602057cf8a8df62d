"""dct-sim --cluster --min-neighbors on the GPU (similarity.tri_degree = dctfp_tri_degree, similarity.tri_link_core =
dctfp_tri_link_core; DensityClusters; the command line) against the numpy rule of density_rule.py (worked by hand, pinned on the
reference fixture and checked against a textbook DBSCAN in test_density_host.py).

The tile of part 1 has 70 rows x 1030 columns -- two bands of 64 rows, the second partial, and two steps of 1024 columns, the second
of 6 -- the shape and the value mix of tests/test_medoid_gpu.py, with the bound and its successor among the values.  Everything is
compared exactly."""

import os

import numpy as np
import pytest

import all_sim_filter_rule as rule
import cluster_rule
import coverage_rule as cr
import density_rule as dr
import golden_util as gu
import medoid_rule as mr

pytestmark = pytest.mark.gpu
G6PD = os.path.join(gu.GOLD, 'ref_fixtures', 'G6PD-dct.npz')
N_ROWS, N_COLS, CAP, BOUND = 70, 1030, 17000, 8500
N_NODES = 1200
# (row0, col0): the diagonal through the middle of the tile, the tile wholly left of it (nothing counts), wholly right of it
PLACES = {'diagonal_inside': (500, 10), 'left_of_diagonal': (1100, 0), 'right_of_diagonal': (3, 100)}


def _values(rng, n_rows, n_cols, cap=CAP, bound=BOUND):
    """L1 values of every kind: 0, the bound, its successor, cap - 1, cap, 0x7fffffff, negative ones and ordinary ones."""
    t = rng.integers(0, cap + 2, size=(n_rows, n_cols))
    kind = rng.random((n_rows, n_cols))
    for lo, v in ((0.0, 0), (0.05, bound), (0.1, bound + 1), (0.15, cap - 1), (0.2, cap), (0.25, 0x7fffffff), (0.3, -5), (0.35, -0x80000000)):
        t[(kind >= lo) & (kind < lo + 0.05)] = v
    return t.astype(np.int32)


@pytest.fixture(scope='module')
def tile():
    """(values, row flags, column flags, views): the views are the tile as a contiguous tensor, with ld > n_cols, and from an odd
    column of a wider tensor with an odd row stride."""
    import torch
    rng = np.random.default_rng(23)
    t = _values(rng, N_ROWS, N_COLS)
    flags = (rng.random(N_ROWS) < 0.2, rng.random(N_COLS) < 0.2)
    dev = torch.as_tensor(t, device='cuda')
    wide = torch.full((N_ROWS, N_COLS + 50), 1, dtype=torch.int32, device='cuda')        # (1 would count if it were read)
    odd = torch.full((N_ROWS, N_COLS + 11), 1, dtype=torch.int32, device='cuda')
    views = {'contiguous': dev, 'wide_ld': wide[:, :N_COLS], 'odd_column': odd[:, 3:3 + N_COLS]}
    for v in views.values():
        v.copy_(dev)
    assert views['wide_ld'].stride(0) > N_COLS and views['odd_column'].stride(0) % 2 == 1 and views['odd_column'].data_ptr() % 16 == 12
    return t, flags, views


CORES = {'none': lambda rng: np.zeros(N_NODES, dtype=np.uint8), 'all': lambda rng: np.ones(N_NODES, dtype=np.uint8),
         'half': lambda rng: (rng.random(N_NODES) < 0.5).astype(np.uint8)}


def _degrees(view, row0, col0, flags=(None, None), bound=BOUND, deg=None):
    import torch
    from dctdomain_amd.similarity import tri_degree
    deg = deg if deg is not None else torch.zeros(N_NODES, dtype=torch.int32, device='cuda')
    tri_degree(view, row0, col0, bound, deg, *flags, cap=CAP)
    return deg.cpu().numpy().view(np.uint32)


def _fresh():
    import torch
    from dctdomain_amd.similarity import NEAREST_NONE
    return (torch.arange(N_NODES, dtype=torch.int32, device='cuda'), torch.full((N_NODES,), NEAREST_NONE, dtype=torch.int32, device='cuda'))


def _linked(view, row0, col0, core, flags=(None, None), bound=BOUND):
    """(labels, nearest) of one call on a fresh forest."""
    import torch
    from dctdomain_amd.similarity import cluster_labels, tri_link_core
    parent, nearest = _fresh()
    tri_link_core(view, row0, col0, bound, torch.as_tensor(core, device='cuda'), parent, nearest, *flags, cap=CAP)
    return cluster_labels(parent).cpu().numpy(), nearest.cpu().numpy()


# ---- 1. the two kernels against numpy on hand-made tiles

@pytest.mark.parametrize('place', sorted(PLACES))
def test_tri_degree_of_one_tile(tile, place):
    from dctdomain_amd.similarity import tri_filter_count
    t, flags, views = tile
    row0, col0 = PLACES[place]
    for use in ((None, None), flags):
        want = dr.tile_degrees(t, row0, col0, BOUND, *use, cap=CAP, n_nodes=N_NODES)
        assert want.any() == (place != 'left_of_diagonal')
        for name, view in views.items():
            assert np.array_equal(_degrees(view, row0, col0, use), want), (name, use[0] is not None)
        # the row side alone is tri_filter_count's count: every counted entry is counted once per end
        count = tri_filter_count(views['contiguous'], row0, col0, BOUND, *use, cap=CAP).cpu().numpy()
        assert int(want.sum()) == 2 * int(count.sum())
        if place == 'right_of_diagonal':                          # (rows and columns name different proteins there)
            assert np.array_equal(want[row0:row0 + N_ROWS], count) and count.any()
            assert int(want[col0:col0 + N_COLS].sum()) == int(count.sum())
    if place == 'diagonal_inside':
        plain, flagged = dr.tile_degrees(t, row0, col0, BOUND, n_nodes=N_NODES), dr.tile_degrees(t, row0, col0, BOUND, *flags, n_nodes=N_NODES)
        assert (plain != flagged).any() and plain[row0 + 64:row0 + N_ROWS].any() and plain[col0 + 1024:col0 + N_COLS].any()
        # the bound itself counts and its successor does not: entries of both values are there, so a bound one lower or one higher
        # gives other degrees; a bound of -1 and of cap: nothing and everything right of the diagonal
        assert not np.array_equal(dr.tile_degrees(t, row0, col0, BOUND - 1, n_nodes=N_NODES), plain)
        assert not np.array_equal(dr.tile_degrees(t, row0, col0, BOUND + 1, n_nodes=N_NODES), plain)
        for bound in (BOUND - 1, BOUND + 1, -1, 0, CAP):
            want = dr.tile_degrees(t, row0, col0, bound, *flags, cap=CAP, n_nodes=N_NODES)
            assert np.array_equal(_degrees(views['odd_column'], row0, col0, flags, bound), want), bound
        assert not _degrees(views['contiguous'], row0, col0, flags, -1).any()
        upper = int((col0 + np.arange(N_COLS)[None, :] > row0 + np.arange(N_ROWS)[:, None]).sum())
        assert int(_degrees(views['contiguous'], row0, col0, flags, CAP).sum()) == 2 * upper


@pytest.mark.parametrize('pattern', sorted(CORES))
@pytest.mark.parametrize('place', sorted(PLACES))
def test_tri_link_core_of_one_tile(tile, place, pattern):
    import torch
    from dctdomain_amd.similarity import NEAREST_NONE, cluster_labels, tri_link
    assert NEAREST_NONE == dr.NONE
    t, flags, views = tile
    row0, col0 = PLACES[place]
    core = CORES[pattern](np.random.default_rng(5))
    for use in ((None, None), flags):
        labels, nearest = dr.tile_link_core(t, row0, col0, BOUND, core, *use, cap=CAP)
        live = place != 'left_of_diagonal'
        assert (labels != np.arange(N_NODES)).any() == (live and pattern != 'none')
        assert (nearest != dr.NONE).any() == (live and pattern == 'half')
        for name, view in views.items():
            got_labels, got_nearest = _linked(view, row0, col0, core, use)
            assert np.array_equal(got_labels, labels) and np.array_equal(got_nearest, nearest), (name, use[0] is not None)
        if pattern == 'all':                                      # every counted entry is a union: tri_link's forest
            parent = torch.arange(N_NODES, dtype=torch.int32, device='cuda')
            tri_link(views['contiguous'], row0, col0, BOUND, parent, *use, cap=CAP)
            assert np.array_equal(cluster_labels(parent).cpu().numpy(), labels)
    if place == 'diagonal_inside' and pattern == 'half':
        labels, nearest = dr.tile_link_core(t, row0, col0, BOUND, core, *flags, cap=CAP)
        rows, cols = np.arange(row0, row0 + N_ROWS), np.arange(col0, col0 + N_COLS)
        assert not core[nearest != dr.NONE].any() and core[nearest[nearest != dr.NONE]].all()
        # non-core rows of the second band and non-core columns of the second step got a nearest core: both flushes ran
        assert (nearest[rows[64:]] != dr.NONE).any() and (nearest[col0 + 1024:col0 + N_COLS] != dr.NONE).any()
        assert (nearest[cols] != dr.NONE).sum() > 100


def test_sub_tiles_in_any_order_give_what_one_call_gives(tile):
    import torch
    from dctdomain_amd.similarity import cluster_labels, tri_degree, tri_link_core
    t, flags, views = tile
    row0, col0 = PLACES['diagonal_inside']
    core = CORES['half'](np.random.default_rng(7))
    core_dev = torch.as_tensor(core, device='cuda')
    want_deg = dr.tile_degrees(t, row0, col0, BOUND, *flags, cap=CAP, n_nodes=N_NODES)
    want_labels, want_nearest = dr.tile_link_core(t, row0, col0, BOUND, core, *flags, cap=CAP)
    parts = [(r0, r1, c0, c1) for r0, r1 in ((0, 37), (37, N_ROWS)) for c0, c1 in ((0, 513), (513, N_COLS))]
    for order in ((0, 1, 2, 3), (3, 1, 0, 2), (2, 3, 1, 0)):
        deg = torch.zeros(N_NODES, dtype=torch.int32, device='cuda')
        parent, nearest = _fresh()
        for k in order:
            r0, r1, c0, c1 = parts[k]
            part = views['odd_column'][r0:r1, c0:c1], row0 + r0, col0 + c0, BOUND
            tri_degree(*part, deg, flags[0][r0:r1], flags[1][c0:c1], cap=CAP)
            tri_link_core(*part, core_dev, parent, nearest, flags[0][r0:r1], flags[1][c0:c1], cap=CAP)
        assert np.array_equal(deg.cpu().numpy().view(np.uint32), want_deg), order
        assert np.array_equal(nearest.cpu().numpy(), want_nearest) and np.array_equal(cluster_labels(parent).cpu().numpy(), want_labels), order
    # a second pass over the same tile counts the same again (the caller zeroes deg) and changes neither nearest nor the forest
    assert np.array_equal(_degrees(views['contiguous'], row0, col0, flags, deg=deg), 2 * want_deg)
    tri_link_core(views['wide_ld'], row0, col0, BOUND, core_dev, parent, nearest, *flags, cap=CAP)
    assert np.array_equal(nearest.cpu().numpy(), want_nearest) and np.array_equal(cluster_labels(parent).cpu().numpy(), want_labels)


def test_the_exports_refuse_what_they_cannot_bound(tile):
    import torch
    from dctdomain_amd import _lib, similarity
    t, _, views = tile
    view = views['contiguous']
    dev = view.device
    room = torch.zeros(N_NODES + 1, dtype=torch.int32, device='cuda')
    core = torch.ones(N_NODES, dtype=torch.uint8, device='cuda')
    parent, nearest = _fresh()
    lead = (view.data_ptr(), N_ROWS, N_COLS, N_COLS, 0, 100, None, None, CAP, BOUND)

    def refused(name, *args):
        with pytest.raises(_lib.DctfpError) as err:
            similarity._launch(dev, name, *args)
        assert err.value.code == _lib.DCTFP_ERR_INVALID and err.value.msg.startswith(name + ': ')
        return err.value.msg

    for name, arrays in (('dctfp_tri_degree', (room.data_ptr(),)), ('dctfp_tri_link_core', (core.data_ptr(), parent.data_ptr(), nearest.data_ptr()))):
        assert 'outside' in refused(name, *lead, *arrays, 100 + N_COLS - 1)                  # the last column is no node
        assert 'outside' in refused(name, *lead[:4], N_NODES - N_ROWS + 1, 0, *lead[6:], *arrays, N_NODES)
        assert 'n_nodes' in refused(name, *lead, *arrays, -1)
        assert 'n_nodes' in refused(name, *lead, *arrays, 1 << 31)
        assert 'aligned' in refused(name, *lead, *arrays[:-1], arrays[-1] + 2, N_NODES)
        assert 'aligned' in refused(name, lead[0] + 2, *lead[1:], *arrays, N_NODES)
        assert 'NULL' in refused(name, None, *lead[1:], *arrays, N_NODES)
        for k in range(len(arrays)):
            assert 'NULL' in refused(name, *lead, *arrays[:k], None, *arrays[k + 1:], N_NODES)
        assert 'shape' in refused(name, *lead[:3], N_COLS - 1, *lead[4:], *arrays, N_NODES)
        assert 'shape' in refused(name, *lead[:1], -1, *lead[2:], *arrays, N_NODES)
        assert 'bound' in refused(name, *lead[:9], CAP + 1, *arrays, N_NODES)
    # the wrappers' own checks, and the empty tile: nothing launched
    deg = room[:N_NODES]
    with pytest.raises(IndexError):
        similarity.tri_degree(view, N_NODES - N_ROWS + 1, 0, BOUND, deg)
    with pytest.raises(ValueError):
        similarity.tri_degree(view, 0, 100, BOUND, deg.to(torch.int64))
    with pytest.raises(ValueError):
        similarity.tri_degree(view, 0, 100, BOUND, deg.cpu())
    with pytest.raises(IndexError):
        similarity.tri_link_core(view, 0, N_NODES - N_COLS + 1, BOUND, core, parent, nearest)
    with pytest.raises(ValueError):
        similarity.tri_link_core(view, 0, 100, BOUND, core[:-1], parent, nearest)
    with pytest.raises(ValueError):
        similarity.tri_link_core(view, 0, 100, BOUND, core.to(torch.int32), parent, nearest)
    with pytest.raises(ValueError):
        similarity.tri_link_core(view, 0, 100, BOUND, core, parent, nearest.to(torch.int64))
    for empty in (view[:0], view[:, :0]):
        similarity.tri_degree(empty, 0, 100, BOUND, deg)
        similarity.tri_link_core(empty, 0, 100, BOUND, core, parent, nearest)
    # nothing was written by any of these
    assert not room.any().item() and (nearest == similarity.NEAREST_NONE).all().item()
    assert torch.equal(parent, torch.arange(N_NODES, dtype=torch.int32, device='cuda'))


# ---- 2. DensityClusters

@pytest.fixture(scope='module')
def g6pd():
    with np.load(G6PD) as data:
        sid, idx, dct, dom = [str(s) for s in data['sid']], data['idx'], data['dct'], data['dom']
    tri = rule.triangle_l1(dct, idx)
    return {'sid': sid, 'idx': idx, 'dct': dct, 'dom': dom, 'tri': tri,
            'domain': mr.key_matrix(dct, idx, 'domain', tri), 'global': mr.key_matrix(dct, idx, 'global', tri)}


# the cases pinned in test_density_host.py, and both cut-offs at once
CASES = {'global0.6-m6': ({'min_global': 0.6}, 6, (15, 5, 7)), 'global0.6-m8': ({'min_global': 0.6}, 8, (4, 9, 14)),
         'global0.6-m12': ({'min_global': 0.6}, 12, (0, 0, 27)), 'global0.5-m8': ({'min_global': 0.5}, 8, (12, 1, 14)),
         'domain0.5-m12': ({'min_domain': 0.5}, 12, (27, 0, 0)), 'both-m6': ({'min_domain': 0.5, 'min_global': 0.6}, 6, (15, 5, 7))}


def _same(job, want):
    label, kind, deg = want
    got = job.labels()
    assert got.dtype == np.int32 and np.array_equal(got, label)
    assert job.kinds().dtype == np.uint8 and np.array_equal(job.kinds(), kind)
    assert job.degrees().dtype == np.int32 and np.array_equal(job.degrees(), deg)


@pytest.mark.parametrize('case', sorted(CASES))
def test_density_clusters_of_the_reference_fixture(g6pd, case, monkeypatch):
    from dctdomain_amd import dct_sim
    kw, m, counts = CASES[case]
    sid, idx, dct = g6pd['sid'], g6pd['idx'], g6pd['dct']
    want = dr.of_file(dct, idx, m, triangle=g6pd['tri'], **kw)
    assert dr.counts(want[1]) == counts
    fills = []
    for name in ('protein_min', 'l1_matrix'):
        monkeypatch.setattr(dct_sim, name, lambda *a, _fn=getattr(dct_sim, name), **k: (fills.append(1), _fn(*a, **k))[1])
    job = dct_sim.DensityClusters(sid, idx, dct, min_neighbors=m, **kw)
    assert len(list(job.stripes())) == 1
    got = job.labels()
    # one stripe: the tile of the first pass serves the second; with both cut-offs the pairs come from chunks(), twice
    assert len(fills) == (2 if case.startswith('both') else 1)
    assert np.array_equal(got, want[0])
    _same(job, want)
    # several stripes and column groups: the tiles are filled again, the result is the same
    for tile_ints, col_rows in ((90, 7), (5, 3), (1, 1)):
        small = dct_sim.DensityClusters(sid, idx, dct, min_neighbors=m, **kw)
        small.TILE_INTS, small.COL_ROWS = tile_ints, col_rows
        assert len(list(small.stripes())) > 2
        del fills[:]
        _same(small, want)
        assert len(fills) >= 2 * len(list(small.stripes()))


def test_one_neighbour_is_clusters_itself(g6pd):
    from dctdomain_amd import dct_sim
    sid, idx, dct = g6pd['sid'], g6pd['idx'], g6pd['dct']
    for kw in ({'min_domain': 0.9}, {'min_global': 0.6}, {'min_domain': 0.8, 'min_global': 0.5}):
        plain = dct_sim.Clusters(sid, idx, dct, **kw).labels()
        assert len(set(plain.tolist())) > 2
        job = dct_sim.DensityClusters(sid, idx, dct, min_neighbors=1, **kw)
        assert np.array_equal(job.labels(), plain) and np.array_equal(plain, cluster_rule.labels(dct, idx, **kw)[0])
        assert not (job.kinds() == dr.BORDER).any()


def test_a_coverage_decides_the_edges(g6pd):
    from dctdomain_amd import dct_sim
    sid, idx, dct = g6pd['sid'], g6pd['idx'], g6pd['dct']
    w = cr.weights(idx, g6pd['dom'], 'residues')
    for min_global, m, counts in ((None, 6, (20, 0, 7)), (None, 8, (12, 1, 14)), (0.6, 6, (15, 5, 7))):
        i, j, mn, last, keep = cr.edges(dct, idx, w, 0.5, 0.8, min_global)
        want = dr.clusters(27, i[keep], j[keep], m)
        plain = dr.of_file(dct, idx, m, triangle=g6pd['tri'], min_domain=0.5, min_global=min_global)
        assert dr.counts(want[1]) == counts
        # (alone, the coverage removes edges; every pair DCTglobal 0.6 keeps covers enough already)
        assert np.array_equal(want[2], plain[2]) == (min_global is not None)
        _same(dct_sim.DensityClusters(sid, idx, dct, min_domain=0.5, min_global=min_global, min_neighbors=m).with_coverage(0.8, w), want)
        small = dct_sim.DensityClusters(sid, idx, dct, min_domain=0.5, min_global=min_global, min_neighbors=m).with_coverage(0.8, w)
        small.TILE_INTS, small.COL_ROWS = 90, 7
        _same(small, want)


def test_medoids_of_density_clusters(g6pd, monkeypatch):
    from dctdomain_amd import dct_sim
    sid, idx, dct = g6pd['sid'], g6pd['idx'], g6pd['dct']
    for kw, m in (({'min_global': 0.6}, 6), ({'min_global': 0.5}, 8), ({'min_domain': 0.5, 'min_global': 0.6}, 6)):
        labels = dr.of_file(dct, idx, m, triangle=g6pd['tri'], **kw)[0]
        want = mr.medoids(g6pd['global'], labels)
        assert (want != labels).any()
        job = dct_sim.DensityClusters(sid, idx, dct, min_neighbors=m, **kw)
        assert np.array_equal(job.medoids(), want) and np.array_equal(job.last_labels, labels)
        small = dct_sim.DensityClusters(sid, idx, dct, min_neighbors=m, **kw)
        small.TILE_INTS, small.COL_ROWS = 90, 7
        assert np.array_equal(small.medoids(), want)
    # one stripe: the tile filled for the degrees serves the link pass and the sums
    fills = []
    for name in ('protein_min', 'l1_matrix'):
        monkeypatch.setattr(dct_sim, name, lambda *a, _fn=getattr(dct_sim, name), **k: (fills.append(1), _fn(*a, **k))[1])
    job = dct_sim.DensityClusters(sid, idx, dct, min_global=0.6, min_neighbors=6)
    job.medoids()
    assert len(fills) == 1


@pytest.fixture(scope='module')
def planar():
    """300 proteins of 1 .. 3 fingerprints (two of them without any) whose last rows are points of the plane: 60 % in six Gaussian
    blobs (sigma 14) on a grid, the rest uniform in +-120 -- dense families, thin bridges between them and scattered outliers; a
    protein's other rows are noise, far from everything.  L1 of two last rows = 240 (|dx| + |dy|)."""
    rng = np.random.default_rng(29)
    n, d = 300, 480
    counts = rng.integers(1, 4, size=n)
    centres = np.array([[-80, -80], [0, -80], [80, -80], [-80, 60], [0, 60], [80, 60]], dtype=float)
    blob = rng.random(n) < 0.6
    which = rng.integers(0, 6, size=n)
    xy = np.where(blob[:, None], centres[which] + rng.normal(0, 14, size=(n, 2)), rng.uniform(-120, 120, size=(n, 2)))
    xy = np.clip(np.rint(xy), -127, 127)
    counts[[41, 299]] = 0
    rows = []
    for p in np.flatnonzero(counts):
        r = rng.integers(-100, 101, size=(counts[p], d))
        r[-1] = np.repeat(xy[p], d // 2)
        rows.append(r)
    dct = np.concatenate(rows).astype(np.int8)
    idx = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return {'sid': [f'prot{p}' for p in range(n)], 'idx': idx, 'dct': dct, 'n': n, 'tri': rule.triangle_l1(dct, idx)}


PLANAR_CUTS = {'domain': {'min_domain': 0.5}, 'global': {'min_global': 0.6}, 'both': {'min_domain': 0.5, 'min_global': 0.6}}


@pytest.mark.parametrize('cut', sorted(PLANAR_CUTS))
def test_a_planar_file_with_all_three_kinds(planar, cut):
    from dctdomain_amd import dct_sim
    kw, m = PLANAR_CUTS[cut], 4
    sid, idx, dct, n = planar['sid'], planar['idx'], planar['dct'], planar['n']
    want = dr.of_file(dct, idx, m, triangle=planar['tri'], **kw)
    label, kind, deg = want
    assert min(dr.counts(kind)) >= 5 and kind[41] == dr.NOISE and kind[299] == dr.NOISE and deg[41] == 0 and deg[299] == 0
    single = cluster_rule.labels(dct, idx, **kw)[0]
    assert len(set(label.tolist())) > len(set(single.tolist())) and (np.bincount(label) > 1).sum() >= 1
    _same(dct_sim.DensityClusters(sid, idx, dct, min_neighbors=m, **kw), want)
    small = dct_sim.DensityClusters(sid, idx, dct, min_neighbors=m, **kw)
    small.TILE_INTS, small.COL_ROWS = 4000, 100
    assert len(list(small.stripes())) > 5
    _same(small, want)
    assert np.array_equal(dct_sim.DensityClusters(sid, idx, dct, min_neighbors=1, **kw).labels(), single)


# ---- 3. the command line

def _main(tmp_path, *argv, dct=G6PD) -> bytes:
    from dctdomain_amd import dct_sim
    out = str(tmp_path / 'out.txt')
    dct_sim.main(['--dct', dct, '--output', out] + list(argv))
    with open(out, 'rb') as fh:
        return fh.read()


def test_cli_prints_density_clusters(tmp_path, g6pd):
    sid, idx, dct = g6pd['sid'], g6pd['idx'], g6pd['dct']
    cut = ('--cluster', '--min-global', '0.6')
    labels = dr.of_file(dct, idx, 6, triangle=g6pd['tri'], min_global=0.6)[0]
    plain = _main(tmp_path, *cut)
    dense = _main(tmp_path, *cut, '--min-neighbors', '6')
    assert dense == cluster_rule.HEADER + cluster_rule.text(sid, labels) and dense != plain
    assert plain == cluster_rule.HEADER + cluster_rule.text(sid, cluster_rule.labels(dct, idx, min_global=0.6)[0])
    assert _main(tmp_path, *cut, '--min-neighbors', '1') == plain
    # the medoids of the density clusters, and --min-neighbors 1 beside --rep medoid
    assert _main(tmp_path, *cut, '--min-neighbors', '6', '--rep', 'medoid') == \
        cluster_rule.HEADER + mr.text(sid, labels, mr.medoids(g6pd['global'], labels))
    assert _main(tmp_path, *cut, '--min-neighbors', '1', '--rep', 'medoid') == _main(tmp_path, *cut, '--rep', 'medoid')
    # under a coverage
    cover = ('--cluster', '--min-domain', '0.5', '--min-coverage', '0.8')
    i, j, mn, last, keep = cr.edges(dct, idx, cr.weights(idx, g6pd['dom'], 'residues'), 0.5, 0.8)
    assert _main(tmp_path, *cover, '--min-neighbors', '6') == cluster_rule.HEADER + cluster_rule.text(sid, dr.clusters(27, i[keep], j[keep], 6)[0])
    assert _main(tmp_path, *cover, '--min-neighbors', '1') == _main(tmp_path, *cover)
