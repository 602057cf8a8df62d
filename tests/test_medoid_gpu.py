"""dct-sim --cluster --rep medoid on the GPU (similarity.label_sums = dctfp_label_sums; Clusters.medoids; the command line) against
the numpy rule of medoid_rule.py (worked by hand and pinned on the reference fixture in test_medoid_host.py).

The tile of part 1 has 70 rows x 1030 columns -- two bands of 64 rows, the second partial, and two steps of 1024 columns, the second
of 6 -- the shape tests/test_tri_walk_gpu.py uses.  All sums are compared as exact uint64."""

import os

import numpy as np
import pytest

import all_sim_filter_rule as rule
import cluster_rule
import coverage_rule as cr
import golden_util as gu
import medoid_rule as mr

pytestmark = pytest.mark.gpu
G6PD = os.path.join(gu.GOLD, 'ref_fixtures', 'G6PD-dct.npz')
N_ROWS, N_COLS, CAP = 70, 1030, 17000
MAX_CAP = 0xffffffff // 1024          # a row's partial sum of 1024 keys stays in 32 bits (a column's has 64)
N_NODES = 1200
# (row0, col0): the diagonal through the middle of the tile, the tile wholly left of it (nothing counts), wholly right of it
PLACES = {'diagonal_inside': (500, 10), 'left_of_diagonal': (1100, 0), 'right_of_diagonal': (3, 100)}
LABELS = {'one': np.zeros(N_NODES, dtype=np.int32), 'own': np.arange(N_NODES, dtype=np.int32),
          'five': (np.arange(N_NODES) * 7 % 5).astype(np.int32)}


def _values(rng, n_rows, n_cols, cap=CAP):
    """L1 values of every kind: 0, cap - 1, cap, 0x7fffffff, negative ones and ordinary ones."""
    t = rng.integers(0, cap + 2, size=(n_rows, n_cols))
    kind = rng.random((n_rows, n_cols))
    for lo, v in ((0.0, 0), (0.1, cap - 1), (0.2, cap), (0.3, 0x7fffffff), (0.4, -5), (0.45, -0x80000000)):
        t[(kind >= lo) & (kind < lo + 0.05)] = v
    return t.astype(np.int32)


@pytest.fixture(scope='module')
def tile():
    """(values, row flags, column flags, views): the views are the tile as a contiguous tensor, with ld > n_cols, and from an odd
    column of a wider tensor with an odd row stride (no two successive rows share a 16-byte shift)."""
    import torch
    rng = np.random.default_rng(11)
    t = _values(rng, N_ROWS, N_COLS)
    flags = (rng.random(N_ROWS) < 0.2, rng.random(N_COLS) < 0.2)
    dev = torch.as_tensor(t, device='cuda')
    wide = torch.full((N_ROWS, N_COLS + 50), 1, dtype=torch.int32, device='cuda')        # (1 would be added if it were read)
    odd = torch.full((N_ROWS, N_COLS + 11), 1, dtype=torch.int32, device='cuda')
    views = {'contiguous': dev, 'wide_ld': wide[:, :N_COLS], 'odd_column': odd[:, 3:3 + N_COLS]}
    for v in views.values():
        v.copy_(dev)
    assert views['wide_ld'].stride(0) > N_COLS and views['odd_column'].stride(0) % 2 == 1 and views['odd_column'].data_ptr() % 16 == 12
    return t, flags, views


def _sums(view, row0, col0, labels, flags=(None, None), cap=CAP, n_nodes=N_NODES):
    import torch
    from dctdomain_amd.similarity import label_sums
    sums = torch.zeros(n_nodes, dtype=torch.int64, device='cuda')
    label_sums(view, row0, col0, torch.as_tensor(labels, device='cuda'), sums, *flags, cap=cap)
    return sums.cpu().numpy().view(np.uint64)


# ---- 1. label_sums against numpy on hand-made tiles

@pytest.mark.parametrize('pattern', sorted(LABELS))
@pytest.mark.parametrize('place', sorted(PLACES))
def test_label_sums_of_one_tile(tile, place, pattern):
    t, flags, views = tile
    row0, col0 = PLACES[place]
    labels = LABELS[pattern]
    for use in ((None, None), flags):
        want = mr.tile_sums(t, row0, col0, labels, *use)
        assert want.any() == (place != 'left_of_diagonal' and pattern != 'own')
        for name, view in views.items():
            assert np.array_equal(_sums(view, row0, col0, labels, use), want), (name, use[0] is not None)
    if place == 'diagonal_inside' and pattern == 'one':
        plain, flagged = mr.tile_sums(t, row0, col0, labels), mr.tile_sums(t, row0, col0, labels, *flags)
        assert (plain != flagged).any() and plain[row0 + 64:row0 + N_ROWS].any() and plain[col0 + 1024:col0 + N_COLS].any()
        assert int(plain.max()) > 1 << 22                        # (beyond anything 32-bit partial sums of a smaller cap would hide)


def test_the_largest_cap_fills_the_partial_sums_and_the_next_is_refused():
    """A full band x a full step of 0x7fffffff under one label: every row's partial sum is 1024 x cap = 2^32 - 1024."""
    import torch
    from dctdomain_amd import _lib
    t = np.full((64, 1024), 0x7fffffff, dtype=np.int32)
    labels = np.zeros(2000, dtype=np.int32)
    view = torch.as_tensor(t, device='cuda')
    want = mr.tile_sums(t, 0, 64, labels, cap=MAX_CAP)
    assert int(want[0]) == 1024 * MAX_CAP == (1 << 32) - 1024 and int(want[64]) == 64 * MAX_CAP
    assert np.array_equal(_sums(view, 0, 64, labels, cap=MAX_CAP, n_nodes=2000), want)
    with pytest.raises(_lib.DctfpError) as err:
        _sums(view, 0, 64, labels, cap=MAX_CAP + 1, n_nodes=2000)
    assert err.value.code == _lib.DCTFP_ERR_INVALID and 'dctfp_label_sums' in err.value.msg and str(MAX_CAP) in err.value.msg


def test_sub_tiles_in_any_order_add_up_to_one_call(tile):
    import torch
    from dctdomain_amd.similarity import label_sums
    t, flags, views = tile
    row0, col0 = PLACES['diagonal_inside']
    labels = LABELS['five']
    want = mr.tile_sums(t, row0, col0, labels, *flags)
    lab = torch.as_tensor(labels, device='cuda')
    parts = [(r0, r1, c0, c1) for r0, r1 in ((0, 37), (37, N_ROWS)) for c0, c1 in ((0, 513), (513, N_COLS))]
    got = []
    for order in ((0, 1, 2, 3), (3, 1, 0, 2), (2, 3, 1, 0)):
        sums = torch.zeros(N_NODES, dtype=torch.int64, device='cuda')
        for k in order:
            r0, r1, c0, c1 = parts[k]
            label_sums(views['odd_column'][r0:r1, c0:c1], row0 + r0, col0 + c0, lab, sums, flags[0][r0:r1], flags[1][c0:c1])
        got.append(sums.cpu().numpy().view(np.uint64))
    assert all(np.array_equal(g, want) for g in got)
    # a second pass over the same tile adds the same again: the caller zeroes the sums
    label_sums(views['contiguous'], row0, col0, lab, sums, *flags)
    assert np.array_equal(sums.cpu().numpy().view(np.uint64), 2 * want)


def test_the_export_refuses_what_it_cannot_bound(tile):
    import torch
    from dctdomain_amd import _lib, similarity
    t, _, views = tile
    view = views['contiguous']
    dev = view.device
    labels = torch.zeros(N_NODES, dtype=torch.int32, device='cuda')
    room = torch.zeros(N_NODES + 1, dtype=torch.int64, device='cuda')
    lead = (view.data_ptr(), N_ROWS, N_COLS, N_COLS, 0, 100, None, None, CAP, CAP)

    def refused(*args):
        with pytest.raises(_lib.DctfpError) as err:
            similarity._launch(dev, 'dctfp_label_sums', *args)
        assert err.value.code == _lib.DCTFP_ERR_INVALID and 'dctfp_label_sums' in err.value.msg
        return err.value.msg

    assert 'outside' in refused(*lead, labels.data_ptr(), room.data_ptr(), 100 + N_COLS - 1)      # the last column is no node
    assert 'outside' in refused(*lead[:4], N_NODES - N_ROWS + 1, 0, *lead[6:], labels.data_ptr(), room.data_ptr(), N_NODES)
    assert 'aligned' in refused(*lead, labels.data_ptr(), room.data_ptr() + 4, N_NODES)
    assert 'NULL' in refused(*lead, None, room.data_ptr(), N_NODES)
    assert 'NULL' in refused(*lead, labels.data_ptr(), None, N_NODES)
    assert 'shape' in refused(*lead[:3], N_COLS - 1, *lead[4:], labels.data_ptr(), room.data_ptr(), N_NODES)
    assert not room.any().item()
    # the wrapper's own checks, and the empty tile: nothing launched, nothing written
    sums = room[:N_NODES]
    with pytest.raises(IndexError):
        similarity.label_sums(view, N_NODES - N_ROWS + 1, 0, labels, sums)
    with pytest.raises(ValueError):
        similarity.label_sums(view, 0, 100, labels, room)
    with pytest.raises(ValueError):
        similarity.label_sums(view, 0, 100, labels.to(torch.int64), sums)
    similarity.label_sums(view[:0], 0, 100, labels, sums)
    similarity.label_sums(view[:, :0], 0, 100, labels, sums)
    assert not room.any().item()


# ---- 2. Clusters.medoids

@pytest.fixture(scope='module')
def g6pd():
    with np.load(G6PD) as data:
        sid, idx, dct, dom = [str(s) for s in data['sid']], data['idx'], data['dct'], data['dom']
    tri = rule.triangle_l1(dct, idx)
    return {'sid': sid, 'idx': idx, 'dct': dct, 'dom': dom, 'tri': tri,
            'domain': mr.key_matrix(dct, idx, 'domain', tri), 'global': mr.key_matrix(dct, idx, 'global', tri)}


CUTS = {'domain': {'min_domain': 0.5}, 'global': {'min_global': 0.5}, 'both': {'min_domain': 0.5, 'min_global': 0.5}}


@pytest.mark.parametrize('cut', sorted(CUTS))
def test_medoids_of_the_reference_fixture(g6pd, cut, monkeypatch):
    from dctdomain_amd import dct_sim
    kw = CUTS[cut]
    sid, idx, dct = g6pd['sid'], g6pd['idx'], g6pd['dct']
    labels, _ = cluster_rule.labels(dct, idx, **kw)
    want = mr.medoids(g6pd[mr.route_of(kw.get('min_global'))], labels)
    if cut == 'domain':
        assert want.tolist() == [11] * 27
    else:
        assert [int(want[c]) for c in (0, 8, 21)] == [7, 14, 24] and int((want != np.arange(27)).sum()) == 13 + 7 + 6 - 3
    fills = []
    for name in ('protein_min', 'l1_matrix'):
        monkeypatch.setattr(dct_sim, name, lambda *a, _fn=getattr(dct_sim, name), **k: (fills.append(1), _fn(*a, **k))[1])
    job = dct_sim.Clusters(sid, idx, dct, **kw)
    got = job.medoids()
    assert got.dtype == np.int32 and np.array_equal(got, want) and np.array_equal(job.last_labels, labels)
    # one stripe that tri_link read: the tile of the first pass is kept; with both cut-offs the pairs came from chunks(): filled again
    assert len(fills) == (2 if cut == 'both' else 1)
    assert np.array_equal(job.medoids(labels), want)              # labels it gave before: one pass of sums
    # several stripes and column groups: the tiles are filled again, the result is the same
    for tile_ints, col_rows in ((90, 7), (5, 3), (1, 1)):
        small = dct_sim.Clusters(sid, idx, dct, **kw)
        small.TILE_INTS, small.COL_ROWS = tile_ints, col_rows
        assert len(list(small.stripes())) > 2
        assert np.array_equal(small.medoids(), want), (tile_ints, col_rows)


def test_a_coverage_decides_membership_and_the_plain_distances_the_medoid(g6pd):
    from dctdomain_amd import dct_sim
    sid, idx, dct = g6pd['sid'], g6pd['idx'], g6pd['dct']
    n = len(sid)
    w = cr.weights(idx, g6pd['dom'], 'residues')
    i, j, mn, last, keep = cr.edges(dct, idx, w, 0.5, 0.8)
    labels = cr.components(n, i, j, keep)
    assert len(set(labels.tolist())) == 4
    want = mr.medoids(g6pd['domain'], labels)                     # the UNMASKED keys with the coverage's labels
    # pairs the coverage rejected inside one cluster exist, and masking them would name another protein
    rejected = ~keep & (labels[i] == labels[j]) & (mn <= 8500)
    masked = g6pd['domain'].copy()
    masked[i[~keep], j[~keep]] = masked[j[~keep], i[~keep]] = 17000
    assert rejected.any() and not np.array_equal(mr.medoids(masked, labels), want)
    job = dct_sim.Clusters(sid, idx, dct, min_domain=0.5).with_coverage(0.8, w)
    assert np.array_equal(job.medoids(), want) and np.array_equal(job.last_labels, labels)
    small = dct_sim.Clusters(sid, idx, dct, min_domain=0.5).with_coverage(0.8, w)
    small.TILE_INTS, small.COL_ROWS = 90, 7
    assert np.array_equal(small.medoids(), want)


@pytest.fixture(scope='module')
def planted():
    """300 proteins of 1 .. 4 fingerprints in 30 planted families (a family's k-th fingerprints are near each other, everything
    else is far), two of them without any fingerprint."""
    rng = np.random.default_rng(17)
    n, d, families = 300, 480, 30
    base = rng.integers(-50, 51, size=(families, 4, d))
    family = rng.integers(0, families, size=n)
    counts = rng.integers(1, 5, size=n)
    counts[[41, 299]] = 0
    idx = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rows = [base[family[p], :counts[p]] + rng.integers(-3, 4, size=(counts[p], d)) * rng.integers(1, 4) for p in range(n)]
    dct = np.concatenate(rows).astype(np.int8)
    sid = [f'prot{p}' for p in range(n)]
    tri = rule.triangle_l1(dct, idx)
    return {'sid': sid, 'idx': idx, 'dct': dct, 'tri': tri, 'n': n,
            'domain': mr.key_matrix(dct, idx, 'domain', tri), 'global': mr.key_matrix(dct, idx, 'global', tri)}


@pytest.mark.parametrize('cut', sorted(CUTS) + ['none'])
def test_medoids_of_a_random_file_with_empty_proteins(planted, cut):
    from dctdomain_amd import dct_sim
    kw = CUTS.get(cut, {'min_domain': 0.0})                       # 'none': no cut-off excludes anything -- one cluster, no linking pass
    sid, idx, dct, n = planted['sid'], planted['idx'], planted['dct'], planted['n']
    i, j, mn, last = planted['tri']
    labels = cluster_rule.components(n, *(v[rule.kept(mn, last, **kw)] for v in (i, j)))
    sizes = np.bincount(labels)
    assert (sizes.max() == n) if cut == 'none' else ((sizes > 2).sum() > 5 and labels[41] == 41 and labels[299] == 299)
    key = planted[mr.route_of(kw.get('min_global'))]
    want = mr.medoids(key, labels)
    assert (want != labels).sum() > 20
    job = dct_sim.Clusters(sid, idx, dct, **kw)
    assert np.array_equal(job.medoids(), want) and np.array_equal(job.last_labels, labels)
    # labels of the caller's put the proteins without fingerprints inside clusters: 17000 to everyone, on either route
    mixed = cluster_rule.components(n, np.arange(n - 7), np.arange(7, n))             # seven clusters: the residues mod 7
    assert np.array_equal(job.medoids(mixed), mr.medoids(key, mixed))
    small = dct_sim.Clusters(sid, idx, dct, **kw)
    small.TILE_INTS, small.COL_ROWS = 4000, 100
    assert len(list(small.stripes())) > 5 and np.array_equal(small.medoids(), want)


# ---- 3. the command line

def _main(tmp_path, *argv, dct=G6PD) -> bytes:
    from dctdomain_amd import dct_sim
    out = str(tmp_path / 'out.txt')
    dct_sim.main(['--dct', dct, '--output', out] + list(argv))
    with open(out, 'rb') as fh:
        return fh.read()


def test_cli_names_clusters_by_their_medoids(tmp_path, g6pd):
    from dctdomain_amd import dct_sim
    sid, idx, dct = g6pd['sid'], g6pd['idx'], g6pd['dct']
    labels = np.zeros(27, dtype=np.int32)
    assert _main(tmp_path, '--cluster', '--min-domain', '0.5', '--rep', 'medoid') == cluster_rule.HEADER + mr.text(sid, labels, [11] * 27)
    plain = _main(tmp_path, '--cluster', '--min-domain', '0.5')
    assert plain == cluster_rule.HEADER + cluster_rule.text(sid, labels)
    assert _main(tmp_path, '--cluster', '--min-domain', '0.5', '--rep', 'first') == plain
    # DCTglobal's clusters, the medoids written out and read back, and the file placed on them
    labels, _ = cluster_rule.labels(dct, idx, min_global=0.5)
    rep = mr.medoids(g6pd['global'], labels)
    reps_out = str(tmp_path / 'medoids-dct.npz')
    text = _main(tmp_path, '--cluster', '--min-global', '0.5', '--rep', 'medoid', '--reps-out', reps_out)
    assert text == cluster_rule.HEADER + mr.text(sid, labels, rep)
    chosen = rep[np.flatnonzero(labels == np.arange(27))]         # one per cluster, in the order of the clusters' smallest members
    assert chosen.tolist()[:3] == [7, 6, 14] and len(set(chosen.tolist())) == len(chosen) == len(set(labels.tolist()))
    rsid, ridx, rfps = dct_sim._load_npz(reps_out)
    assert [str(s) for s in rsid] == [sid[k] for k in chosen]
    assert np.array_equal(np.diff(ridx), np.diff(idx)[chosen])
    assert np.array_equal(rfps, np.concatenate([dct[idx[k]:idx[k + 1]] for k in chosen]))
    with np.load(reps_out) as data:
        assert len(data['dom']) == len(data['dct'])
    lines = _main(tmp_path, '--assign', reps_out, '--min-global', '0.5').split(b'\n')[1:-1]
    placed = dict(reversed(x.decode('utf8').split(' ')) for x in lines)
    assert len(placed) == 27 and all(placed[sid[k]] == sid[k] for k in chosen)
    # under a coverage: the labels of the coverage, the medoids of the plain distances
    i, j, mn, last, keep = cr.edges(dct, idx, cr.weights(idx, g6pd['dom'], 'residues'), 0.5, 0.8)
    labels = cr.components(27, i, j, keep)
    text = _main(tmp_path, '--cluster', '--min-domain', '0.5', '--min-coverage', '0.8', '--rep', 'medoid')
    assert text == cluster_rule.HEADER + mr.text(sid, labels, mr.medoids(g6pd['domain'], labels))
