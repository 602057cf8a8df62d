"""dct-sim --auc1 on the GPU (similarity.tri_first_fp = dctfp_tri_first_fp, similarity.tri_tp_before = dctfp_tri_tp_before; Auc1;
the command line) against the numpy rule of auc1_rule.py (worked by hand and pinned on the reference fixture in
test_auc1_host.py).

The tile of part 1 is that of tests/test_density_gpu.py: 70 rows x 1030 columns -- two bands of 64 rows, the second partial, and two
steps of 1024 columns, the second of 6 -- with its value mix, and with one row and one column of equal keys planted so that the
index alone decides a minimum, inside a wave, across the waves and across the bands.  Everything is compared exactly."""

import os

import numpy as np
import pytest

import all_sim_filter_rule as rule
import auc1_rule as ar
import cluster_rule
import golden_util as gu

pytestmark = pytest.mark.gpu
G6PD = os.path.join(gu.GOLD, 'ref_fixtures', 'G6PD-dct.npz')
N_ROWS, N_COLS, CAP, BOUND = 70, 1030, 17000, 8500
N_NODES = 1200
TIE_ROW, TIE_ROW_2, TIE_COL, TIE_KEY = 5, 66, 700, 77
# (row0, col0): the diagonal through the middle of the tile, the tile wholly left of it (nothing counts), wholly right of it
PLACES = {'diagonal_inside': (500, 10), 'left_of_diagonal': (1100, 0), 'right_of_diagonal': (3, 100)}
NONE = np.uint64(ar.NONE)


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
    column of a wider tensor with an odd row stride.  Rows TIE_ROW (first band) and TIE_ROW_2 (second band) and column TIE_COL
    hold one key throughout and are not flagged."""
    import torch
    rng = np.random.default_rng(23)
    t = _values(rng, N_ROWS, N_COLS)
    t[TIE_ROW] = t[TIE_ROW_2] = TIE_KEY
    t[:, TIE_COL] = TIE_KEY
    flags = (rng.random(N_ROWS) < 0.2, rng.random(N_COLS) < 0.2)
    flags[0][[TIE_ROW, TIE_ROW_2]] = False
    flags[1][TIE_COL] = False
    dev = torch.as_tensor(t, device='cuda')
    wide = torch.full((N_ROWS, N_COLS + 50), 1, dtype=torch.int32, device='cuda')        # (1 would count if it were read)
    odd = torch.full((N_ROWS, N_COLS + 11), 1, dtype=torch.int32, device='cuda')
    views = {'contiguous': dev, 'wide_ld': wide[:, :N_COLS], 'odd_column': odd[:, 3:3 + N_COLS]}
    for v in views.values():
        v.copy_(dev)
    assert views['wide_ld'].stride(0) > N_COLS and views['odd_column'].stride(0) % 2 == 1 and views['odd_column'].data_ptr() % 16 == 12
    return t, flags, views


FAMILIES = {'one': lambda rng: np.zeros(N_NODES, dtype=np.int32), 'all_different': lambda rng: np.arange(N_NODES, dtype=np.int32),
            'five': lambda rng: rng.integers(0, 5, size=N_NODES).astype(np.int32),
            'many': lambda rng: rng.integers(0, 300, size=N_NODES).astype(np.int32)}


def _fresh_first():
    import torch
    from dctdomain_amd.similarity import BEST_NONE
    return torch.full((N_NODES,), BEST_NONE, dtype=torch.int64, device='cuda')


def _words(first) -> np.ndarray:
    return first.cpu().numpy().view(np.uint64)


def _first_fp(view, row0, col0, fam, flags=(None, None), bound=BOUND, first=None):
    import torch
    from dctdomain_amd.similarity import tri_first_fp
    first = first if first is not None else _fresh_first()
    tri_first_fp(view, row0, col0, bound, torch.as_tensor(fam, device='cuda'), first, *flags, cap=CAP)
    return _words(first)


def _tp_before(view, row0, col0, fam, first, flags=(None, None), bound=BOUND, tp=None):
    """``first``: uint64 numpy words."""
    import torch
    from dctdomain_amd.similarity import tri_tp_before
    tp = tp if tp is not None else torch.zeros(N_NODES, dtype=torch.int32, device='cuda')
    tri_tp_before(view, row0, col0, bound, torch.as_tensor(fam, device='cuda'), torch.as_tensor(first.view(np.int64), device='cuda'), tp,
                  *flags, cap=CAP)
    return tp.cpu().numpy().view(np.uint32)


# ---- 1. the two kernels against numpy on hand-made tiles

@pytest.mark.parametrize('pattern', sorted(FAMILIES))
@pytest.mark.parametrize('place', sorted(PLACES))
def test_tri_first_fp_of_one_tile(tile, place, pattern):
    from dctdomain_amd.similarity import BEST_NONE
    assert np.array([BEST_NONE], dtype=np.int64).view(np.uint64)[0] == NONE
    t, flags, views = tile
    row0, col0 = PLACES[place]
    fam = FAMILIES[pattern](np.random.default_rng(5))
    for use in ((None, None), flags):
        want = ar.tile_first_fp(t, row0, col0, BOUND, fam, *use, cap=CAP)
        # one family: pass 1 leaves first untouched; and so does a tile left of the diagonal
        assert (want != NONE).any() == (place != 'left_of_diagonal' and pattern != 'one')
        for name, view in views.items():
            assert np.array_equal(_first_fp(view, row0, col0, fam, use), want), (name, use[0] is not None)
    if place != 'left_of_diagonal' and pattern in ('five', 'many'):
        want = ar.tile_first_fp(t, row0, col0, BOUND, fam, cap=CAP)
        i, j = row0 + np.arange(N_ROWS), col0 + np.arange(N_COLS)
        apart = place == 'right_of_diagonal'                      # (rows and columns name different proteins there)
        for r in (TIE_ROW, TIE_ROW_2):
            # a row of equal keys: the lowest column of another family right of the diagonal wins, whichever wave or step holds it
            others = j[(j > i[r]) & (fam[j] != fam[i[r]])]
            tied = np.uint64(TIE_KEY << 32 | int(others.min()))
            assert len(others) > 256 and want[i[r]] <= tied and (want[i[r]] == tied or not apart)
        # a column of equal keys: the lowest row of another family above the diagonal wins, across the two bands
        c = TIE_COL
        others = i[(i < j[c]) & (fam[i] != fam[j[c]])]
        assert len(others) > 40 and others.max() >= i[64] and want[j[c]] == np.uint64(TIE_KEY << 32 | int(others.min()))
        # the last column of a tied row alone of another family: a minimum from the last wave's part, in the second step
        lone = np.zeros(N_NODES, dtype=np.int32)
        lone[j[N_COLS - 1]] = 1
        assert _first_fp(views['contiguous'], row0, col0, lone)[i[TIE_ROW]] == np.uint64(TIE_KEY << 32 | int(j[N_COLS - 1]))
        assert np.array_equal(_first_fp(views['contiguous'], row0, col0, lone), ar.tile_first_fp(t, row0, col0, BOUND, lone, cap=CAP))
    if place == 'diagonal_inside' and pattern == 'five':
        plain, flagged = ar.tile_first_fp(t, row0, col0, BOUND, fam, cap=CAP), ar.tile_first_fp(t, row0, col0, BOUND, fam, *flags, cap=CAP)
        assert (plain != flagged).any() and (plain[row0 + 64:row0 + N_ROWS] != NONE).any() and (plain[col0 + 1024:col0 + N_COLS] != NONE).any()
        for bound in (BOUND - 1, BOUND + 1, -1, 0, CAP):
            want = ar.tile_first_fp(t, row0, col0, bound, fam, *flags, cap=CAP)
            assert np.array_equal(_first_fp(views['odd_column'], row0, col0, fam, flags, bound), want), bound
        assert (_first_fp(views['contiguous'], row0, col0, fam, flags, -1) == NONE).all()
        # the cap as the bound: everything right of the diagonal is a hit, the flagged rows with key cap
        full = _first_fp(views['contiguous'], row0, col0, fam, flags, CAP)
        assert (full[row0:row0 + N_ROWS] != NONE).all() and (full >> np.uint64(32))[row0:row0 + N_ROWS].max() <= CAP


def _random_first(rng, fam):
    """Words of every kind: none, key 0, the planted key with a low and a high index, ordinary ones."""
    key = rng.integers(0, CAP + 1, size=N_NODES).astype(np.uint64)
    kind = rng.random(N_NODES)
    key[kind < 0.2] = TIE_KEY
    key[(kind >= 0.2) & (kind < 0.3)] = 0
    first = key << np.uint64(32) | rng.integers(0, N_NODES, size=N_NODES).astype(np.uint64)
    first[(kind >= 0.3) & (kind < 0.5)] = NONE
    return first


@pytest.mark.parametrize('pattern', sorted(FAMILIES))
@pytest.mark.parametrize('place', sorted(PLACES))
def test_tri_tp_before_of_one_tile(tile, place, pattern):
    t, flags, views = tile
    row0, col0 = PLACES[place]
    rng = np.random.default_rng(5)
    fam = FAMILIES[pattern](rng)
    arbitrary = _random_first(rng, fam)
    for use in ((None, None), flags):
        for first in (ar.tile_first_fp(t, row0, col0, BOUND, fam, *use, cap=CAP), arbitrary):
            want, split = ar.tile_tp_before(t, row0, col0, BOUND, fam, first, *use, cap=CAP)
            # all different: pass 2 adds nothing; and so does a tile left of the diagonal
            if pattern == 'all_different' or place == 'left_of_diagonal':
                assert not want.any()
            for name, view in views.items():
                assert np.array_equal(_tp_before(view, row0, col0, fam, first, use), want), (name, use[0] is not None)
    if place == 'diagonal_inside' and pattern == 'five':
        # entries that count for one of their ends only: with the tile's own first, and with the arbitrary one
        first = ar.tile_first_fp(t, row0, col0, BOUND, fam, *flags, cap=CAP)
        want, split = ar.tile_tp_before(t, row0, col0, BOUND, fam, first, *flags, cap=CAP)
        much, far = ar.tile_tp_before(t, row0, col0, BOUND, fam, arbitrary, *flags, cap=CAP)
        assert split > 50 and far > 500
        assert want[row0 + 64:row0 + N_ROWS].any() and want[col0 + 1024:col0 + N_COLS].any() and want.max() > 2
        assert much[row0 + 64:row0 + N_ROWS].any() and much[col0 + 1024:col0 + N_COLS].any() and much.max() > 64
        # the bound itself counts and its successor does not: entries of both values are there, so a bound one lower or one higher
        # gives other counts
        at = {b: ar.tile_tp_before(t, row0, col0, b, fam, arbitrary, *flags, cap=CAP)[0] for b in (BOUND - 1, BOUND, BOUND + 1)}
        assert not np.array_equal(at[BOUND - 1], at[BOUND]) and not np.array_equal(at[BOUND + 1], at[BOUND])
        for bound in (BOUND - 1, BOUND + 1, -1, 0, CAP):
            for words in (ar.tile_first_fp(t, row0, col0, bound, fam, *flags, cap=CAP), arbitrary):
                want = ar.tile_tp_before(t, row0, col0, bound, fam, words, *flags, cap=CAP)[0]
                assert np.array_equal(_tp_before(views['odd_column'], row0, col0, fam, words, flags, bound), want), bound
        assert not _tp_before(views['contiguous'], row0, col0, fam, arbitrary, flags, -1).any()
    if place == 'right_of_diagonal' and pattern == 'one':
        # one family and no false positive: every counted entry counts at both ends -- tri_degree's degrees
        from density_rule import tile_degrees
        none = np.full(N_NODES, NONE, dtype=np.uint64)
        assert np.array_equal(_tp_before(views['wide_ld'], row0, col0, fam, none, flags), tile_degrees(t, row0, col0, BOUND, *flags, cap=CAP, n_nodes=N_NODES))


def test_sub_tiles_in_any_order_give_what_one_call_gives(tile):
    import torch
    from dctdomain_amd.similarity import tri_first_fp, tri_tp_before
    t, flags, views = tile
    row0, col0 = PLACES['diagonal_inside']
    fam = FAMILIES['five'](np.random.default_rng(7))
    fam_dev = torch.as_tensor(fam, device='cuda')
    want_first = ar.tile_first_fp(t, row0, col0, BOUND, fam, *flags, cap=CAP)
    want_tp = ar.tile_tp_before(t, row0, col0, BOUND, fam, want_first, *flags, cap=CAP)[0]
    parts = [(r0, r1, c0, c1) for r0, r1 in ((0, 37), (37, N_ROWS)) for c0, c1 in ((0, 513), (513, N_COLS))]
    for order in ((0, 1, 2, 3), (3, 1, 0, 2), (2, 3, 1, 0)):
        first = _fresh_first()
        tp = torch.zeros(N_NODES, dtype=torch.int32, device='cuda')
        for k in order:
            r0, r1, c0, c1 = parts[k]
            tri_first_fp(views['odd_column'][r0:r1, c0:c1], row0 + r0, col0 + c0, BOUND, fam_dev, first, flags[0][r0:r1], flags[1][c0:c1], cap=CAP)
        for k in order:
            r0, r1, c0, c1 = parts[k]
            tri_tp_before(views['odd_column'][r0:r1, c0:c1], row0 + r0, col0 + c0, BOUND, fam_dev, first, tp, flags[0][r0:r1], flags[1][c0:c1],
                          cap=CAP)
        assert np.array_equal(_words(first), want_first), order
        assert np.array_equal(tp.cpu().numpy().view(np.uint32), want_tp), order
    # a second pass 1 over the same tile changes nothing (a minimum); a second pass 2 counts the same again (the caller zeroes tp)
    assert np.array_equal(_first_fp(views['wide_ld'], row0, col0, fam, flags, first=first), want_first)
    assert np.array_equal(_tp_before(views['contiguous'], row0, col0, fam, want_first, flags, tp=tp), 2 * want_tp)


def test_the_exports_refuse_what_they_cannot_bound(tile):
    import torch
    from dctdomain_amd import _lib, similarity
    t, _, views = tile
    view = views['contiguous']
    dev = view.device
    fam = torch.zeros(N_NODES, dtype=torch.int32, device='cuda')
    fam[::2] = 1                                                   # (two families: a launch would write)
    first = _fresh_first()
    tp = torch.zeros(N_NODES, dtype=torch.int32, device='cuda')
    lead = (view.data_ptr(), N_ROWS, N_COLS, N_COLS, 0, 100, None, None, CAP, BOUND)

    def refused(name, *args):
        with pytest.raises(_lib.DctfpError) as err:
            similarity._launch(dev, name, *args)
        assert err.value.code == _lib.DCTFP_ERR_INVALID and err.value.msg.startswith(name + ': ')
        return err.value.msg

    for name, arrays in (('dctfp_tri_first_fp', (fam.data_ptr(), first.data_ptr())),
                         ('dctfp_tri_tp_before', (fam.data_ptr(), first.data_ptr(), tp.data_ptr()))):
        assert 'outside' in refused(name, *lead, *arrays, 100 + N_COLS - 1)                  # the last column is no node
        assert 'outside' in refused(name, *lead[:4], N_NODES - N_ROWS + 1, 0, *lead[6:], *arrays, N_NODES)
        assert 'n_nodes' in refused(name, *lead, *arrays, -1)
        assert 'n_nodes' in refused(name, *lead, *arrays, 1 << 31)
        assert 'aligned' in refused(name, *lead, *arrays[:-1], arrays[-1] + 2, N_NODES)
        assert 'aligned' in refused(name, *lead, arrays[0] + 2, *arrays[1:], N_NODES)
        assert 'aligned' in refused(name, *lead[:-2], CAP, BOUND, arrays[0], arrays[1] + 4, *arrays[2:], N_NODES)     # first: 8 bytes
        assert 'aligned' in refused(name, lead[0] + 2, *lead[1:], *arrays, N_NODES)
        assert 'NULL' in refused(name, None, *lead[1:], *arrays, N_NODES)
        for k in range(len(arrays)):
            assert 'NULL' in refused(name, *lead, *arrays[:k], None, *arrays[k + 1:], N_NODES)
        assert 'shape' in refused(name, *lead[:3], N_COLS - 1, *lead[4:], *arrays, N_NODES)
        assert 'shape' in refused(name, *lead[:1], -1, *lead[2:], *arrays, N_NODES)
        assert 'bound' in refused(name, *lead[:9], CAP + 1, *arrays, N_NODES)
    # a cap whose packed minima would not fit a word: pass 1 refuses it
    big = 4194303
    assert 'cap above 4194302' in refused('dctfp_tri_first_fp', *lead[:8], big, BOUND, fam.data_ptr(), first.data_ptr(), N_NODES)
    with pytest.raises(_lib.DctfpError):
        similarity.tri_first_fp(view, 0, 100, BOUND, fam, first, cap=big)
    similarity._launch(dev, 'dctfp_tri_first_fp', *lead[:8], big - 1, -1, fam.data_ptr(), first.data_ptr(), N_NODES)     # (4194302 is taken; bound -1: no hit)
    # the wrappers' own checks, and the empty tile: nothing launched
    with pytest.raises(IndexError):
        similarity.tri_first_fp(view, N_NODES - N_ROWS + 1, 0, BOUND, fam, first)
    with pytest.raises(IndexError):
        similarity.tri_tp_before(view, 0, N_NODES - N_COLS + 1, BOUND, fam, first, tp)
    with pytest.raises(ValueError):
        similarity.tri_first_fp(view, 0, 100, BOUND, fam.to(torch.int64), first)
    with pytest.raises(ValueError):
        similarity.tri_first_fp(view, 0, 100, BOUND, fam, first.to(torch.int32))
    with pytest.raises(ValueError):
        similarity.tri_first_fp(view, 0, 100, BOUND, fam, first.cpu())
    with pytest.raises(ValueError):
        similarity.tri_tp_before(view, 0, 100, BOUND, fam, first[:-1], tp)
    with pytest.raises(ValueError):
        similarity.tri_tp_before(view, 0, 100, BOUND, fam, first, tp.to(torch.int64))
    for empty in (view[:0], view[:, :0]):
        similarity.tri_first_fp(empty, 0, 100, BOUND, fam, first)
        similarity.tri_tp_before(empty, 0, 100, BOUND, fam, first, tp)
    # nothing was written by any of these
    assert (first == similarity.BEST_NONE).all().item() and not tp.any().item()


# ---- 2. Auc1

@pytest.fixture(scope='module')
def g6pd():
    with np.load(G6PD) as data:
        sid, idx, dct = [str(s) for s in data['sid']], data['idx'], data['dct']
    tri = rule.triangle_l1(dct, idx)
    fam = cluster_rule.labels(dct, idx, min_global=0.6)[0]
    return {'sid': sid, 'idx': idx, 'dct': dct, 'tri': tri, 'fam': fam, 'names': [f'fam{f}' for f in fam]}


def _same(job, want, fam):
    got = job.counts()
    for g, w in zip(got, want):
        assert g.dtype == np.int32 and np.array_equal(g, w)
    assert job.auc1().dtype == np.float64 and np.allclose(job.auc1(), ar.auc1(want[0], fam), atol=1e-15)
    s, w = job.summary(), ar.summary(want[0], fam)
    assert s['queries'] == w['queries'] and s['families'] == w['families']
    assert all(abs(s[k] - w[k]) < 1e-12 for k in ('mean_auc1', 'top1_raw', 'top1_norm'))


CASES = {'domain': ('domain', None), 'domain0.8': ('domain', 0.8), 'global': ('global', None), 'global0.6': ('global', 0.6),
         'domain1.0': ('domain', 1.0), 'global0.0': ('global', 0.0)}


@pytest.mark.parametrize('case', sorted(CASES))
def test_auc1_of_the_reference_fixture(g6pd, case, monkeypatch):
    from dctdomain_amd import dct_sim
    score, cut = CASES[case]
    sid, idx, dct, fam = g6pd['sid'], g6pd['idx'], g6pd['dct'], g6pd['fam']
    want = ar.of_file(dct, idx, fam, score, min_cut=cut, triangle=g6pd['tri'])
    if case == 'domain':
        assert '%.4f' % ar.summary(want[0], fam)['mean_auc1'] == '0.7596'
    fills = []
    for name in ('protein_min', 'l1_matrix'):
        monkeypatch.setattr(dct_sim, name, lambda *a, _fn=getattr(dct_sim, name), **k: (fills.append(1), _fn(*a, **k))[1])
    job = dct_sim.Auc1(sid, idx, dct, g6pd['names'], score=score, min_cut=cut)
    assert len(list(job.stripes())) == 1
    _same(job, want, fam)
    assert len(fills) == 1                                        # one stripe: the tile of the first pass serves the second
    # several stripes and column groups: the tiles are filled again, the result is the same
    for tile_ints, col_rows in ((90, 7), (5, 3)):
        small = dct_sim.Auc1(sid, idx, dct, g6pd['names'], score=score, min_cut=cut)
        small.TILE_INTS, small.COL_ROWS = tile_ints, col_rows
        stripes = len(list(small.stripes()))
        assert stripes >= 3 and int(idx[-1]) > 2 * col_rows
        del fills[:]
        _same(small, want, fam)
        assert len(fills) >= 2 * (stripes + 1)                    # two passes over every stripe, the first in two column groups or more


@pytest.fixture(scope='module')
def planted():
    """300 proteins of 1 .. 3 fingerprints (two of them without any) in 24 planted families and 6 families of one: a family's
    rows are its centre plus noise whose width differs from protein to protein, so some queries rank strangers first."""
    rng = np.random.default_rng(31)
    n, d = 300, 480
    counts = rng.integers(1, 4, size=n)
    counts[[41, 299]] = 0
    fam = rng.integers(0, 24, size=n)
    fam[[7, 100, 101, 150, 222, 298]] = 100 + np.arange(6)
    centres = rng.integers(-40, 41, size=(130, d))
    width = rng.choice([4, 12, 30, 60], size=n)
    rows = []
    for p in np.flatnonzero(counts):
        r = centres[fam[p]][None, :] + np.rint(rng.normal(0, width[p], size=(counts[p], d)))
        rows.append(np.clip(r, -127, 127))
    dct = np.concatenate(rows).astype(np.int8)
    idx = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return {'sid': [f'prot{p}' for p in range(n)], 'idx': idx, 'dct': dct, 'n': n, 'fam': fam, 'tri': rule.triangle_l1(dct, idx)}


@pytest.mark.parametrize('score', ['domain', 'global'])
def test_a_planted_file_with_empty_proteins_and_families_of_one(planted, score):
    from dctdomain_amd import dct_sim
    sid, idx, dct, fam = planted['sid'], planted['idx'], planted['dct'], planted['fam']
    for cut in (None, 0.25):
        want = ar.of_file(dct, idx, fam, score, min_cut=cut, triangle=planted['tri'])
        if cut is None:
            tp, fp_index, fp_key = want
            s = ar.summary(tp, fam)
            assert s['queries'] == 294 and 0.2 < s['mean_auc1'] < 0.95 and 0.5 < s['top1_raw'] < 1
            assert tp[41] == 0 and tp[299] == 0 and fp_index[41] == -1 and fp_index[299] == -1 and (fp_index >= 0).sum() > 200
        _same(dct_sim.Auc1(sid, idx, dct, fam.tolist(), score=score, min_cut=cut), want, fam)
    small = dct_sim.Auc1(sid, idx, dct, fam.tolist(), score=score)
    small.TILE_INTS, small.COL_ROWS = 4000, 100
    assert len(list(small.stripes())) > 5
    _same(small, ar.of_file(dct, idx, fam, score, triangle=planted['tri']), fam)


@pytest.mark.parametrize('score', ['domain', 'global'])
def test_against_the_search_path(g6pd, score):
    """Every protein searched in its own file with top = n: the ranked hits dct-sim --db prints.  Skip the self hit, walk to the
    first hit of another family -- the reference's read_results on this project's own ranking."""
    from dctdomain_amd import dct_sim
    sid, idx, dct, fam = g6pd['sid'], g6pd['idx'], g6pd['dct'], g6pd['fam']
    n = len(sid)
    hits = dct_sim.ProteinSearch(dct, idx).search(dct, idx, top=n, threshold=0.0, rank=score)
    tp, fp_index, fp_key = np.zeros(n, dtype=np.int32), np.full(n, -1, dtype=np.int32), np.full(n, 17000, dtype=np.int32)
    for x, (found, mn, last) in enumerate(hits):
        assert len(found) == n
        for y, l1 in zip(found.tolist(), (mn if score == 'domain' else last).tolist()):
            if y == x:
                continue
            if min(l1, 17000) > ar.BOUND_ALL:
                break
            if fam[y] != fam[x]:
                fp_index[x], fp_key[x] = y, l1
                break
            tp[x] += 1
    got = dct_sim.Auc1(sid, idx, dct, fam.tolist(), score=score).counts()
    assert np.array_equal(got[0], tp) and np.array_equal(got[1], fp_index) and np.array_equal(got[2], fp_key)


# ---- 3. the command line

def _main(tmp_path, *argv, dct=G6PD) -> bytes:
    from dctdomain_amd import dct_sim
    out = str(tmp_path / 'out.txt')
    dct_sim.main(['--dct', dct, '--output', out] + list(argv))
    with open(out, 'rb') as fh:
        return fh.read()


def test_cli_prints_the_auc1_of_a_file(tmp_path, g6pd, capsys):
    from dctdomain_amd import dct_sim
    sid, idx, dct, fam, names = g6pd['sid'], g6pd['idx'], g6pd['dct'], g6pd['fam'], g6pd['names']
    fam_file = tmp_path / 'families.txt'
    fam_file.write_text('# id family\n\n' + ''.join(f'{s}\t{f}\n' for s, f in zip(reversed(sid), reversed(names))) + 'stranger fam9\n')
    texts = {}
    for score, cut in (('domain', None), ('global', None), ('domain', 0.8), ('global', 0.6)):
        want = ar.HEADER + ar.text(sid, names, *ar.of_file(dct, idx, fam, score, min_cut=cut, triangle=g6pd['tri']))
        argv = ['--auc1', score, '--families', str(fam_file)] + ([f'--min-{score}', str(cut)] if cut is not None else [])
        texts[score, cut] = _main(tmp_path, *argv)
        assert texts[score, cut] == want, (score, cut)
    assert len(set(texts.values())) == 4
    assert texts['domain', None].splitlines()[-1] == b'# queries=26 families=3 mean_auc1=0.7596 top1_raw=0.9615 top1_norm=0.9744'
    assert texts['global', None].splitlines()[-1] == b'# queries=26 families=3 mean_auc1=1.0000 top1_raw=1.0000 top1_norm=1.0000'
    assert _main(tmp_path, '--auc1', '--families', str(fam_file)) == texts['domain', None]
    # the family in the id: the reference's CATH20 convention
    tagged = str(tmp_path / 'tagged-dct.npz')
    np.savez(tagged, sid=np.array([f'{s}|{f}' for s, f in zip(sid, names)]), idx=idx, dct=dct)
    want = ar.HEADER + ar.text([f'{s}|{f}' for s, f in zip(sid, names)], names, *ar.of_file(dct, idx, fam, 'domain', triangle=g6pd['tri']))
    assert _main(tmp_path, '--auc1', '--family-sep', '|', dct=tagged) == want
    # without --output the same text goes to stdout
    capsys.readouterr()
    dct_sim.main(['--dct', G6PD, '--auc1', 'global', '--families', str(fam_file)])
    printed = [line for line in capsys.readouterr().out.splitlines() if not line.startswith(('dct loaded', 'total time', 'distance calculation'))]
    assert ('\n'.join(printed) + '\n').encode() == texts['global', None]
    # a protein without a family is an error that names it
    fam_file.write_text(''.join(f'{s} {f}\n' for s, f in zip(sid[1:], names[1:])))
    with pytest.raises(ValueError, match=f'gives no family for {sid[0]}'):
        _main(tmp_path, '--auc1', '--families', str(fam_file))
