"""dct-sim --hist on the GPU (similarity.tri_hist = dctfp_tri_hist; Histogram; the command line) against the numpy rule of
hist_rule.py (worked by hand and pinned on the reference fixture in test_hist_host.py).

The tile of part 1 is that of tests/test_auc1_gpu.py: 70 rows x 1030 columns with its value mix -- for the kernel's job of 64 rows x
1024 columns two bands, the second partial, and two steps, the second of 6: a partial last job in both directions.  Everything is
compared exactly."""

import os

import numpy as np
import pytest

import all_sim_filter_rule as rule
import cluster_rule
import golden_util as gu
import hist_rule as hr

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
    column of a wider tensor with an odd row stride; 20 % of the rows and of the columns are flagged."""
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


FAMILIES = {'none': lambda rng: None, 'one': lambda rng: np.zeros(N_NODES, dtype=np.int32),
            'all_different': lambda rng: np.arange(N_NODES, dtype=np.int32),
            'five': lambda rng: rng.integers(0, 5, size=N_NODES).astype(np.int32),
            'many': lambda rng: rng.integers(0, 300, size=N_NODES).astype(np.int32)}


def _fresh(fam, cap=CAP):
    import torch
    return torch.zeros((1 if fam is None else 2, cap + 1), dtype=torch.int64, device='cuda')


def _hist(view, row0, col0, fam, flags=(None, None), bound=BOUND, hist=None, cap=CAP):
    import torch
    from dctdomain_amd.similarity import tri_hist
    hist = hist if hist is not None else _fresh(fam, cap)
    tri_hist(view, row0, col0, bound, hist, None if fam is None else torch.as_tensor(fam, device='cuda'), *flags, cap=cap)
    return hist.cpu().numpy().view(np.uint64)


# ---- 1. the kernel against numpy on hand-made tiles

@pytest.mark.parametrize('pattern', sorted(FAMILIES))
@pytest.mark.parametrize('place', sorted(PLACES))
def test_tri_hist_of_one_tile(tile, place, pattern):
    t, flags, views = tile
    row0, col0 = PLACES[place]
    fam = FAMILIES[pattern](np.random.default_rng(5))
    for use in ((None, None), flags):
        want = hr.tile_hist(t, row0, col0, BOUND, fam, *use, cap=CAP)
        assert want.any() == (place != 'left_of_diagonal')
        if place != 'left_of_diagonal':
            # the classes that can be hit are: row 1 stays empty with one family, row 0 with all different
            assert want[0].any() == (pattern != 'all_different') and (pattern in ('none', 'one') or want[1].any())
            assert want[:, BOUND].any() and not want[:, BOUND + 1:].any() and want[:, 0].any()
        for name, view in views.items():
            assert np.array_equal(_hist(view, row0, col0, fam, use), want), (name, use[0] is not None)
    if place == 'diagonal_inside' and pattern in ('none', 'five'):
        plain, flagged = hr.tile_hist(t, row0, col0, BOUND, fam, cap=CAP), hr.tile_hist(t, row0, col0, BOUND, fam, *flags, cap=CAP)
        assert (plain != flagged).any()
        # the second band and the second step hold counted entries: the partial last job in both directions
        assert hr.tile_hist(t[64:], row0 + 64, col0, BOUND, fam, cap=CAP).any() and hr.tile_hist(t[:, 1024:], row0, col0 + 1024, BOUND, fam, cap=CAP).any()
        at = {b: hr.tile_hist(t, row0, col0, b, fam, *flags, cap=CAP).sum() for b in (BOUND - 1, BOUND, BOUND + 1)}
        assert at[BOUND - 1] < at[BOUND] < at[BOUND + 1]            # (the bound itself counts and its successor does not)
        for bound in (-1, 0, BOUND - 1, BOUND + 1, CAP):
            want = hr.tile_hist(t, row0, col0, bound, fam, *flags, cap=CAP)
            assert np.array_equal(_hist(views['odd_column'], row0, col0, fam, flags, bound), want), bound
        assert not _hist(views['contiguous'], row0, col0, fam, flags, -1).any()
        # the cap as the bound: every entry right of the diagonal counts, the flagged ones in the last bin
        full = _hist(views['contiguous'], row0, col0, fam, flags, CAP)
        i, j = row0 + np.arange(N_ROWS)[:, None], col0 + np.arange(N_COLS)[None, :]
        assert full.sum() == (j > i).sum() and full[:, CAP].sum() > flags[0].sum() * 100


@pytest.mark.parametrize('pattern', ['none', 'one', 'five'])
def test_a_tile_of_one_key_lands_in_one_bin(pattern):
    """The hot bin: every lane of every wave adds to the same counter, in every row."""
    import torch
    fam = FAMILIES[pattern](np.random.default_rng(5))
    t = np.full((N_ROWS, N_COLS), 4242, dtype=np.int32)
    view = torch.as_tensor(t, device='cuda')
    for row0, col0 in PLACES.values():
        want = hr.tile_hist(t, row0, col0, BOUND, fam, cap=CAP)
        got = _hist(view, row0, col0, fam)
        assert np.array_equal(got, want) and not np.delete(got, 4242, axis=1).any()
    right = _hist(view, *PLACES['right_of_diagonal'], fam)
    assert right[:, 4242].sum() == N_ROWS * N_COLS and (pattern == 'five' or right[0, 4242] == N_ROWS * N_COLS)
    # two keys in stripes of 3 columns: the lanes that do not share the first lane's key add on their own
    t[:, ::3] = 77
    view = torch.as_tensor(t, device='cuda')
    assert np.array_equal(_hist(view, *PLACES['diagonal_inside'], fam), hr.tile_hist(t, *PLACES['diagonal_inside'], BOUND, fam, cap=CAP))


def test_sub_tiles_in_any_order_and_a_second_call(tile):
    import torch
    from dctdomain_amd.similarity import tri_hist
    t, flags, views = tile
    row0, col0 = PLACES['diagonal_inside']
    fam = FAMILIES['five'](np.random.default_rng(7))
    fam_dev = torch.as_tensor(fam, device='cuda')
    want = hr.tile_hist(t, row0, col0, BOUND, fam, *flags, cap=CAP)
    parts = [(r0, r1, c0, c1) for r0, r1 in ((0, 37), (37, N_ROWS)) for c0, c1 in ((0, 513), (513, N_COLS))]
    for order in ((0, 1, 2, 3), (3, 1, 0, 2), (2, 3, 1, 0)):
        hist = _fresh(fam)
        for k in order:
            r0, r1, c0, c1 = parts[k]
            tri_hist(views['odd_column'][r0:r1, c0:c1], row0 + r0, col0 + c0, BOUND, hist, fam_dev, flags[0][r0:r1], flags[1][c0:c1], cap=CAP)
        assert np.array_equal(hist.cpu().numpy().view(np.uint64), want), order
    # a second call over the same tile counts the same again (the caller zeroes hist)
    assert np.array_equal(_hist(views['wide_ld'], row0, col0, fam, flags, hist=hist), 2 * want)
    # and one class is the sum of the two
    assert np.array_equal(_hist(views['contiguous'], row0, col0, None, flags)[0], want.sum(axis=0))


def test_many_workgroups_flush_into_the_same_bins():
    """300 x 5000: 5 bands x 5 steps, 25 workgroups whose keys crowd into 500 values, with the diagonal through it."""
    import torch
    rng = np.random.default_rng(41)
    t = rng.integers(3000, 3500, size=(300, 5000)).astype(np.int32)
    t[rng.random(t.shape) < 0.1] = 0x7fffffff
    fam = rng.integers(0, 40, size=6000).astype(np.int32)
    view = torch.as_tensor(t, device='cuda')
    for fams in (None, fam):
        for row0, col0 in ((0, 1), (700, 0)):
            want = hr.tile_hist(t, row0, col0, CAP - 1, fams, cap=CAP)
            assert want.sum() > 1_000_000 and want.max() > 2000
            hist = torch.zeros((1 if fams is None else 2, CAP + 1), dtype=torch.int64, device='cuda')
            from dctdomain_amd.similarity import tri_hist
            tri_hist(view, row0, col0, CAP - 1, hist, None if fams is None else torch.as_tensor(fams, device='cuda'))
            assert np.array_equal(hist.cpu().numpy().view(np.uint64), want)


def test_the_export_refuses_what_it_cannot_bound(tile):
    import torch
    from dctdomain_amd import _lib, similarity
    t, _, views = tile
    view = views['contiguous']
    dev = view.device
    fam = torch.zeros(N_NODES, dtype=torch.int32, device='cuda')
    fam[::2] = 1
    hist = _fresh(fam)
    one = _fresh(None)
    lead = (view.data_ptr(), N_ROWS, N_COLS, N_COLS, 0, 100, None, None, CAP, BOUND)
    name = 'dctfp_tri_hist'

    def refused(*args):
        with pytest.raises(_lib.DctfpError) as err:
            similarity._launch(dev, name, *args)
        assert err.value.code == _lib.DCTFP_ERR_INVALID and err.value.msg.startswith(name + ': ')
        return err.value.msg

    arrays = (fam.data_ptr(), N_NODES, hist.data_ptr())
    assert 'outside' in refused(*lead, fam.data_ptr(), 100 + N_COLS - 1, hist.data_ptr())          # the last column is no node
    assert 'outside' in refused(*lead[:4], N_NODES - N_ROWS + 1, 0, *lead[6:], *arrays)
    assert 'outside' in refused(*lead, None, 100 + N_COLS - 1, one.data_ptr())                      # ... with or without fam
    assert 'n_nodes' in refused(*lead, fam.data_ptr(), -1, hist.data_ptr())
    assert 'n_nodes' in refused(*lead, fam.data_ptr(), 1 << 31, hist.data_ptr())
    assert 'aligned' in refused(*lead, fam.data_ptr(), N_NODES, hist.data_ptr() + 4)                # hist: 8 bytes
    assert 'aligned' in refused(*lead, fam.data_ptr() + 2, N_NODES, hist.data_ptr())
    assert 'aligned' in refused(lead[0] + 2, *lead[1:], *arrays)
    assert 'NULL' in refused(None, *lead[1:], *arrays)
    assert 'NULL' in refused(*lead, fam.data_ptr(), N_NODES, None)
    assert 'shape' in refused(*lead[:3], N_COLS - 1, *lead[4:], *arrays)
    assert 'shape' in refused(*lead[:1], -1, *lead[2:], *arrays)
    assert 'bound' in refused(*lead[:9], CAP + 1, *arrays)
    assert 'bound' in refused(*lead[:9], -2, *arrays)
    # a cap whose two class rows would not fit the LDS of a CU is refused with the limit; the limit itself is taken, with both classes
    limit = 20479
    big = torch.zeros((2, limit + 2), dtype=torch.int64, device='cuda')
    assert f'cap above {limit}' in refused(*lead[:8], limit + 1, BOUND, fam.data_ptr(), N_NODES, big.data_ptr())
    with pytest.raises(_lib.DctfpError, match=f'cap above {limit}'):
        similarity.tri_hist(view, 0, 100, BOUND, big, fam, cap=limit + 1)
    assert not big.any().item()
    most = torch.zeros((2, limit + 1), dtype=torch.int64, device='cuda')
    similarity.tri_hist(view, 0, 100, limit, most, fam, cap=limit)
    assert np.array_equal(most.cpu().numpy().view(np.uint64), hr.tile_hist(t, 0, 100, limit, fam.cpu().numpy(), cap=limit))
    assert most[:, limit].sum().item() > 1000 and most.sum().item() == N_ROWS * N_COLS
    # the wrapper's own checks, and the empty tile: nothing launched
    with pytest.raises(IndexError):
        similarity.tri_hist(view, N_NODES - N_ROWS + 1, 0, BOUND, hist, fam)
    with pytest.raises(IndexError):
        similarity.tri_hist(view, 0, N_NODES - N_COLS + 1, BOUND, hist, fam)
    with pytest.raises(ValueError):
        similarity.tri_hist(view, 0, 100, BOUND, hist, fam.to(torch.int64))
    with pytest.raises(ValueError):
        similarity.tri_hist(view, 0, 100, BOUND, hist, fam.cpu())
    with pytest.raises(ValueError):
        similarity.tri_hist(view, 0, 100, BOUND, hist.to(torch.int32), fam)
    with pytest.raises(ValueError):
        similarity.tri_hist(view, 0, 100, BOUND, hist.cpu(), fam)
    with pytest.raises(ValueError):
        similarity.tri_hist(view, 0, 100, BOUND, hist[:, :-1], fam)
    with pytest.raises(ValueError, match='two rows with it'):
        similarity.tri_hist(view, 0, 100, BOUND, one, fam)
    with pytest.raises(ValueError, match='one row without fam'):
        similarity.tri_hist(view, 0, 100, BOUND, hist)
    with pytest.raises(IndexError):
        similarity.tri_hist(view, 0, 100, BOUND, hist, fam[:100 + N_COLS - 1])       # fam too short for the tile
    for empty in (view[:0], view[:, :0]):
        similarity.tri_hist(empty, 0, 100, BOUND, hist, fam)
        similarity.tri_hist(empty, 0, 100, BOUND, one)
    similarity._launch(dev, name, view.data_ptr(), 0, N_COLS, N_COLS, 0, 100, None, None, CAP, BOUND, *arrays)
    # nothing was written by any of these
    assert not hist.any().item() and not one.any().item()


# ---- 2. Histogram

@pytest.fixture(scope='module')
def g6pd():
    with np.load(G6PD) as data:
        sid, idx, dct = [str(s) for s in data['sid']], data['idx'], data['dct']
    tri = rule.triangle_l1(dct, idx)
    fam = cluster_rule.labels(dct, idx, min_global=0.6)[0]
    return {'sid': sid, 'idx': idx, 'dct': dct, 'tri': tri, 'fam': fam, 'names': [f'fam{f}' for f in fam]}


def _same(job, want):
    hist, rest = job.counts()
    assert hist.dtype == np.uint64 and rest.dtype == np.uint64
    assert hist.shape == want[0].shape and np.array_equal(hist, want[0]) and np.array_equal(rest, want[1])


CASES = {'domain': ('domain', None), 'domain0.8': ('domain', 0.8), 'global': ('global', None), 'global0.6': ('global', 0.6),
         'domain1.0': ('domain', 1.0), 'global0.0': ('global', 0.0)}


@pytest.mark.parametrize('case', sorted(CASES))
def test_histogram_of_the_reference_fixture(g6pd, case, monkeypatch):
    from dctdomain_amd import dct_sim
    score, cut = CASES[case]
    sid, idx, dct, fam = g6pd['sid'], g6pd['idx'], g6pd['dct'], g6pd['fam']
    fills = []
    for name in ('protein_min', 'l1_matrix'):
        monkeypatch.setattr(dct_sim, name, lambda *a, _fn=getattr(dct_sim, name), **k: (fills.append(1), _fn(*a, **k))[1])
    for families, labels in ((None, None), (g6pd['names'], fam)):
        want = hr.of_file(dct, idx, labels, score, min_cut=cut, triangle=g6pd['tri'])
        del fills[:]
        job = dct_sim.Histogram(sid, idx, dct, families, score=score, min_cut=cut)
        _same(job, want)
        assert len(fills) == 1                                    # one pass over one stripe
        for bins in (10, 100):
            assert ('\n'.join(job.lines(bins)) + '\n').encode() == hr.text(*want, bins, cut)
        # several stripes and column groups: the same counts
        for tile_ints, col_rows in ((90, 7), (5, 3)):
            small = dct_sim.Histogram(sid, idx, dct, families, score=score, min_cut=cut)
            small.TILE_INTS, small.COL_ROWS = tile_ints, col_rows
            assert len(list(small.stripes())) >= 3
            _same(small, want)
    if cut is None:
        last = {'domain': '# pairs=351 same=114 other=237 roc_auc=0.7467 best_f1=0.7006 at=0.847971',
                'global': '# pairs=351 same=114 other=237 roc_auc=1.0000 best_f1=1.0000 at=' + hr.at_text(8633)}[score]
        assert job.lines(10)[-1] == last and dct_sim.sim_bound(float(job.summary()['at'])) == {'domain': 2584, 'global': 8633}[score]


@pytest.fixture(scope='module')
def planted():
    """300 proteins of 1 .. 3 fingerprints (two of them without any) in 24 planted families and 6 families of one."""
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
def test_a_planted_file_in_several_stripes_is_the_one_stripe_result(planted, score):
    from dctdomain_amd import dct_sim
    sid, idx, dct, fam = planted['sid'], planted['idx'], planted['dct'], planted['fam']
    for cut in (None, 0.25):
        want = hr.of_file(dct, idx, fam, score, min_cut=cut, triangle=planted['tri'])
        if cut is None:
            assert int(want[0].sum()) > 5000 and int(want[1].sum()) >= 299 + 298       # (the two empty proteins' pairs are in the rest)
            s = hr.summary(*want)
            assert s['pairs'] == 300 * 299 // 2 and 0.5 < s['roc_auc'] < 1 and 0.1 < s['best_f1'] < 1
        one = dct_sim.Histogram(sid, idx, dct, fam.tolist(), score=score, min_cut=cut)
        assert len(list(one.stripes())) == 1
        _same(one, want)
        small = dct_sim.Histogram(sid, idx, dct, fam.tolist(), score=score, min_cut=cut)
        small.TILE_INTS, small.COL_ROWS = 4000, 100
        assert len(list(small.stripes())) > 5
        _same(small, want)
        assert small.lines(50) == one.lines(50) and ('\n'.join(one.lines(50)) + '\n').encode() == hr.text(*want, 50, cut)
    _same(dct_sim.Histogram(sid, idx, dct, score=score), hr.of_file(dct, idx, None, score, triangle=planted['tri']))


# ---- 3. the command line

def _main(tmp_path, *argv, dct=G6PD) -> bytes:
    from dctdomain_amd import dct_sim
    out = str(tmp_path / 'out.txt')
    dct_sim.main(['--dct', dct, '--output', out] + list(argv))
    with open(out, 'rb') as fh:
        return fh.read()


def test_cli_prints_the_histogram_of_a_file(tmp_path, g6pd, capsys):
    from dctdomain_amd import dct_sim
    sid, idx, dct, fam, names = g6pd['sid'], g6pd['idx'], g6pd['dct'], g6pd['fam'], g6pd['names']
    fam_file = tmp_path / 'families.txt'
    fam_file.write_text('# id family\n\n' + ''.join(f'{s}\t{f}\n' for s, f in zip(reversed(sid), reversed(names))) + 'stranger fam9\n')
    texts = {}
    for score, cut, labelled, bins in (('domain', None, True, 100), ('global', None, True, 10), ('domain', 0.8, False, 7), ('global', 0.6, True, 1000),
                                       ('domain', None, False, 100)):
        counts = hr.of_file(dct, idx, fam if labelled else None, score, min_cut=cut, triangle=g6pd['tri'])
        want = hr.header(score, labelled) + hr.text(*counts, bins, cut)
        argv = ['--hist', score] + (['--families', str(fam_file)] if labelled else []) + ([f'--min-{score}', str(cut)] if cut is not None else [])
        texts[score, cut, labelled] = _main(tmp_path, *argv, *(['--bins', str(bins)] if bins != 100 else []))
        assert texts[score, cut, labelled] == want, (score, cut, labelled)
    assert len(set(texts.values())) == 5
    assert texts['domain', None, True].splitlines()[-1] == b'# pairs=351 same=114 other=237 roc_auc=0.7467 best_f1=0.7006 at=0.847971'
    assert texts['global', None, True].splitlines()[-1] == b'# pairs=351 same=114 other=237 roc_auc=1.0000 best_f1=1.0000 at=0.492147'
    assert texts['domain', None, False].splitlines()[-1] == b'# pairs=351 scored=351' and len(texts['domain', None, False].splitlines()) == 102
    assert _main(tmp_path, '--hist', '--families', str(fam_file)) == texts['domain', None, True]
    # the family in the id
    tagged = str(tmp_path / 'tagged-dct.npz')
    np.savez(tagged, sid=np.array([f'{s}|{f}' for s, f in zip(sid, names)]), idx=idx, dct=dct)
    assert _main(tmp_path, '--hist', '--family-sep', '|', dct=tagged) == texts['domain', None, True]
    # without --output the same text goes to stdout
    capsys.readouterr()
    dct_sim.main(['--dct', G6PD, '--hist', 'global', '--families', str(fam_file), '--bins', '10'])
    printed = [line for line in capsys.readouterr().out.splitlines() if not line.startswith(('dct loaded', 'total time', 'distance calculation'))]
    assert ('\n'.join(printed) + '\n').encode() == texts['global', None, True]
    # hist_sim with a path, as the other mode functions take one
    out = str(tmp_path / 'direct.txt')
    dct_sim.hist_sim(G6PD, out, score='global', bins=10, families=str(fam_file))
    with open(out, 'rb') as fh:
        assert fh.read() == texts['global', None, True]


def test_kept_is_what_all_sim_prints_at_that_cut_off(tmp_path):
    """For three cut-offs of a --hist table, "kept" = the lines dct-sim --min-domain <that text> prints; and at the best-F1 cut-off
    the printed pairs are the kept ones of the summary."""
    from dctdomain_amd import dct_sim
    table = _main(tmp_path, '--hist', 'domain', '--bins', '10').splitlines()
    assert table[0] == b'#min-domain pairs kept' and len(table) == 12
    rows = {line.split()[0].decode(): int(line.split()[2]) for line in table[1:-1]}
    assert [rows[t] for t in ('0.9000', '0.8000', '0.7000', '0.6000', '0.5000')] == [31, 125, 241, 328, 351]
    for text in ('0.9000', '0.7000', '0.6000'):
        printed = _main(tmp_path, '--min-domain', text).splitlines()
        assert len(printed) - 1 == rows[text], text
