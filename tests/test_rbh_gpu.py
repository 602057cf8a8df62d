"""dct-sim --db --rbh (dct_sim.ReciprocalBest; dctfp_rect_best) against numpy: the scan kernel on raw tiles with ties everywhere,
accumulation over shuffled sub-tiles, the class against the oracle of rbh_rule.py (pinned on the CPU in test_rbh_host.py) on
planted families with duplicates and proteins without fingerprints, and the text -- the reference golden's lines included."""

import os

import numpy as np
import pytest

import rbh_rule as rrule

pytestmark = pytest.mark.gpu
CAP = 17000
NONE = np.uint64(0xffffffffffffffff)
SHAPES = [(1, 1), (1, 1025), (63, 3), (64, 1024), (65, 1025), (130, 2051)]


# ---- 1. rect_best against numpy on raw tiles

def _np_best(t, row0, col0, bound, n_a, n_b, row_empty=None, col_empty=None, cap=CAP):
    """(best_row, best_col) as uint64 after one call on a fresh state: the lexicographic (key, index) minimum of the hits of every
    row and of every column, all ones elsewhere."""
    key = np.minimum(t.astype(np.int64) & 0xffffffff, cap)    # (a negative value counts as cap)
    if row_empty is not None:
        key[np.asarray(row_empty, dtype=bool)] = cap
    if col_empty is not None:
        key[:, np.asarray(col_empty, dtype=bool)] = cap
    best_row, best_col = np.full(n_a, NONE, dtype=np.uint64), np.full(n_b, NONE, dtype=np.uint64)
    r, c = np.nonzero(key <= bound)
    k = key[r, c].astype(np.uint64) << np.uint64(32)
    np.minimum.at(best_row, row0 + r, k | (col0 + c).astype(np.uint64))
    np.minimum.at(best_col, col0 + c, k | (row0 + r).astype(np.uint64))
    return best_row, best_col


def _tile(rng, n_rows, n_cols):
    """Values 0 .. 5 (nearly every row and column has tied minima), about a tenth replaced by values that count as cap."""
    t = rng.integers(0, 6, size=(n_rows, n_cols)).astype(np.int64)
    u = rng.random((n_rows, n_cols))
    for k, v in enumerate((CAP, CAP + 1, 0x7fffffff, -1)):
        t[(u >= 0.025 * k) & (u < 0.025 * (k + 1))] = v
    return t.astype(np.int32)


def _view(t):
    """The tile as the view big[:, 1:1 + n_cols] of a wider device tensor: ld != n_cols, rows off 16-byte boundaries; what lies
    beside it is 0 = the best hit if it were read."""
    import torch
    big = torch.zeros((t.shape[0], t.shape[1] + 6), dtype=torch.int32, device='cuda')
    view = big[:, 1:1 + t.shape[1]]
    view.copy_(torch.as_tensor(t, device='cuda'))
    assert view.data_ptr() - big.data_ptr() == 4 and (t.shape[0] == 1 or view.stride(0) == t.shape[1] + 6)
    return view


def _state_arrays(state):
    return state.best_row.cpu().numpy().view(np.uint64), state.best_col.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize('n_rows,n_cols', SHAPES)
def test_rect_best_against_numpy(n_rows, n_cols):
    from dctdomain_amd.similarity import BEST_NONE, BestState, rect_best
    rng = np.random.default_rng(100 * n_rows + n_cols)
    t = _tile(rng, n_rows, n_cols)
    view = _view(t)
    tied = 0
    for k, (row0, col0) in enumerate([(0, 0), (5, 0), (0, 7), (3, 1030)]):
        n_a, n_b = row0 + n_rows + k, col0 + n_cols + 2 * k
        for flags in ((None, None), (rng.random(n_rows) < 0.2, rng.random(n_cols) < 0.2)):
            for bound in (-1, 2, CAP):
                state = BestState(n_a, n_b)
                rect_best(view, row0, col0, bound, state, *flags)
                want = _np_best(t, row0, col0, bound, n_a, n_b, *flags)
                got = _state_arrays(state)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (row0, col0, bound, flags[0] is not None)
                # outside the tile nothing is written
                outside_a = np.setdiff1d(np.arange(n_a), row0 + np.arange(n_rows))
                outside_b = np.setdiff1d(np.arange(n_b), col0 + np.arange(n_cols))
                assert (state.best_row.cpu().numpy()[outside_a] == BEST_NONE).all() and (state.best_col.cpu().numpy()[outside_b] == BEST_NONE).all()
                if bound == -1:
                    assert (got[0] == NONE).all() and (got[1] == NONE).all()
                # hits() unpacks what the arrays hold
                (ia, ka), (ib, kb) = state.hits()
                for idx, key, packed in ((ia, ka, want[0]), (ib, kb, want[1])):
                    none = packed == NONE
                    assert idx.dtype == key.dtype == np.int64 and (idx[none] == -1).all() and (key[none] == -1).all()
                    assert np.array_equal(idx[~none], (packed[~none] & np.uint64(0xffffffff)).astype(np.int64))
                    assert np.array_equal(key[~none], (packed[~none] >> np.uint64(32)).astype(np.int64))
                if bound == 2 and flags[0] is None:
                    key = np.minimum(t.astype(np.int64) & 0xffffffff, CAP)
                    tied += int(((key == key.min(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
    assert tied > 0 or n_cols < 3                                # (the minima this test ranks are tied)


def test_rect_best_refuses_what_it_cannot_hold():
    import torch
    from dctdomain_amd import _lib
    from dctdomain_amd.similarity import BestState, rect_best
    tile = torch.zeros((4, 8), dtype=torch.int32, device='cuda')
    state = BestState(4, 8)
    for bad in (tile.long(), tile[0], tile.t(), tile.cpu()):
        with pytest.raises(ValueError):
            rect_best(bad, 0, 0, 5, state)
    with pytest.raises(ValueError):
        rect_best(tile, -1, 0, 5, state)
    for row0, col0 in ((1, 0), (0, 1)):
        with pytest.raises(IndexError):
            rect_best(tile, row0, col0, 5, state)
    with pytest.raises(_lib.DctfpError) as err:                  # (key << 10 | column must fit 32 bits)
        rect_best(tile, 0, 0, 5, state, cap=1 << 22)
    assert err.value.code == _lib.DCTFP_ERR_INVALID and 'dctfp_rect_best' in err.value.msg
    rect_best(tile[:0], 0, 0, 5, state)                          # an empty tile: nothing launched, nothing written
    rect_best(tile[:, :0], 0, 0, 5, state)
    assert (state.best_row == -1).all() and (state.best_col == -1).all()
    rect_best(tile, 0, 0, 10 ** 9, state, cap=(1 << 22) - 2)     # the largest cap; a bound beyond it is clipped to it
    assert state.best_row.tolist() == [0] * 4 and state.best_col.tolist() == [0] * 8


# ---- 2. accumulation

def test_sub_tiles_in_any_order_equal_one_call():
    from dctdomain_amd.similarity import BestState, rect_best
    n_rows, n_cols = SHAPES[-1]
    rng = np.random.default_rng(7)
    t = _tile(rng, n_rows, n_cols)
    view = _view(t)
    row_empty, col_empty = rng.random(n_rows) < 0.1, rng.random(n_cols) < 0.1
    whole = BestState(n_rows + 1, n_cols + 1)
    rect_best(view, 1, 1, 3, whole, row_empty, col_empty)
    parts = [(r0, r1, c0, c1) for r0, r1 in ((0, 67), (67, n_rows)) for c0, c1 in ((0, 1000), (1000, 1029), (1029, n_cols))]
    cut = BestState(n_rows + 1, n_cols + 1)
    for k in rng.permutation(len(parts)).tolist():
        r0, r1, c0, c1 = parts[k]
        rect_best(view[r0:r1, c0:c1], 1 + r0, 1 + c0, 3, cut, row_empty[r0:r1], col_empty[c0:c1])
    assert all(np.array_equal(a, b) for a, b in zip(_state_arrays(cut), _state_arrays(whole)))
    assert all(np.array_equal(a, b) for a, b in zip(_state_arrays(whole), _np_best(t, 1, 1, 3, n_rows + 1, n_cols + 1, row_empty, col_empty)))


# ---- 3. ReciprocalBest against the oracle

def _families(seed, width, families=30, members=5, dups=6, bare=5):
    """Two files of planted families: (sid, idx, fps) each.  Every protein has 1-4 fingerprints = its family's centre + noise; B
    holds a permutation of the members (built anew); on each side `dups` proteins are repeated at random positions and `bare`
    proteins without fingerprints are inserted."""
    rng = np.random.default_rng(seed)
    centre = rng.integers(0, 128, size=(families, width))

    def side(tag, order):
        prots = []
        for f in order:
            k = int(rng.integers(1, 5))
            prots.append(np.clip(centre[f] + rng.integers(-20, 21, size=(k, width)), 0, 127).astype(np.int8))
        for _ in range(dups):
            prots.insert(int(rng.integers(0, len(prots) + 1)), prots[int(rng.integers(0, len(prots)))].copy())
        for _ in range(bare):
            prots.insert(int(rng.integers(0, len(prots) + 1)), np.zeros((0, width), dtype=np.int8))
        idx = np.concatenate([[0], np.cumsum([len(p) for p in prots])]).astype(np.int64)
        return [f'{tag}{k:03d}' for k in range(len(prots))], idx, np.concatenate(prots)

    members_of = np.repeat(np.arange(families), members)
    return side('a', members_of), side('b', rng.permutation(members_of))


_CASES = {}


def _case(width):
    """(file A, file B, {score: key matrix}) of a width, computed once."""
    if width not in _CASES:
        a, b = _families(11, width)
        _CASES[width] = (a, b, {s: rrule.keys(a[2], a[1], b[2], b[1], s) for s in ('domain', 'global')})
    return _CASES[width]


@pytest.fixture
def small_tiles(monkeypatch):
    from dctdomain_amd import dct_sim
    monkeypatch.setattr(dct_sim.ReciprocalBest, 'COL_ROWS', 64)
    monkeypatch.setattr(dct_sim.ReciprocalBest, 'TILE_INTS', 1000)
    return dct_sim


def _assert_same(job, k, bound):
    want_best, want_pairs = rrule.best(k, bound), rrule.pairs(k, bound)
    got_best, got_pairs = job.best(), job.pairs()
    for got, want in zip(got_best, want_best):
        assert all(g.dtype == np.int64 and np.array_equal(g, w) for g, w in zip(got, want))
    assert len(got_pairs) == 3 and all(g.dtype == np.int64 and np.array_equal(g, w) for g, w in zip(got_pairs, want_pairs))


@pytest.mark.parametrize('cut', [None, 0.65])
@pytest.mark.parametrize('score', ['domain', 'global'])
def test_reciprocal_best_against_the_oracle(small_tiles, score, cut):
    dct_sim = small_tiles
    a, b, keys = _case(480)
    k = keys[score]
    assert len(a[0]) == len(b[0]) == 161
    bound = rrule.DEFAULT_BOUND if cut is None else min(dct_sim.sim_bound(cut), rrule.DEFAULT_BOUND)
    # what the oracle says about the case: it exercises hits, ties and the cut-off
    (best_b, key_a), _ = rrule.best(k)
    assert (best_b >= 0).sum() >= 100 and 40 <= len(rrule.pairs(k)[0]) <= 140
    assert ((k == k.min(axis=1, keepdims=True)) & (k <= rrule.DEFAULT_BOUND)).sum(axis=1).max() > 1      # a row with a tied minimum
    kg = keys['global']
    assert (rrule.best(kg, min(dct_sim.sim_bound(0.65), rrule.DEFAULT_BOUND))[0][0] >= 0).sum() < (rrule.best(kg)[0][0] >= 0).sum()
    job = dct_sim.ReciprocalBest(*a, *b, score=score, min_cut=cut)
    assert len(job.groups) > 1 and job.bound == bound            # (B in several groups; A in several tiles: TILE_INTS < 161 x a group)
    _assert_same(job, k, bound)


@pytest.mark.parametrize('score', ['domain', 'global'])
def test_reciprocal_best_at_a_width_that_is_no_multiple_of_16(small_tiles, score):
    a, b, keys = _case(100)
    _assert_same(small_tiles.ReciprocalBest(*a, *b, score=score), keys[score], rrule.DEFAULT_BOUND)


def test_a_file_against_itself_pairs_every_protein_that_has_a_fingerprint_with_itself_or_its_first_copy(small_tiles):
    a, _, _ = _case(480)
    job = small_tiles.ReciprocalBest(*a, *a, score='domain')
    k = rrule.keys(a[2], a[1], a[2], a[1], 'domain')
    _assert_same(job, k, rrule.DEFAULT_BOUND)
    pa, pb, key = job.pairs()
    has = np.flatnonzero(np.diff(a[1]) > 0)
    assert (key == 0).all() and (pb <= pa).all() and (job.best()[0][1][has] == 0).all()


# ---- 4. the text

def _write_npz(path, side):
    sid, idx, fps = side
    np.savez(path, sid=np.asarray(sid), idx=idx, dct=fps)
    return str(path)


@pytest.mark.parametrize('score', ['domain', 'global'])
def test_rbh_sim_text(tmp_path, small_tiles, score):
    a, b, keys = _case(480)
    pa, pb = _write_npz(tmp_path / 'a-dct.npz', a), _write_npz(tmp_path / 'b-dct.npz', b)
    out = str(tmp_path / 'out.txt')
    small_tiles.rbh_sim(pa, pb, out, score=score)
    want = rrule.text(a[0], a[2], a[1], b[0], b[2], b[1], score)
    assert open(out).read().splitlines() == [rrule.HEADER] + want and len(want) >= 40
    small_tiles.rbh_sim(pa, pb, out, score=score, domains=True)
    wide = rrule.text(a[0], a[2], a[1], b[0], b[2], b[1], score, domains=True)
    assert open(out).read().splitlines() == [rrule.HEADER + ' dom1 dom2'] + wide
    assert [' '.join(line.split()[:4]) for line in wide] == want


def test_main_on_the_reference_golden_prints_the_reference_lines(tmp_path):
    from dctdomain_amd import dct_sim
    _, want = rrule.reference_rbh_lines()
    out = str(tmp_path / 'out.txt')
    q, db = (os.path.join(rrule.GOLD, name + '-dct.npz') for name in ('query', 'db'))
    dct_sim.main(['--dct', q, '--db', db, '--rbh', 'global', '--output', out])
    assert open(out).read().splitlines() == [rrule.HEADER] + want and len(want) == 27
