"""dct-sim --cluster --linkage greedy (dct_sim.Representatives; dctfp_greedy_decide / dctfp_greedy_tri_mark / dctfp_greedy_pairs_mark)
against the plain-Python oracle of greedy_rule.py (worked by hand on the CPU in test_greedy_host.py): the reference golden, the
filtered mode's own edges on random ragged files, independence from the partition, chains -- where the rounds can go wrong --,
the mark kernels on hand-made tiles and pair lists, bad arguments, and 20 000 proteins with planted families."""

import os

import numpy as np
import pytest

import all_sim_filter_rule as rule
import cluster_rule as crule
import golden_util as gu
import greedy_rule as grule
from test_cluster_gpu import _RAGGED_CUTS, CUTS

pytestmark = pytest.mark.gpu
NPZ = os.path.join(gu.GOLD, 'all_sim', 'all-dct.npz')
NONE = 0x7fffffff
UNDECIDED, MEMBER, NEW, DONE = 0, 1, 2, 3


def _run(path, out, *flags, min_domain=None, min_global=None) -> bytes:
    from dctdomain_amd import dct_sim
    argv = ['--dct', path, '--output', out, '--cluster', *flags]
    for name, v in (('--min-domain', min_domain), ('--min-global', min_global)):
        if v is not None:
            argv += [name, str(v)]
    dct_sim.main(argv)
    with open(out, 'rb') as fh:
        return fh.read()


def _oracle(tri, n, min_domain=None, min_global=None):
    """greedy_rule.labels from a triangle computed once: (labels, i, j of the kept edges)."""
    i, j, mn, last = tri
    keep = rule.kept(mn, last, min_domain, min_global)
    return grule.greedy(n, i[keep], j[keep]), i[keep], j[keep]


# ---- 1. the reference golden

@pytest.fixture(scope='module')
def golden():
    with np.load(NPZ) as data:
        sid, idx, dct = [str(s) for s in data['sid']], np.asarray(data['idx'], dtype=np.int64), data['dct']
    return sid, idx, dct, rule.triangle_l1(dct, idx)


@pytest.mark.parametrize('kw', CUTS, ids=lambda kw: ','.join(f'{k[4:]}={v}' for k, v in kw.items()))
def test_reference_golden(tmp_path, golden, kw):
    from dctdomain_amd import dct_sim
    sid, idx, dct, tri = golden
    want, i, j = _oracle(tri, 139, **kw)
    r = dct_sim.Representatives(sid, idx, dct, **kw)
    got = r.labels()
    assert got.dtype == np.int32 and np.array_equal(got, want)
    grule.check(139, i, j, got)
    assert r.rounds >= 1
    out = str(tmp_path / 'out.txt')
    assert _run(NPZ, out, '--linkage', 'greedy', **kw) == grule.HEADER + grule.text(sid, want)
    single = crule.components(139, i, j)
    assert _run(NPZ, out, **kw) == crule.HEADER + crule.text(sid, single) == _run(NPZ, out, '--linkage', 'single', **kw)


# ---- 2. the filtered mode's own edges, on random ragged files

_ALPHABET = list('abcdefghijklmnopqrstuvwxyz0123456789_|.-') + ['é', 'ß', 'α', '蛋', '😀']


def _ragged(seed, n):
    """Proteins of 0-3 fingerprints (15 % empty) from four families at L1 ~ 6 500 (0.62) within a family, plus planted near
    copies (+-2) of single fingerprints at random places of other proteins (test_cluster_gpu's generator)."""
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


@pytest.mark.parametrize('seed,n', [(1, 60), (2, 150), (3, 2), (4, 300)])
def test_greedy_of_the_filtered_pairs(seed, n):
    from dctdomain_amd import dct_sim
    sid, idx, dct = _ragged(seed, n)
    assert (np.diff(idx) == 0).any() or n < 10
    tri = rule.triangle_l1(dct, idx)
    seen, differs = set(), 0
    for min_domain, min_global in _RAGGED_CUTS:
        i, j, _, _ = dct_sim.FilteredPairs(sid, idx, dct, min_domain, min_global).pairs()
        want = grule.greedy(n, i, j)
        got = dct_sim.Representatives(sid, idx, dct, min_domain, min_global).labels()
        assert got.dtype == np.int32 and np.array_equal(got, want), (min_domain, min_global)
        assert np.array_equal(want, _oracle(tri, n, min_domain, min_global)[0])
        grule.check(n, i, j, got)
        seen.add(len(np.unique(want)))
        differs += not np.array_equal(want, crule.components(n, i, j))
    assert n < 10 or (len(seen) > 2 and differs)              # (the cut-offs fall inside, between and outside the families)


# ---- 3. independence from the partition

@pytest.mark.parametrize('kw', [{'min_domain': 0.62}, {'min_global': 0.62}, {'min_domain': 0.63, 'min_global': 0.6}])
def test_labels_do_not_depend_on_stripes_groups_or_ranges(monkeypatch, kw):
    from dctdomain_amd import dct_sim
    sid, idx, dct = _ragged(7, 90)
    want = grule.labels(dct, idx, **kw)[0]
    assert 2 < len(np.unique(want)) < 80 and not np.array_equal(want, crule.labels(dct, idx, **kw)[0])
    first = dct_sim.Representatives(sid, idx, dct, **kw)
    assert np.array_equal(first.labels(), want) and np.array_equal(first.labels(), want)       # (twice: the same)
    texts = set()
    for tile_ints, col_rows, text_bytes in [(5, 3, 41), (1, 1, 1), (300, 3, 281), (90, 7, 1 << 28), (1000, 40, 100), (1 << 28, 2, 1 << 28)]:
        for name, v in (('TILE_INTS', tile_ints), ('COL_ROWS', col_rows), ('TEXT_BYTES', text_bytes)):
            monkeypatch.setattr(dct_sim.FilteredPairs, name, v)
        r = dct_sim.Representatives(sid, idx, dct, **kw)
        stripes = list(r.stripes())
        assert len(stripes) > 1 and (tile_ints > 1 or all(b - a == 1 for a, b in stripes))      # (one-row stripes among them)
        assert np.array_equal(r.labels(), want), (tile_ints, col_rows, text_bytes)
        assert np.array_equal(r.labels(), want)
        got = []
        r.write(lambda mv: got.append(bytes(mv)))
        texts.add(b''.join(got))
    assert texts == {grule.text(sid, want)}


# ---- 4. chains: neighbours at L1 5 join at the bound of 8, next-neighbours at 10 do not

def _thermometer(levels):
    """One int8 fingerprint per level: L1 between two of them = the difference of their levels (a path through the 480
    coordinates, 250 units along each)."""
    lv = np.asarray(levels, dtype=np.int64)[:, None]
    return (np.clip(lv - 250 * np.arange(480)[None, :], 0, 250) - 125).astype(np.int8)


def _chain_oracle(pos):
    """Labels of the proteins at chain positions `pos` (a permutation of 0 .. n - 1): edges join positions that differ by 1."""
    n = len(pos)
    at = np.empty(n, dtype=np.int64)
    at[pos] = np.arange(n)
    return grule.greedy(n, at[:-1], at[1:]), at[:-1], at[1:]


_CHAIN_CUTS = [{'min_domain': 0.9995}, {'min_global': 0.9995}, {'min_domain': 0.9995, 'min_global': 0.9995}]


@pytest.mark.parametrize('kw', _CHAIN_CUTS, ids=['domain', 'global', 'both'])
@pytest.mark.parametrize('small', [False, True], ids=['one-stripe', 'many-stripes'])
def test_chains_of_three_hundred_and_one(monkeypatch, kw, small):
    from dctdomain_amd import dct_sim
    assert dct_sim.sim_bound(0.9995) == 8
    n = 301
    if small:
        monkeypatch.setattr(dct_sim.FilteredPairs, 'TILE_INTS', 2100)       # 7 rows at first, more further down
        monkeypatch.setattr(dct_sim.FilteredPairs, 'TEXT_BYTES', 300)       # (both cut-offs: ranges of a few rows)
    sid = [f'chain{k:03d}' for k in range(n)]
    idx = np.arange(n + 1, dtype=np.int64)
    in_order = np.arange(n)
    for pos in (in_order, np.random.default_rng(23).permutation(n)):
        r = dct_sim.Representatives(sid, idx, _thermometer(5 * pos), **kw)
        ends = [b for _, b in r.stripes()]
        assert (len(ends) > 10 and {b % 2 for b in ends[:-1]} == {0, 1}) if small else len(ends) == 1
        want, i, j = _chain_oracle(pos)
        got = r.labels()
        assert np.array_equal(got, want)
        grule.check(n, i, j, got)
        if pos is in_order:
            assert got.tolist() == [k - k % 2 for k in range(n)]            # [0, 0, 2, 2, ..., 300]
            assert r.rounds >= 150
        assert len(np.unique(got)) > n // 3                                 # (a maximal independent set of a path)
        assert not dct_sim.Clusters(sid, idx, _thermometer(5 * pos), **kw).labels().any()      # single linkage: one cluster


def test_a_chain_of_three(tmp_path):
    from dctdomain_amd import dct_sim
    sid, idx, dct = ['a', 'b', 'c'], np.arange(4, dtype=np.int64), _thermometer([0, 5, 10])
    for kw in _CHAIN_CUTS:
        assert dct_sim.Clusters(sid, idx, dct, **kw).labels().tolist() == [0, 0, 0]
        assert dct_sim.Representatives(sid, idx, dct, **kw).labels().tolist() == [0, 0, 2]
    path = str(tmp_path / 'three-dct.npz')
    np.savez(path, sid=np.array(sid), idx=idx, dom=np.array(['1-9'] * 3), dct=dct)
    assert _run(path, str(tmp_path / 'out.txt'), '--linkage', 'greedy', min_domain=0.9995) == b'#representative member\na a\na b\nc c\n'
    assert _run(path, str(tmp_path / 'out.txt'), min_domain=0.9995) == b'#representative member\na a\na b\na c\n'


# ---- 5. the mark kernel on hand-made tiles against numpy

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


def _state(n, assign, state, blocked):
    import torch
    from dctdomain_amd.similarity import GreedyState
    gs = GreedyState(n)
    for t, a in ((gs.assign, assign), (gs.state, state), (gs.blocked, blocked)):
        t.copy_(torch.as_tensor(np.asarray(a, dtype=np.int32), device='cuda'))
    return gs


@pytest.mark.parametrize('n_rows,n_cols', [(7, 3000), (1, 5000), (40, 1), (3, 1023), (5, 1025), (64, 64)])
@pytest.mark.parametrize('bound', [0, 8500])
def test_mark_kernel_against_numpy(n_rows, n_cols, bound):
    """New representatives lower assign at every survivor of their rows, undecided rows stamp the survivors below range_end,
    members and finished representatives touch nothing; the bound exactly, entries left of the diagonal and beyond n_cols (the
    padding holds 0 = an edge if it were read), views with ld > n_cols at each of the four 4-byte alignments, the flags."""
    import torch
    from dctdomain_amd.similarity import greedy_tri_mark
    rng = np.random.default_rng(1000 * n_rows + n_cols + bound)
    places = [(10, 5), (n_rows + 3, 0), (0, n_rows + 20), (0, 1), (0, 0), (3, 0)]
    kinds, strides = set(), set()
    for k, (col0, row0) in enumerate(places):
        t = np.full((n_rows, n_cols), bound + 1, dtype=np.int32)
        u = rng.random((n_rows, n_cols))
        t[u < 0.4] = 17000
        t[u > 1 - 6.0 / max(n_cols, 2)] = bound               # (sparse: about six edges per row)
        t[u < 0.02] = -5
        shift = k % 4                                         # the tile's base: 4 * shift bytes off a 16-byte boundary
        pad = 1 + (k - n_cols - shift) % 4                    # the row stride: k + 1 modulo 4
        big = torch.zeros((n_rows, n_cols + pad + shift), dtype=torch.int32, device='cuda')
        view = big[:, shift:shift + n_cols]
        view.copy_(torch.as_tensor(t, device='cuda'))
        assert view.stride(0) > n_cols and (view.data_ptr() - big.data_ptr()) == 4 * shift
        strides.add((view.stride(0) % 4, view.data_ptr() % 16))
        flags = [(None, None), (rng.random(n_rows) < 0.3, None), (None, rng.random(n_cols) < 0.3),
                 (rng.random(n_rows) < 0.2, rng.random(n_cols) < 0.2)][(k + n_rows) % 4]
        n = max(row0 + n_rows, col0 + n_cols) + int(rng.integers(0, 3))
        range_end = [row0 + n_rows, col0 + n_cols // 2, n, 0][k % 4]
        state = rng.integers(0, 4, size=n)
        state[row0:row0 + min(n_rows, 4)] = [UNDECIDED, NEW, MEMBER, DONE][:min(n_rows, 4)]
        if n_rows == 1:
            state[row0] = [NEW, UNDECIDED][k % 2]
        assign = np.where(rng.random(n) < 0.5, NONE, rng.integers(0, n, size=n))
        blocked = rng.integers(0, 6, size=n)
        ei, ej = _np_edges(t, row0, col0, bound, *flags)
        want_assign, want_blocked = assign.copy(), blocked.copy()
        marks = state[ei] == NEW
        np.minimum.at(want_assign, ej[marks], ei[marks])
        stamps = (state[ei] == UNDECIDED) & (ej < range_end)
        want_blocked[ej[stamps]] = 7
        kinds |= {('mark', bool(marks.any())), ('stamp', bool(stamps.any())), ('beyond', bool(((state[ei] == UNDECIDED) & (ej >= range_end)).any())),
                  ('idle', bool(np.isin(state[ei], (MEMBER, DONE)).any()))}
        gs = _state(n, assign, state, blocked)
        greedy_tri_mark(view, row0, col0, bound, gs, range_end, 7, *flags)
        assert np.array_equal(gs.assign.cpu().numpy(), want_assign), (k, 'assign')
        assert np.array_equal(gs.blocked.cpu().numpy(), want_blocked), (k, 'blocked')
        assert np.array_equal(gs.state.cpu().numpy(), state) and gs.left() == 0
        greedy_tri_mark(view, row0, col0, bound, gs, range_end, 7, *flags)       # (a second launch changes nothing)
        assert np.array_equal(gs.assign.cpu().numpy(), want_assign) and np.array_equal(gs.blocked.cpu().numpy(), want_blocked)
        assert n_cols < 3 or (t == bound + 1).sum() > 0.3 * t.size           # (most entries sit one above the bound: none of them counts)
    assert (big.cpu().numpy()[:, shift + n_cols:] == 0).all()
    assert {(1, 0), (2, 4), (3, 8), (0, 12)} <= strides
    assert n_cols < 3 or {('mark', True), ('stamp', True), ('beyond', True)} <= kinds
    assert n_rows < 3 or n_cols < 3 or ('idle', True) in kinds


def test_decide_kernel_on_states_set_by_hand():
    from dctdomain_amd.similarity import greedy_decide
    #         0          1        2        3          4          5          6      7 (outside the range)
    state = [UNDECIDED, MEMBER, NEW, DONE, UNDECIDED, UNDECIDED, UNDECIDED, UNDECIDED]
    assign = [NONE, 0, 2, 3, 2, NONE, NONE, NONE]
    blocked = [0, 9, 9, 9, 9, 9, 4, 3]
    gs = _state(8, assign, state, blocked)
    greedy_decide(gs, 0, 7, 0)                                # the cover pass: members only; 0, 5 and 6 are left
    assert gs.left() == 3
    assert gs.state.cpu().tolist() == [UNDECIDED, MEMBER, DONE, DONE, MEMBER, UNDECIDED, UNDECIDED, UNDECIDED]
    assert gs.assign.cpu().tolist() == assign
    greedy_decide(gs, 0, 7, 9)                                # 5 carries this round's stamp; 0 and 6 (an old stamp) do not
    assert gs.left() == 1
    assert gs.state.cpu().tolist() == [NEW, MEMBER, DONE, DONE, MEMBER, UNDECIDED, NEW, UNDECIDED]
    assert gs.assign.cpu().tolist() == [0, 0, 2, 3, 2, NONE, 6, NONE]
    greedy_decide(gs, 5, 8, 10)
    assert gs.left() == 0
    assert gs.state.cpu().tolist() == [NEW, MEMBER, DONE, DONE, MEMBER, NEW, DONE, NEW]
    assert gs.assign.cpu().tolist() == [0, 0, 2, 3, 2, 5, 6, 7] and gs.blocked.cpu().tolist() == blocked


# ---- 6. lists of pairs, range by range

def _rounds_over_pairs(gs, i0, i1, pi, pj, first_round):
    """The rounds of one range as dctfp.h describes them; returns the next unused round number."""
    from dctdomain_amd.similarity import greedy_decide, greedy_pairs_mark
    greedy_decide(gs, i0, i1, 0)
    if gs.left() == 0:
        return first_round
    r = first_round
    greedy_pairs_mark(pi, pj, gs, i1, r)
    while True:
        greedy_decide(gs, i0, i1, r)
        r += 1
        greedy_pairs_mark(pi, pj, gs, i1, r)
        if gs.left() == 0:
            return r + 1


@pytest.mark.parametrize('n,m', [(50, 30), (1000, 700), (7, 0)])
def test_pairs_mark_against_the_oracle(n, m):
    import torch
    from dctdomain_amd.similarity import GreedyState, greedy_decide
    rng = np.random.default_rng(n + m)
    pi, pj = rng.integers(0, n, size=m), rng.integers(0, n, size=m)
    if m > 20:
        pi[:5], pj[:5] = pj[5:10], pi[5:10]                   # repeats (both ways round)
        pi[10:13] = pj[10:13]                                 # self pairs
        pi[13:17] = [-1, n, 3, 2 ** 31 - 1]                   # out of range: skipped
        pj[13:17] = [4, 5, n + 7, 0]
        pi[17:20], pj[17:20] = [0, 1, 2], [1, 2, 3]           # a path at the start: more than one round
    ok = (pi >= 0) & (pi < n) & (pj >= 0) & (pj < n)
    want = grule.greedy(n, pi[ok], pj[ok])
    lo = np.where(ok, np.minimum(pi, pj), -1)
    dev = lambda a: torch.as_tensor(a.astype(np.int64).astype(np.int32), device='cuda')   # noqa: E731
    for cuts in ([0, n], [0, 1, n // 3, n // 3, n - 2, n]):
        gs = GreedyState(n)
        r = 1
        for i0, i1 in zip(cuts[:-1], cuts[1:]):
            here = ((lo >= i0) & (lo < i1)) | ~ok                 # (the pairs that name no node go to every call)
            r = _rounds_over_pairs(gs, i0, i1, dev(pi[here]), dev(pj[here]), r)
        greedy_decide(gs, n, n, r)
        got = gs.assign.cpu().numpy()
        assert np.array_equal(got, want), cuts
        grule.check(n, pi[ok], pj[ok], got)
        assert m == 0 or r > len(cuts)
        assert not (gs.state.cpu().numpy() == UNDECIDED).any()


# ---- 7. bad arguments

def test_greedy_calls_reject_bad_arguments_and_take_empty_ones():
    import ctypes as C
    import torch
    from dctdomain_amd import _lib
    from dctdomain_amd.similarity import GreedyState, greedy_decide, greedy_pairs_mark, greedy_tri_mark
    t = torch.zeros((6, 100), dtype=torch.int32, device='cuda')
    gs = GreedyState(100)
    a, s, b, u = (x.data_ptr() for x in (gs.assign, gs.state, gs.blocked, gs.undecided))
    ctx = _lib.get_context(0)
    lib = ctx._lib
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    mark = lambda row0=0, col0=0, bound=0, ld=100, n_nodes=100, n_rows=6, end=100, nxt=1, tile=t.data_ptr(), assign=a: lib.dctfp_greedy_tri_mark(   # noqa: E731
        ctx.handle, tile, n_rows, 100, ld, row0, col0, None, None, 17000, bound, assign, s, b, n_nodes, end, nxt, stream)
    assert mark(col0=1) == _lib.DCTFP_ERR_INVALID and mark(row0=95) == _lib.DCTFP_ERR_INVALID      # outside the nodes: on the host
    assert mark(end=101) == _lib.DCTFP_ERR_INVALID and mark(nxt=0) == _lib.DCTFP_ERR_INVALID
    assert mark(bound=17001) == _lib.DCTFP_ERR_INVALID and mark(bound=-2) == _lib.DCTFP_ERR_INVALID and mark(ld=99) == _lib.DCTFP_ERR_INVALID
    assert mark(tile=None) == _lib.DCTFP_ERR_INVALID and mark(assign=None) == _lib.DCTFP_ERR_INVALID
    assert mark(n_nodes=2 ** 31) == _lib.DCTFP_ERR_LIMIT
    decide = lambda i0=0, i1=100, n_nodes=100, rnd=1, und=u, state=s: lib.dctfp_greedy_decide(ctx.handle, a, state, b, n_nodes, i0, i1, rnd, und, stream)   # noqa: E731
    assert decide(i0=5, i1=4) == _lib.DCTFP_ERR_INVALID and decide(i1=101) == _lib.DCTFP_ERR_INVALID and decide(rnd=-1) == _lib.DCTFP_ERR_INVALID
    assert decide(und=None) == _lib.DCTFP_ERR_INVALID and decide(state=None) == _lib.DCTFP_ERR_INVALID
    assert decide(n_nodes=2 ** 31) == _lib.DCTFP_ERR_LIMIT
    pairs = lambda n_pairs=3, n_nodes=100, end=100, nxt=1, p=a, blocked=b: lib.dctfp_greedy_pairs_mark(   # noqa: E731
        ctx.handle, p, p, n_pairs, a, s, blocked, n_nodes, end, nxt, stream)
    assert pairs(n_nodes=2 ** 31) == _lib.DCTFP_ERR_LIMIT and pairs(n_pairs=2 ** 31 + 1) == _lib.DCTFP_ERR_LIMIT
    assert pairs(p=None) == _lib.DCTFP_ERR_INVALID and pairs(blocked=None) == _lib.DCTFP_ERR_INVALID
    assert pairs(end=101) == _lib.DCTFP_ERR_INVALID and pairs(nxt=0) == _lib.DCTFP_ERR_INVALID and pairs(n_pairs=-1) == _lib.DCTFP_ERR_INVALID
    # empty input: nothing to do
    assert mark(n_rows=0) == 0 and decide(i0=40, i1=40) == 0 and pairs(n_pairs=0, p=None) == 0
    assert mark(bound=-1) == 0                                # bound -1: nothing survives
    assert gs.left() == 0 and not gs.state.cpu().numpy().any() and not gs.blocked.cpu().numpy().any()
    assert (gs.assign.cpu().numpy() == NONE).all()            # nothing was touched by any of these
    with pytest.raises(IndexError):
        greedy_tri_mark(t, 0, 1, 0, gs, 100, 1)
    with pytest.raises(IndexError):
        greedy_tri_mark(t, 0, 0, 0, gs, 101, 1)
    with pytest.raises(IndexError):
        greedy_decide(gs, 0, 101, 1)
    with pytest.raises(ValueError):
        greedy_pairs_mark(gs.assign[:3], gs.assign[:2], gs, 100, 1)
    gs.state = gs.state.long()
    with pytest.raises(ValueError):
        greedy_tri_mark(t, 0, 0, 0, gs, 100, 1)
    empty = GreedyState(0)
    greedy_decide(empty, 0, 0, 1)
    assert empty.assign.numel() == 0 and empty.left() == 0


# ---- 8. scale

def test_twenty_thousand_proteins_get_the_first_member_of_their_planted_family(tmp_path):
    """synth's random proteins lie at L1 15 500 +- 500 from each other, far above --min-domain 0.5's bound of 8 500 -- a
    condition on the input, checked below with the oracle on a sample, as test_cluster_gpu's 200 000 proteins are.  Members of a
    family are copies of its first member's rows within +-2 each (L1 <= 1 920 between any two): every member is within the
    cut-off of every other, so greedy's label is the family's lowest index, and every other protein is its own."""
    from dctdomain_amd import dct_sim
    from tools.all_sim_bench import synth
    n, n_fam = 20000, 300
    path = str(tmp_path / 's-dct.npz')
    synth(path, n, 7)
    with np.load(path) as data:
        sid, idx, dct = [str(s) for s in data['sid']], np.asarray(data['idx'], dtype=np.int64), data['dct']
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
    # the condition on the input: 1 000 random pairs outside the families, and members against strangers
    ri, rj = rng.integers(0, n, size=1000), rng.integers(0, n, size=1000)
    rj[:300] = chosen[rng.integers(0, len(chosen), size=300)]
    ok = want[ri] != want[rj]
    rm, rl = rule.pair_l1(dct, idx, ri[ok], rj[ok])
    assert ok.sum() > 950 and not rule.kept(rm, rl, min_domain=0.5).any() and rm.min() > 8500 + 3000
    fi = chosen[:sizes[0]]
    fm, _ = rule.pair_l1(dct, idx, np.repeat(fi[0], len(fi) - 1), fi[1:])
    assert fm.max() <= 1920
    r = dct_sim.Representatives(sid, idx, dct, min_domain=0.5)
    got = r.labels()
    assert np.array_equal(got, want)
    assert len(np.unique(got)) == n - int(sizes.sum()) + n_fam
    assert 1 <= r.rounds <= 4 * len(list(r.stripes()))        # (a family is a clique: its first member, then the others)
    i, j, _, _ = dct_sim.FilteredPairs(sid, idx, dct, min_domain=0.5).pairs()
    assert len(i) == int((sizes * (sizes - 1) // 2).sum())
    assert np.array_equal(got, grule.greedy(n, i, j))
