"""dct-sim --hac (dct_sim.Dendrogram; dctfp_linkage_nearest / dctfp_linkage_merge) against the numpy oracle of linkage_rule.py (pinned
on the CPU in test_linkage_host.py): the scan kernel on hand-made matrices -- both element types, every alignment, ties across
lanes, waves and load steps, the bound exactly, the 64-bit edge --, one round of the merge kernel, whole trees on the two
committed fixtures and on random ragged files, a shuffled chain, 4 000 proteins in planted families and the command line."""

import os

import numpy as np
import pytest

import golden_util as gu
import linkage_rule as lr

pytestmark = pytest.mark.gpu
NPZ = os.path.join(gu.GOLD, 'all_sim', 'all-dct.npz')
G6PD = os.path.join(gu.GOLD, 'ref_fixtures', 'G6PD-dct.npz')
NONE = {np.int32: 0x7fffffff, np.int64: 0x7fffffffffffffff}


def _load(path):
    with np.load(path) as data:
        return [str(s) for s in data['sid']], np.asarray(data['idx'], dtype=np.int64), data['dct']


_KEYS = {}


def _keys(path, score):
    """The fixture's key matrix, computed once per run and never changed."""
    if (path, score) not in _KEYS:
        sid, idx, dct = _load(path)
        key = lr.keys_of(dct, idx, score)
        key.setflags(write=False)
        _KEYS[path, score] = key
    return _KEYS[path, score]


# ---- 1. linkage_nearest against numpy

def _np_nearest(mat, size, live, bound):
    """nn (int64, n; -1 outside ``live``) by the rule; the order of two fractions is decided in Python ints (linkage_rule._exact_min)."""
    n = mat.shape[1]
    wide = mat.dtype == np.int64
    none = NONE[mat.dtype.type]
    size = np.asarray(size, dtype=np.int64)
    w = np.where(size > 0, size, 1) if wide else np.ones(n, dtype=np.int64)
    nn = np.full(n, -1, dtype=np.int64)
    for a in live:
        v = mat[a].astype(np.int64)
        ok = (np.arange(n) != a) & (size > 0) & (v != none)
        ok &= v <= (bound * int(size[a]) * w if wide else bound)
        c = np.flatnonzero(ok)
        if len(c):
            nn[a] = c[lr._exact_min(v[c], w[c], c)]
    return nn


def _device_matrix(mat, shift, pad):
    """``mat`` on the device as a column view at element offset ``shift`` of a wider tensor: ld = n + shift + pad, the padding
    holds 0 (the nearest of all if it were read)."""
    import torch
    rows, n = mat.shape
    big = torch.zeros((rows, n + shift + pad), dtype=torch.int32 if mat.dtype == np.int32 else torch.int64, device='cuda')
    view = big[:, shift:shift + n]
    view.copy_(torch.as_tensor(mat, device='cuda'))
    return big, view


def _run_nearest(mat, size, live, bound, shift=0, pad=0):
    import torch
    from dctdomain_amd.similarity import linkage_nearest
    _big, view = _device_matrix(mat, shift, pad)
    nn = linkage_nearest(view, torch.as_tensor(size.astype(np.int32), device='cuda'), torch.as_tensor(np.asarray(live, dtype=np.int32), device='cuda'),
                         bound)
    return nn.cpu().numpy().astype(np.int64)


def _random_state(rng, n, dtype, bound, values):
    """A symmetric matrix of ``values`` distinct keys (ties everywhere when few), sizes 1 .. 3 with some dead columns."""
    size = rng.integers(1, 4, size=n)
    size[rng.random(n) < 0.15] = 0
    if n > 1 and not size.any():
        size[0] = 1
    k = rng.integers(0, values, size=(n, n)) * max(1, (bound + bound // 3) // values)
    k = np.triu(k, 1)
    k = k + k.T
    if dtype == np.int64:                                       # S of clusters of these sizes at a mean of k
        k = k * size[:, None] * size[None, :]
    mat = k.astype(dtype)
    mat[rng.random((n, n)) < 0.1] = NONE[dtype]                  # (sentinel entries anywhere: never a neighbour)
    np.fill_diagonal(mat, NONE[dtype])
    return mat, size


@pytest.mark.parametrize('dtype', [np.int32, np.int64])
@pytest.mark.parametrize('n', [1, 2, 3, 63, 64, 65, 257, 1025])
def test_nearest_kernel_against_numpy(n, dtype):
    """nn per live row exactly, at every alignment of the base (shift 0 .. 3 entries: the head of 0 .. 3 dword / 0 .. 1 qword loads
    in front of the 16-byte body) with ld > n, few distinct values (ties to the lowest id, across lanes, waves and steps) and
    many, sentinel entries, dead columns, the full live list and a subset of it."""
    rng = np.random.default_rng(100 * n + (dtype == np.int64))
    for shift in range(4):
        for values in (3, 5000):
            bound = 9000
            mat, size = _random_state(rng, n, dtype, bound, values)
            alive = np.flatnonzero(size > 0)
            live = alive if shift % 2 == 0 else alive[rng.random(len(alive)) < 0.5]
            want = _np_nearest(mat, size, live, bound)
            got = _run_nearest(mat, size, live, bound, shift=shift, pad=int(rng.integers(0, 6)))
            assert np.array_equal(got, want), (n, dtype, shift, values)


@pytest.mark.parametrize('dtype', [np.int32, np.int64])
def test_nearest_all_equal_sentinel_columns_and_a_single_live_row(dtype):
    n = 700
    mat = np.full((n, n), 1234, dtype=dtype)
    np.fill_diagonal(mat, NONE[dtype])
    size = np.ones(n, dtype=np.int64)
    got = _run_nearest(mat, size, np.arange(n), 16999)
    assert got[0] == 1 and (got[1:] == 0).all()                  # all entries equal: the lowest id
    mat[:, :5] = NONE[dtype]                                     # sentinel columns: never chosen
    got = _run_nearest(mat, size, np.arange(n), 16999)
    assert (got[:5] == 5).all() and got[5] == 6 and (got[6:] == 5).all()
    got = _run_nearest(mat, size, [n - 1], 16999)                # a single live row: the others are left alone
    assert got[n - 1] == 5 and (got[:n - 1] == -1).all()
    got = _run_nearest(mat, size, np.arange(n), 1233)            # nothing within the bound
    assert (got == -1).all()


@pytest.mark.parametrize('where', [(0, 1), (63, 64), (255, 256), (1023, 1024), (3, 1500)])
def test_nearest_tie_spans_lanes_waves_and_steps(where):
    """Two columns at the same smallest distance -- neighbours in one 16-byte load, in two lanes, two waves (64 lanes x 4 entries
    = 256 apart) and two load steps (1024 entries apart): the lower id; the higher wins once it is strictly smaller."""
    n, (x, y) = 2100, where
    for dtype in (np.int32, np.int64):
        mat = np.full((n, n), 9000, dtype=dtype)
        np.fill_diagonal(mat, NONE[dtype])
        size = np.ones(n, dtype=np.int64)
        a = 2000
        mat[a, x] = mat[a, y] = 7
        assert _run_nearest(mat, size, [a], 16999)[a] == x
        mat[a, y] = 6
        assert _run_nearest(mat, size, [a], 16999)[a] == y


def test_nearest_bound_is_inclusive():
    """D = bound merges, bound + 1 does not; for average S = bound ca cb against one more."""
    n, bound = 70, 6800
    mat = np.full((n, n), 17000, dtype=np.int32)
    np.fill_diagonal(mat, NONE[np.int32])
    mat[3, 40] = mat[40, 3] = bound
    mat[5, 41] = mat[41, 5] = bound + 1
    got = _run_nearest(mat, np.ones(n, dtype=np.int64), np.arange(n), bound)
    assert got[3] == 40 and got[40] == 3 and got[5] == -1 and got[41] == -1 and (got >= 0).sum() == 2
    size = np.full(n, 3, dtype=np.int64)
    size[40], size[41] = 5, 7
    wide = np.full((n, n), 17000 * 49, dtype=np.int64)
    np.fill_diagonal(wide, NONE[np.int64])
    wide[3, 40] = wide[40, 3] = bound * 3 * 5
    wide[5, 41] = wide[41, 5] = bound * 3 * 7 + 1
    got = _run_nearest(wide, size, np.arange(n), bound)
    assert got[3] == 40 and got[40] == 3 and got[5] == -1 and got[41] == -1 and (got >= 0).sum() == 2


def test_nearest_average_goes_by_the_mean_not_the_sum():
    """Unequal sizes: the larger S has the smaller mean."""
    n = 130
    size = np.ones(n, dtype=np.int64)
    size[100], size[7] = 10, 2
    wide = np.full((n, n), NONE[np.int64], dtype=np.int64)
    a = 64
    wide[a, 7] = 2 * 500                                         # mean 500
    wide[a, 100] = 10 * 499                                      # mean 499: S five times as large
    wide[a, 120] = 501
    assert _run_nearest(wide, size, [a], 16999)[a] == 100
    wide[a, 100] = 10 * 500                                      # equal means: the lower id
    assert _run_nearest(wide, size, [a], 16999)[a] == 7


def test_nearest_at_the_64_bit_edge():
    """Three live clusters of 15 446 proteins each among 46 338 nodes, S = 17000 ca cx on every pair: S cy = 6.26e16, which 64 bits
    hold and 2^53 does not; one unit less on one entry decides.  (Only the three live rows of the matrix exist.)"""
    import torch
    from dctdomain_amd.similarity import linkage_nearest
    n, c = 46338, 15446
    full = 17000 * c * c
    mat = torch.full((3, n), NONE[np.int64], dtype=torch.int64, device='cuda')
    size = torch.zeros(n, dtype=torch.int32, device='cuda')
    size[:3] = c
    for a in range(3):
        for x in range(3):
            if a != x:
                mat[a, x] = full
    live = torch.arange(3, dtype=torch.int32, device='cuda')
    assert linkage_nearest(mat, size, live, 17000)[:3].tolist() == [1, 0, 0]
    mat[0, 2] = mat[2, 0] = full - 1
    assert linkage_nearest(mat, size, live, 17000)[:3].tolist() == [2, 0, 0]
    mat[0, 2] = mat[2, 0] = full + 1                             # one past the bound
    assert linkage_nearest(mat, size, live, 17000)[:3].tolist() == [1, 0, 1]
    assert (linkage_nearest(mat, size, live, 16999)[:3] == -1).all()


@pytest.mark.parametrize('n', [65, 1025])
def test_nearest_complete_equals_rect_best(n):
    """For complete linkage with every column live, nn is the column of dctfp_rect_best's best_row on the same matrix."""
    import torch
    from dctdomain_amd.similarity import BestState, rect_best
    rng = np.random.default_rng(n)
    mat, _ = _random_state(rng, n, np.int32, 9000, 40)
    size = np.ones(n, dtype=np.int64)
    got = _run_nearest(mat, size, np.arange(n), 9000)
    state = BestState(n, n)
    rect_best(torch.as_tensor(mat, device='cuda'), 0, 0, 9000, state)       # (the sentinel counts as the cap, 17000: beyond the bound)
    (col, key), _ = state.hits()
    assert np.array_equal(got, col)


# ---- 2. linkage_merge, one round against numpy

def _np_merge(mat, size, pairs):
    """The matrix after the round (entries of dead and dying rows / columns as they were), by the rule's four pre-round values."""
    old, new = mat.astype(object), mat.astype(object)
    comb = max if mat.dtype == np.int32 else (lambda u, v: u + v)
    partner = {a: b for a, b in pairs}
    dying = {b for _, b in pairs}
    n = len(mat)
    for x, px in pairs:
        for y in range(n):
            if y == x or size[y] <= 0 or y in dying:
                continue
            v = comb(old[x, y], old[px, y])
            if y in partner:
                v = comb(v, comb(old[x, partner[y]], old[px, partner[y]]))
            new[x, y] = new[y, x] = v
    return new.astype(mat.dtype)


def _run_merge(mat, size, pairs, shift=0, pad=0):
    import torch
    from dctdomain_amd.similarity import linkage_merge
    n = len(mat)
    _big, view = _device_matrix(mat, shift, pad)
    partner = np.full(n, -1, dtype=np.int32)
    for a, b in pairs:
        partner[a], partner[b] = b, a
    linkage_merge(view, torch.as_tensor(size.astype(np.int32), device='cuda'), torch.as_tensor(partner, device='cuda'),
                  torch.as_tensor(np.array([a for a, _ in pairs], dtype=np.int32), device='cuda'))
    return view.cpu().numpy()


def _random_pairs(rng, alive, count):
    pick = rng.permutation(alive)[:2 * count].reshape(-1, 2)
    return [(int(min(p)), int(max(p))) for p in pick]


@pytest.mark.parametrize('dtype', [np.int32, np.int64])
@pytest.mark.parametrize('n,count', [(2, 1), (5, 2), (64, 1), (257, 60), (300, None), (1025, 300)])
def test_merge_kernel_against_numpy(n, count, dtype):
    """Random disjoint pairs, one pair, every live cluster in a pair (count None): the new matrix exactly -- symmetric between live
    clusters, rows and columns of clusters without a pair byte-identical outside the merged ones, and dead rows and columns
    never win the next scan."""
    rng = np.random.default_rng(7 * n + (dtype == np.int64))
    mat, size = _random_state(rng, n, dtype, 9000, 5000)
    mat[mat == NONE[dtype]] = 77
    mat = np.triu(mat, 1) + np.triu(mat, 1).T                    # (the state is symmetric: the sentinel entries above fell on one side)
    np.fill_diagonal(mat, NONE[dtype])
    if count is None:
        size[:] = np.maximum(size, 1)
    alive = np.flatnonzero(size > 0)
    pairs = _random_pairs(rng, alive, len(alive) // 2 if count is None else min(count, len(alive) // 2))
    want = _np_merge(mat, size, pairs)
    got = _run_merge(mat, size, pairs, shift=n % 3, pad=n % 4)
    assert np.array_equal(got, want)
    merged = {x for p in pairs for x in p}
    after = size.copy()
    for a, b in pairs:
        after[a], after[b] = size[a] + size[b], 0
    left = np.flatnonzero(after > 0)
    sub = got[np.ix_(left, left)]
    assert np.array_equal(sub, sub.T)
    quiet = np.array([x for x in range(n) if x not in merged], dtype=np.int64)
    assert np.array_equal(got[np.ix_(quiet, quiet)], mat[np.ix_(quiet, quiet)])
    for b in (x for _, x in pairs):                              # dying rows and columns keep their values ...
        assert np.array_equal(got[b], mat[b]) and np.array_equal(got[:, b], mat[:, b])
    bound = 17000
    nn = _run_nearest(got, after, left, bound)                   # ... and never win the next scan
    assert np.array_equal(nn, _np_nearest(got, after, left, bound))
    assert not np.isin(nn[left], np.flatnonzero(after == 0)).any()


# ---- 3. Dendrogram against the rule

BOUNDS = [None, 0.5, 0.6, 'l1:3000']


def _cut_of(b):
    """(min_cut, bound): 'l1:K' = a cut-off whose bound is K."""
    from dctdomain_amd.dct_sim import sim_bound
    if b is None:
        return None, 16999
    if isinstance(b, str):
        k = int(b[3:])
        cut = 1 - k / 17000
        assert sim_bound(cut) == k
        return cut, k
    return b, sim_bound(b)


def _as_tuples(merges):
    return [tuple(int(v[k]) for v in merges) for k in range(len(merges[0]))]


@pytest.mark.parametrize('b', BOUNDS)
@pytest.mark.parametrize('method', lr.METHODS)
@pytest.mark.parametrize('score', ['domain', 'global'])
@pytest.mark.parametrize('path', [NPZ, G6PD], ids=['all', 'g6pd'])
def test_dendrogram_of_the_fixtures(path, score, method, b):
    from dctdomain_amd import dct_sim
    sid, idx, dct = _load(path)
    cut, bound = _cut_of(b)
    want, rounds = lr.rounds(_keys(path, score), bound, method)
    tree = dct_sim.Dendrogram(sid, idx, dct, method=method, score=score, min_cut=cut)
    assert _as_tuples(tree.merges()) == lr.ordered(want)
    assert tree.rounds == rounds
    assert tree.heights() == [(m[2], m[3]) for m in lr.ordered(want)]
    assert np.array_equal(tree.labels(), lr.labels_at(len(sid), want, bound))


def _ragged_file(rng, n, d=24, families=12):
    """n proteins of 0 .. 4 fingerprints in a few families, some without any, some a copy of an earlier one (planted ties)."""
    centres = rng.integers(-100, 100, size=(families, d))
    prot = []
    for p in range(n):
        if p >= families and rng.random() < 0.2:
            prot.append(prot[int(rng.integers(0, p))].copy())
            continue
        k = 0 if rng.random() < 0.05 else int(rng.integers(1, 5))
        noise = rng.integers(-12, 13, size=(k, d)) * (rng.random((k, d)) < 0.3)
        prot.append(np.clip(centres[p % families] + noise, -127, 127).astype(np.int8).reshape(k, d))
    idx = np.concatenate([[0], np.cumsum([len(x) for x in prot])]).astype(np.int64)
    return [f'p{p}' for p in range(n)], idx, np.concatenate(prot, axis=0)


@pytest.mark.parametrize('method', lr.METHODS)
@pytest.mark.parametrize('score,seed', [('domain', 1), ('global', 2)])
def test_dendrogram_of_random_ragged_files(score, seed, method):
    from dctdomain_amd import dct_sim
    sid, idx, dct = _ragged_file(np.random.default_rng(seed), 200 + seed)
    key = lr.keys_of(dct, idx, score)
    for cut in (None, 0.9):
        bound = 16999 if cut is None else dct_sim.sim_bound(cut)
        want, rounds = lr.rounds(key, bound, method)
        tree = dct_sim.Dendrogram(sid, idx, dct, method=method, score=score, min_cut=cut)
        assert _as_tuples(tree.merges()) == lr.ordered(want) and tree.rounds == rounds
        if cut is None:                                          # labels(cut) = a fresh tree at that cut
            for c in (0.97, 0.9, 0.5):
                fresh = dct_sim.Dendrogram(sid, idx, dct, method=method, score=score, min_cut=c)
                assert np.array_equal(tree.labels(c), fresh.labels())
        else:
            with pytest.raises(ValueError):
                tree.labels(0.5)


@pytest.mark.parametrize('method', lr.METHODS)
def test_shuffled_chain_takes_many_rounds(method):
    """300 proteins on a line with growing gaps, in shuffled order: nearest neighbours are rarely mutual, so the rule needs many
    rounds -- the count is the rule's, whatever it is."""
    from dctdomain_amd import dct_sim
    rng = np.random.default_rng(5)
    n, d = 300, 180
    pos = np.cumsum(np.arange(n))                                # gaps 1, 2, 3, ...: the chain merges from one end
    assert pos[-1] < d * 254                                     # (a thermometer code: L1 of two rows = the distance of their positions)
    fp = np.zeros((n, d), dtype=np.int64)
    for k in range(d):
        fp[:, k] = np.clip(pos - k * 254 - 127, -127, 127)
    order = rng.permutation(n)
    dct = fp[order].astype(np.int8)
    idx = np.arange(n + 1, dtype=np.int64)
    sid = [f'c{p}' for p in order]
    want, rounds = lr.rounds(lr.keys_of(dct, idx, 'global'), 16999, method)
    tree = dct_sim.Dendrogram(sid, idx, dct, method=method, score='global')
    assert _as_tuples(tree.merges()) == lr.ordered(want)
    assert tree.rounds == rounds and rounds > 20


@pytest.mark.parametrize('method', lr.METHODS)
def test_planted_families_of_4000_proteins(tmp_path, method):
    """--flat at the planted cut recovers the families: members within 0.5 of each other, families further apart."""
    from dctdomain_amd import dct_sim
    rng = np.random.default_rng(11)
    n, fams, d = 4000, 80, 256
    centres = rng.choice([-100, 100], size=(fams, d))
    fam = rng.permutation(np.arange(n) % fams)
    dct = (centres[fam] + rng.integers(-8, 9, size=(n, d))).astype(np.int8)                       # inside a family: L1 <= 256 * 16 = 4096
    assert dct_sim.sim_bound(0.5) == 8500
    assert np.abs(centres[:, None, :] - centres[None, :, :]).sum(axis=2)[np.triu_indices(fams, 1)].min() - 4096 > 8500
    path = str(tmp_path / 'fam-dct.npz')
    np.savez(path, sid=np.array([f'f{fam[p]}_{p}' for p in range(n)]), idx=np.arange(n + 1), dct=dct)
    out = str(tmp_path / 'flat.txt')
    dct_sim.main(['--dct', path, '--output', out, '--hac', 'global', '--method', method, '--min-global', '0.5', '--flat'])
    first = np.full(fams, n)
    np.minimum.at(first, fam, np.arange(n))
    assert open(out, 'rb').read() == b'#representative member\n' + lr.flat_text([f'f{fam[p]}_{p}' for p in range(n)], first[fam])


@pytest.mark.parametrize('method', lr.METHODS)
@pytest.mark.parametrize('score,cut', [('domain', None), ('domain', 0.6), ('global', 0.6)])
def test_main_end_to_end(tmp_path, score, cut, method):
    """The three texts byte for byte: the merge lines, --flat and --newick."""
    from dctdomain_amd import dct_sim
    sid, idx, dct = _load(G6PD)
    bound = 16999 if cut is None else dct_sim.sim_bound(cut)
    want, _ = lr.rounds(_keys(G6PD, score), bound, method)
    out, nwk = str(tmp_path / 'out.txt'), str(tmp_path / 'out.nwk')
    argv = ['--dct', G6PD, '--output', out, '--hac'] + ([score] if score != 'domain' else []) + ['--method', method, '--newick', nwk]
    if cut is not None:
        argv += ['--min-' + score, str(cut)]
    dct_sim.main(argv)
    assert open(out, 'rb').read() == lr.text(sid, want)
    assert open(nwk, 'rb').read() == lr.newick(sid, want)
    if cut is not None:
        dct_sim.main(argv + ['--flat'])
        assert open(out, 'rb').read() == b'#representative member\n' + lr.flat_text(sid, lr.labels_at(len(sid), want, bound))
        assert open(nwk, 'rb').read() == lr.newick(sid, want)
