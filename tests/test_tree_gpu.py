"""dct-sim --tree (dct_sim.Tree; dctfp_tri_nearest / dctfp_tree_hook) against the numpy oracle of tree_rule.py (pinned on the CPU
in test_tree_host.py): the reference golden, the scan kernel on hand-made tiles, ties, the hook on hand-made rounds, the cut
property against dct_sim.Clusters on random ragged files, independence from the partition, a shuffled chain of 2 000 proteins and
20 000 proteins with planted families."""

import ctypes as C
import math
import os

import numpy as np
import pytest

import all_sim_filter_rule as rule
import cluster_rule as crule
import golden_util as gu
import tree_rule as trule

pytestmark = pytest.mark.gpu
NPZ = os.path.join(gu.GOLD, 'all_sim', 'all-dct.npz')
NONE = np.uint64(0xffffffffffffffff)


def _load(path):
    with np.load(path) as data:
        return [str(s) for s in data['sid']], np.asarray(data['idx'], dtype=np.int64), data['dct']


@pytest.fixture(scope='module')
def golden():
    sid, idx, dct = _load(NPZ)
    return sid, idx, dct, rule.triangle_l1(dct, idx)


def _same_edges(got, want):
    return all(g.dtype == np.int64 and np.array_equal(g, w) for g, w in zip(got, want)) and len(got) == 3


# ---- 1. the reference golden

@pytest.mark.parametrize('score,cut', [('domain', None), ('domain', 0.5), ('global', None), ('global', 0.9)])
def test_reference_golden(tmp_path, golden, score, cut):
    from dctdomain_amd import dct_sim
    sid, idx, dct, tri = golden
    bound = trule.DEFAULT_BOUND if cut is None else dct_sim.sim_bound(cut)
    want = trule.edges(dct, idx, score, bound, triangle=tri)
    tree = dct_sim.Tree(sid, idx, dct, score=score, min_cut=cut)
    assert _same_edges(tree.edges(), want)
    assert 1 <= tree.rounds <= math.ceil(math.log2(139)) + 1
    out = str(tmp_path / 'out.txt')
    argv = ['--dct', NPZ, '--output', out, '--tree'] + ([score] if score != 'domain' or cut is not None else [])
    if cut is not None:
        argv += ['--min-' + score, str(cut)]
    dct_sim.main(argv)
    text = open(out, 'rb').read()
    assert text == trule.HEADER + trule.text(sid, dct, idx, want[0], want[1])
    # a subset of the plain all-against-all's lines
    lines = set(rule.read_lines(os.path.join(gu.GOLD, 'all_sim', 'expected.txt.gz'))[1:])
    assert set(text.split(b'\n')[1:-1]) <= lines and len(text.split(b'\n')) - 2 == len(want[0])


# ---- 2. tri_nearest against numpy on hand-made tiles

def _np_best(t, row0, col0, bound, comp, row_empty=None, col_empty=None, cap=17000):
    """best (uint64, n) after one call on a fresh state: per label the smallest packed edge among the surviving entries whose
    ends carry different labels, each counted for both labels."""
    key = np.minimum(t.astype(np.int64) & 0xffffffff, cap)    # (a negative value counts as cap)
    if row_empty is not None:
        key[np.asarray(row_empty, dtype=bool)] = cap
    if col_empty is not None:
        key[:, np.asarray(col_empty, dtype=bool)] = cap
    i = row0 + np.arange(t.shape[0])[:, None]
    j = col0 + np.arange(t.shape[1])[None, :]
    r, c = np.nonzero((j > i) & (key <= bound))
    ei, ej, ek = row0 + r, col0 + c, key[r, c]
    out = comp[ei] != comp[ej]
    packed = (ek[out].astype(np.uint64) << np.uint64(48)) | (ei[out].astype(np.uint64) << np.uint64(24)) | ej[out].astype(np.uint64)
    best = np.full(len(comp), NONE, dtype=np.uint64)
    np.minimum.at(best, comp[ei[out]], packed)
    np.minimum.at(best, comp[ej[out]], packed)
    return best, int(out.sum())


def _labelling(rng, n, groups):
    """comp (int32, n): `groups` random groups, each labelled by its smallest member."""
    g = rng.integers(0, groups, size=n) if groups < n else np.arange(n)
    first = np.full(max(groups, n), n, dtype=np.int64)
    np.minimum.at(first, g, np.arange(n))
    return first[g].astype(np.int32)


@pytest.mark.parametrize('n_rows,n_cols', [(7, 3000), (1, 5000), (40, 1), (3, 1023), (5, 1025), (9, 2048), (300, 37), (64, 64)])
@pytest.mark.parametrize('bound,dense', [(0, False), (8500, False), (16999, True)])
def test_nearest_kernel_against_numpy(n_rows, n_cols, bound, dense):
    """`best` per label exactly: the bound exactly, entries left of the diagonal and beyond n_cols (the padding holds 0 = the
    lightest edge if it were read), views with ld > n_cols at each of the four 4-byte alignments, the flags, negative entries;
    labellings of 1, 2, about sqrt(n) and n components.  `dense`: nearly every entry survives, with many equal keys."""
    import torch
    from dctdomain_amd.similarity import TreeState, tri_nearest
    rng = np.random.default_rng(1000 * n_rows + n_cols + bound)
    places = [(10, 5), (n_rows + 3, 0), (0, n_rows + 20), (0, 1), (0, 0), (3, 0)]
    for k, (col0, row0) in enumerate(places):
        u = rng.random((n_rows, n_cols))
        if dense:
            t = rng.integers(0, 40, size=(n_rows, n_cols)).astype(np.int32) * 400      # keys 0 .. 15 600 in steps: ties everywhere
            t[u < 0.05] = 17000
        else:
            t = np.full((n_rows, n_cols), bound + 1, dtype=np.int32)
            t[u < 0.4] = 17000
            t[u > 1 - 3.0 / max(n_cols, 2)] = bound            # (sparse: about three edges per row)
            t[(u > 0.5) & (u < 0.5 + 1.0 / max(n_cols, 2))] = bound // 2
        t[u < 0.02] = -5
        pad, shift = int(rng.integers(1, 9)), k % 4
        big = torch.zeros((n_rows, n_cols + pad + shift), dtype=torch.int32, device='cuda')
        view = big[:, shift:shift + n_cols]
        view.copy_(torch.as_tensor(t, device='cuda'))
        assert (n_rows == 1 or view.stride(0) > n_cols) and (view.data_ptr() - big.data_ptr()) == 4 * shift
        flags = [(None, None), (rng.random(n_rows) < 0.3, None), (None, rng.random(n_cols) < 0.3),
                 (rng.random(n_rows) < 0.2, rng.random(n_cols) < 0.2)][(k + n_rows) % 4]
        n = max(row0 + n_rows, col0 + n_cols) + int(rng.integers(0, 3))
        comp = _labelling(rng, n, [1, 2, max(2, int(math.sqrt(n))), n][(k + n_cols) % 4])
        want, crossing = _np_best(t, row0, col0, bound, comp, *flags)
        ts = TreeState(n)
        ts.comp = torch.as_tensor(comp, device='cuda')
        tri_nearest(view, row0, col0, bound, ts, *flags)
        got = ts.best.cpu().numpy().view(np.uint64)
        assert np.array_equal(got, want), (col0, row0, int((got != want).sum()))
        # nothing left of the diagonal, nothing inside one component, every edge between the right labels
        for c in np.flatnonzero(got != NONE).tolist():
            i, j = int(got[c] >> np.uint64(24)) & 0xffffff, int(got[c]) & 0xffffff
            assert i < j and comp[i] != comp[j] and c in (comp[i], comp[j]) and comp[c] == c
        assert len(np.unique(comp)) > 1 or (got == NONE).all()
        # a second call lowers nothing further; the other arrays are untouched
        tri_nearest(view, row0, col0, bound, ts, *flags)
        assert np.array_equal(ts.best.cpu().numpy().view(np.uint64), want)
        assert ts.parent.cpu().tolist() == list(range(n)) and int(ts.counter.item()) == 0
    assert (big.cpu().numpy()[:, shift + n_cols:] == 0).all()


# ---- 3. ties

def _boruvka(tile, n, bound, flags=(None, None)):
    """Rounds of tri_nearest / tree_hook / cluster_labels on one tile: (state, rounds run)."""
    from dctdomain_amd.similarity import TreeState, cluster_labels, tree_hook, tri_nearest
    ts = TreeState(n)
    rounds = done = 0
    while True:
        tri_nearest(tile, 0, 0, bound, ts, *flags)
        tree_hook(ts)
        rounds += 1
        total = int(ts.counter.item())
        if total == done:
            return ts, rounds
        done = total
        ts.comp = cluster_labels(ts.parent)
        assert rounds <= math.ceil(math.log2(max(n, 2))) + 1


def _sorted(i, j, key):
    order = np.lexsort((j, i, key))
    return i[order], j[order], key[order]


@pytest.mark.parametrize('n', [2, 65, 1500])
def test_a_tile_of_equal_entries_gives_the_star_on_node_0(n):
    import torch
    bound = 8500
    tile = torch.full((n, n), bound, dtype=torch.int32, device='cuda')
    ts, rounds = _boruvka(tile, n, bound)
    i, j, key = _sorted(*ts.edges())
    assert i.tolist() == [0] * (n - 1) and j.tolist() == list(range(1, n)) and key.tolist() == [bound] * (n - 1)
    assert rounds == 2 and int(ts.counter.item()) == n - 1     # (every node's lightest edge leads to 0; then one round finds nothing)
    assert (ts.best.cpu().numpy() == -1).all()
    ts, _ = _boruvka(tile, n, bound - 1)
    assert int(ts.counter.item()) == 0 and ts.parent.cpu().tolist() == list(range(n))


def _thermometer(levels):
    """One int8 fingerprint per level: L1 between two of them = the difference of their levels (a path through the 480
    coordinates, 250 units along each)."""
    lv = np.asarray(levels, dtype=np.int64)[:, None]
    return (np.clip(lv - 250 * np.arange(480)[None, :], 0, 250) - 125).astype(np.int8)


@pytest.mark.parametrize('score', ['domain', 'global'])
def test_equally_spaced_proteins_give_the_path_in_index_order(score):
    from dctdomain_amd import dct_sim
    n = 300
    dct = _thermometer(7 * np.arange(n))
    tree = dct_sim.Tree([f'p{k}' for k in range(n)], np.arange(n + 1), dct, score=score)
    i, j, key = tree.edges()
    assert i.tolist() == list(range(n - 1)) and j.tolist() == list(range(1, n)) and key.tolist() == [7] * (n - 1)
    assert tree.rounds <= math.ceil(math.log2(n)) + 1


# ---- 4. tree_hook on a hand-made round

def _pack(key, i, j):
    return (key << 48) | (i << 24) | j


def test_hook_appends_once_joins_resets_and_stays_inside_its_slots():
    import torch
    from dctdomain_amd.similarity import TreeState, cluster_labels, tree_hook
    comp = [0, 0, 2, 2, 4, 5, 5, 5, 8, 9]
    best = [-1] * 10
    best[0] = best[2] = _pack(5, 1, 2)                         # chosen from both sides: once
    best[4] = _pack(9, 4, 6)                                   # 4 -> {5, 6, 7}
    best[5] = best[8] = _pack(3, 5, 8)                         # both sides again
    best[1] = _pack(0, 0, 9)                                   # not a label's entry: never read
    best[3] = _pack(1, 2, 3)
    want_edges = {(1, 2, 5), (4, 6, 9), (5, 8, 3)}
    want_labels = [0, 0, 0, 0, 4, 4, 4, 4, 4, 9]
    for max_edges in (9, 3, 2, 0):
        ts = TreeState(10, max_edges=0)
        room = torch.full((3, 12), -7, dtype=torch.int32, device='cuda')
        ts.edge_i, ts.edge_j, ts.edge_key = (room[k, :max_edges] for k in range(3))
        ts.comp = torch.tensor(comp, dtype=torch.int32, device='cuda')
        ts.parent = ts.comp.clone()                            # (the forest the labels came from: every node under its label)
        ts.best = torch.tensor(best, dtype=torch.int64, device='cuda')
        tree_hook(ts)
        assert int(ts.counter.item()) == 3                     # the counter = the edges chosen, whatever room there was
        got = room.cpu().numpy()
        written = min(3, max_edges)
        assert (got[:, written:] == -7).all()                  # nothing at or beyond max_edges
        assert {tuple(int(v) for v in got[:, k]) for k in range(written)} <= want_edges and len({tuple(got[:, k]) for k in range(written)}) == written
        assert (ts.best.cpu().numpy() == -1).all()             # reset, the entries no label owns too
        p = ts.parent.cpu().numpy()
        assert (p <= np.arange(10)).all() and (p >= 0).all()
        assert cluster_labels(ts.parent).cpu().tolist() == want_labels
        assert len(ts.edges()[0]) == written
    # a second hook on the reset state appends nothing
    tree_hook(ts)
    assert int(ts.counter.item()) == 3 and cluster_labels(ts.parent).cpu().tolist() == want_labels
    # entries that name no edge of their label are skipped: i >= j, j outside the nodes, both ends inside, neither end inside
    ts = TreeState(10)
    ts.comp = torch.tensor(comp, dtype=torch.int32, device='cuda')
    ts.best = torch.tensor([_pack(1, 3, 3), -1, _pack(1, 2, 10), -1, _pack(1, 5, 6), _pack(1, 5, 6), -1, -1, _pack(2, 0, 9), -1],
                           dtype=torch.int64, device='cuda')
    tree_hook(ts)
    assert int(ts.counter.item()) == 0 and ts.parent.cpu().tolist() == list(range(10))


# ---- 5. the cut property end to end, on random ragged files

_ALPHABET = list('abcdefghijklmnopqrstuvwxyz0123456789_|.-') + ['é', 'ß', 'α', '蛋', '😀']


def _ragged(seed, n):
    """Proteins of 0-3 fingerprints (15 % empty) from four families at L1 ~ 6 500 (0.62) within a family, plus planted near
    copies (+-2) of single fingerprints at random places of other proteins (test_cluster_gpu.py's files)."""
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


@pytest.mark.parametrize('score', ['domain', 'global'])
@pytest.mark.parametrize('seed,n', [(1, 60), (2, 150), (3, 2), (4, 300)])
def test_cut_at_any_cut_off_the_tree_gives_the_clusters(seed, n, score):
    """Every value _RAGGED_CUTS holds for the score (a tree orders the pairs by one score: a pair of cut-offs gives its value for
    that score), against dct_sim.Clusters at that cut-off alone; the edges against the oracle's."""
    from dctdomain_amd import dct_sim
    sid, idx, dct = _ragged(seed, n)
    assert (np.diff(idx) == 0).any() or n < 10
    tree = dct_sim.Tree(sid, idx, dct, score=score)
    want = trule.edges(dct, idx, score)
    assert _same_edges(tree.edges(), want)
    empty = np.flatnonzero(np.diff(idx) == 0)
    assert not np.isin(tree.edges()[0], empty).any() and not np.isin(tree.edges()[1], empty).any()
    seen = set()
    for x in sorted({pair[0 if score == 'domain' else 1] for pair in _RAGGED_CUTS} - {None}):
        assert dct_sim.sim_bound(x) <= tree.bound
        clusters = dct_sim.Clusters(sid, idx, dct, **{'min_' + score: x}).labels()
        got = tree.labels(x)
        assert got.dtype == np.int32 and np.array_equal(got, clusters), x
        assert np.array_equal(trule.cut(n, *want, dct_sim.sim_bound(x)), clusters)
        # built with that cut-off: the tree's edges up to it, n - clusters of them
        part = dct_sim.Tree(sid, idx, dct, score=score, min_cut=x).edges()
        keep = want[2] <= dct_sim.sim_bound(x)
        assert _same_edges(part, tuple(w[keep] for w in want)) and len(part[0]) == n - len(np.unique(clusters))
        seen.add(len(np.unique(clusters)))
    assert n < 10 or len(seen) > 1                            # (the score's cut-offs fall inside and outside the families)


# ---- 6. independence from the partition

@pytest.mark.parametrize('score,cut', [('domain', None), ('global', 0.62)])
def test_edges_and_text_do_not_depend_on_stripes_groups_or_ranges(monkeypatch, score, cut):
    from dctdomain_amd import dct_sim
    sid, idx, dct = _ragged(7, 90)
    bound = trule.DEFAULT_BOUND if cut is None else dct_sim.sim_bound(cut)
    want = trule.edges(dct, idx, score, bound)
    want_text = trule.text(sid, dct, idx, want[0], want[1])
    assert 10 < len(want[0]) < 89
    first = dct_sim.Tree(sid, idx, dct, score=score, min_cut=cut)
    assert len(list(first.stripes())) == 1 and _same_edges(first.edges(), want)                # (the kept-tile route)
    for tile_ints, col_rows, text_bytes in [(5, 3, 41), (1, 1, 1), (300, 3, 281), (1 << 28, 2, 1 << 28)]:
        for name, v in (('TILE_INTS', tile_ints), ('COL_ROWS', col_rows), ('TEXT_BYTES', text_bytes)):
            monkeypatch.setattr(dct_sim.FilteredPairs, name, v)
        tree = dct_sim.Tree(sid, idx, dct, score=score, min_cut=cut)
        stripes = list(tree.stripes())
        assert len(stripes) > 1 and (tile_ints > 1 or all(b - a == 1 for a, b in stripes))      # (recomputed tiles; one-row stripes among them)
        assert _same_edges(tree.edges(), want), (tile_ints, col_rows, text_bytes)
        assert tree.rounds <= math.ceil(math.log2(90)) + 1
        got = []
        tree.write(lambda mv: got.append(bytes(mv)))
        assert b''.join(got) == want_text
        assert text_bytes > 1 or len(got) == len(want[0])      # (one line per range)


# ---- 7. a shuffled chain

def test_a_shuffled_chain_of_two_thousand_proteins(tmp_path):
    from dctdomain_amd import dct_sim
    n = 2000
    place = np.random.default_rng(17).permutation(n)          # chain position of the protein at each file index
    dct = _thermometer(5 * place)                             # neighbours at L1 5, the next ones at 10
    sid = [f'chain{k:04d}' for k in range(n)]
    where = np.argsort(place)                                 # file index of the protein at each chain position
    a, b = np.minimum(where[:-1], where[1:]), np.maximum(where[:-1], where[1:])
    order = np.lexsort((b, a))
    tree = dct_sim.Tree(sid, np.arange(n + 1), dct)
    i, j, key = tree.edges()
    assert len(i) == n - 1 and np.array_equal(i, a[order]) and np.array_equal(j, b[order]) and (key == 5).all()
    print(f'\ntree of a shuffled chain of {n}: {tree.rounds} rounds')
    assert tree.rounds <= math.ceil(math.log2(n)) + 1
    assert not tree.labels(0.9995).any() and dct_sim.sim_bound(0.9995) == 8
    path, out = str(tmp_path / 'chain-dct.npz'), str(tmp_path / 'out.txt')
    np.savez(path, sid=np.array(sid), idx=np.arange(n + 1, dtype=np.int64), dom=np.array(['1-9'] * n), dct=dct)
    dct_sim.main(['--dct', path, '--output', out, '--tree', '--min-domain', '0.9995'])
    lines = open(out, 'rb').read().split(b'\n')
    assert lines[0] + b'\n' == trule.HEADER and lines[-1] == b'' and len(lines) == n + 1
    assert lines[1:-1] == [f'{sid[x]} {sid[y]} 1.000 1.000'.encode() for x, y in zip(i.tolist(), j.tolist())]


# ---- 8. planted families

def test_twenty_thousand_proteins_with_planted_families(tmp_path):
    """test_cluster_gpu.py's construction at a tenth of its size: synth's random proteins lie at L1 15 500 +- 500 from each other,
    far above --min-domain 0.5's bound of 8 500 -- a condition on the input, asserted below on a sample --, members of a family
    within 1 920 of each other.  So the forest at 0.5 has a tree per family: n - clusters edges, all inside families."""
    from dctdomain_amd import dct_sim
    from tools.all_sim_bench import synth
    n, n_fam = 20000, 300
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
    tree = dct_sim.Tree(sid, idx, dct, min_cut=0.5)
    i, j, key = tree.edges()
    clusters = n - int(sizes.sum()) + n_fam
    assert len(i) == n - clusters and (want[i] == want[j]).all() and key.max() <= 1920
    assert np.array_equal(crule.components(n, i, j), want)
    assert np.array_equal(np.lexsort((j, i, key)), np.arange(len(i)))
    assert len(list(tree.stripes())) > 1 and tree.rounds <= math.ceil(math.log2(n)) + 1        # (the recomputed-tiles route)
    assert np.array_equal(tree.labels(0.5), want) and np.array_equal(tree.labels(1.5), np.arange(n))


# ---- 9. bad arguments and empty calls

def test_tree_calls_reject_bad_arguments_and_take_empty_ones():
    import torch
    from dctdomain_amd import _lib
    from dctdomain_amd.similarity import TreeState, tree_hook, tri_nearest
    t = torch.zeros((6, 100), dtype=torch.int32, device='cuda')
    ts = TreeState(100)
    ctx = _lib.get_context(0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda row0=0, col0=0, bound=0, ld=100, n_nodes=100, n_rows=6, cap=17000, best=ts.best.data_ptr(): ctx._lib.dctfp_tri_nearest(   # noqa: E731
        ctx.handle, t.data_ptr(), n_rows, 100, ld, row0, col0, None, None, cap, bound, ts.comp.data_ptr(), best, n_nodes, stream)
    hook = lambda n_nodes=100, max_edges=99, best=ts.best.data_ptr(), edges=ts.edge_i.data_ptr(): ctx._lib.dctfp_tree_hook(               # noqa: E731
        ctx.handle, ts.comp.data_ptr(), best, ts.parent.data_ptr(), n_nodes, edges, ts.edge_j.data_ptr(), ts.edge_key.data_ptr(),
        ts.counter.data_ptr(), max_edges, stream)
    assert call(col0=1) == _lib.DCTFP_ERR_INVALID and call(row0=95) == _lib.DCTFP_ERR_INVALID      # outside the nodes: on the host
    assert call(bound=17001) == _lib.DCTFP_ERR_INVALID and call(bound=-2) == _lib.DCTFP_ERR_INVALID and call(ld=99) == _lib.DCTFP_ERR_INVALID
    assert call(best=ts.best.data_ptr() + 4) == _lib.DCTFP_ERR_INVALID and call(best=None) == _lib.DCTFP_ERR_INVALID
    assert call(n_nodes=2 ** 24 + 1) == _lib.DCTFP_ERR_LIMIT and call(cap=40000, bound=40000) == _lib.DCTFP_ERR_LIMIT
    assert hook(n_nodes=2 ** 24 + 1) == _lib.DCTFP_ERR_LIMIT and hook(n_nodes=-1) == _lib.DCTFP_ERR_INVALID
    assert hook(max_edges=-1) == _lib.DCTFP_ERR_INVALID and hook(edges=None) == _lib.DCTFP_ERR_INVALID
    assert hook(best=ts.best.data_ptr() + 4) == _lib.DCTFP_ERR_INVALID
    assert call(n_rows=0) == 0 and hook(n_nodes=0) == 0

    def untouched():
        return (ts.best.cpu().numpy() == -1).all() and ts.parent.cpu().tolist() == list(range(100)) and int(ts.counter.item()) == 0
    assert untouched()                                         # nothing was written by any of these
    with pytest.raises(IndexError):
        tri_nearest(t, 0, 1, 0, ts)
    ts.best = ts.best.int()
    with pytest.raises(ValueError):
        tri_nearest(t, 0, 0, 0, ts)
    with pytest.raises(ValueError):
        tree_hook(ts)
    ts.best = ts.best.long()
    tree_hook(TreeState(0))
    assert call(bound=-1) == 0 and untouched()                 # bound -1: nothing survives
    assert call() == 0 and hook() == 0                         # every entry 0: each node's lightest edge leads to node 0, or from it to 1
    i, j, key = ts.edges()
    assert sorted(zip(i.tolist(), j.tolist())) == [(0, c) for c in range(1, 100)] and not key.any()
    assert int(ts.counter.item()) == 99 and (ts.best.cpu().numpy() == -1).all()
