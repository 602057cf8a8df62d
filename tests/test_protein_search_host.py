"""Host logic of the protein-level search (dct_sim.ProteinSearch): the threshold -> integer L1 bound, the merge of the
database groups' hit lists, the pair chunking of pair_sim.  No GPU."""

import numpy as np
import pytest

from dctdomain_amd import dct_sim


def _reference_keeps(l1: int, threshold: float) -> bool:
    """src/dct-sim.py:24-26 + :151: a hit past the first `top` stays unless its similarity is below the threshold."""
    d = np.int64(l1) / 17000
    s = 1 - min(d, 1)
    return not (s < threshold)


@pytest.mark.parametrize('threshold', [0.25, 0.0, -0.5, 1.0, 1.5, 0.5, 0.1, 0.9999, 1e-12, float('nan'),
                                       1 - 12750 / 17000, 1 - 4321 / 17000, 1 - 16999 / 17000, 1 - 1 / 17000,
                                       np.nextafter(0.25, 1), np.nextafter(0.25, 0), np.nextafter(1 - 4321 / 17000, 1),
                                       np.nextafter(1 - 4321 / 17000, 0)])
def test_sim_bound_matches_reference_expression_on_every_l1(threshold):
    bound = dct_sim.sim_bound(threshold)
    keep = np.array([_reference_keeps(l1, threshold) for l1 in range(17002)])
    assert keep.tolist() == [min(l1, 17000) <= bound for l1 in range(17002)]


def test_sim_bound_edges():
    assert dct_sim.sim_bound(0.25) == 12750
    assert dct_sim.sim_bound(0) == dct_sim.sim_bound(-3) == 17000        # every column
    assert dct_sim.sim_bound(1.5) == -1                                   # top only
    assert dct_sim.sim_bound(1.0) == 0


def _first(keys, cols, top, bound):
    order = np.lexsort((cols, keys))
    m = min(len(order), max(top, int(np.count_nonzero(keys <= bound))))
    return keys[order[:m]], cols[order[:m]]


@pytest.mark.parametrize('seed', range(6))
def test_merge_candidates_equals_whole_row_selection(seed):
    rng = np.random.default_rng(seed)
    for _ in range(40):
        n = int(rng.integers(1, 300))
        keys = np.minimum(rng.integers(0, 17400, size=n), 17000)
        keys[rng.random(n) < 0.3] = 17000                                 # many ties at similarity 0
        keys[rng.random(n) < 0.1] = int(rng.integers(0, 17000))           # and elsewhere
        cols = np.arange(n)
        top = int(rng.choice([1, 5, 50, 2000]))
        bound = int(rng.choice([-1, 0, 5000, 12750, 17000]))
        cuts = np.sort(rng.choice(np.arange(1, n), size=min(n - 1, int(rng.integers(0, 5))), replace=False)) if n > 1 else []
        edges = [0, *cuts, n]
        parts = [_first(keys[a:b], cols[a:b], top, bound) for a, b in zip(edges[:-1], edges[1:])]
        got_k, got_c = dct_sim.merge_candidates(parts, top, bound)
        exp_k, exp_c = _first(keys, cols, top, bound)
        np.testing.assert_array_equal(got_c, exp_c)
        np.testing.assert_array_equal(got_k, exp_k)


def test_pair_chunks_cover_pairs_within_the_row_budget():
    rng = np.random.default_rng(3)
    sizes = rng.integers(0, 7, size=50)
    idx = np.concatenate([[0], np.cumsum(sizes)])
    pairs = rng.integers(0, 50, size=(400, 2))
    chunks = list(dct_sim._pair_chunks(idx, pairs, 20))
    assert chunks[0][0] == 0 and chunks[-1][1] == len(pairs)
    assert all(a < b for a, b in chunks) and all(b == c for (_, b), (c, _) in zip(chunks[:-1], chunks[1:]))
    for a, b in chunks:
        rows = sizes[np.unique(pairs[a:b])].sum()
        assert rows <= 20 or b - a == 1


def test_compact_gathers_the_named_proteins():
    rng = np.random.default_rng(4)
    sizes = rng.integers(0, 5, size=30)
    idx = np.concatenate([[0], np.cumsum(sizes)])
    fps = rng.integers(-128, 128, size=(idx[-1], 8)).astype(np.int8)
    proteins = np.array([2, 5, 6, 17, 29])
    rows, sub = dct_sim._compact(fps, idx, proteins)
    exp = np.concatenate([fps[idx[p]:idx[p + 1]] for p in proteins])
    np.testing.assert_array_equal(rows, exp)
    np.testing.assert_array_equal(np.diff(sub), sizes[proteins])


def test_last_rows_flag_proteins_without_fingerprints():
    idx = np.array([0, 2, 2, 5, 5])
    fps = np.arange(5 * 3, dtype=np.int8).reshape(5, 3)
    last, empty = dct_sim._last_rows(fps, idx)
    assert empty.tolist() == [0, 1, 0, 1]
    np.testing.assert_array_equal(last[[0, 2]], fps[[1, 4]])
    assert not last[[1, 3]].any()
