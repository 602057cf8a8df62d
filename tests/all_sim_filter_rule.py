"""The rule of dct-sim's all-against-all cut-offs (--min-domain / --min-global), stated in numpy: the oracle of
test_all_sim_filter_host.py (where it is pinned on the committed reference golden) and test_all_sim_filter_gpu.py.

A pair is printed unless ``sim < cut-off`` -- the reference's own comparison (src/dct-sim.py:148) -- with
sim = 1 - min(L1 / 17000, 1) in float64 (src/dct-sim.py:24-26), for DCTdomain on the smallest L1 over all fingerprint pairs of
the two proteins and for DCTglobal on the L1 of their last fingerprints.  A protein without fingerprints has no L1 against
anything: 0x7fffffff, similarity 0."""

import gzip

import numpy as np

NO_L1 = 0x7fffffff


def pair_l1(dct, idx, i, j):
    """(min, last) L1 of the protein pairs (i[k], j[k]), int64."""
    dct = np.asarray(dct, dtype=np.int64)
    idx = np.asarray(idx, dtype=np.int64)
    mn = np.full(len(i), NO_L1, dtype=np.int64)
    last = mn.copy()
    for k, (p, q) in enumerate(zip(i, j)):
        a, b = dct[idx[p]:idx[p + 1]], dct[idx[q]:idx[q + 1]]
        if len(a) and len(b):
            d = np.abs(a[:, None, :] - b[None, :, :]).sum(axis=2)
            mn[k], last[k] = d.min(), d[-1, -1]
    return mn, last


def triangle_l1(dct, idx):
    """(i, j, min, last) over the upper triangle in output order (i ascending, then j)."""
    n = len(idx) - 1
    i, j = np.triu_indices(n, 1)
    return (i, j) + pair_l1(dct, idx, i, j)


def similarity(l1):
    return 1 - np.minimum(np.asarray(l1, dtype=np.int64) / 17000, 1)


def kept(mn, last, min_domain=None, min_global=None):
    """Boolean mask of the pairs that are printed."""
    keep = np.ones(len(mn), dtype=bool)
    if min_domain is not None:
        keep &= ~(similarity(mn) < min_domain)
    if min_global is not None:
        keep &= ~(similarity(last) < min_global)
    return keep


def filtered_text(lines, keep) -> bytes:
    """``lines`` = the unfiltered output split at newlines (header first, pair k on line 1 + k): the header and the kept lines."""
    return b''.join(x + b'\n' for x in [lines[0]] + [lines[1 + k] for k in np.flatnonzero(keep)])


def read_lines(path):
    with (gzip.open(path, 'rb') if path.endswith('.gz') else open(path, 'rb')) as fh:
        return fh.read().split(b'\n')[:-1]


# ---- the rule on one int32 tile of L1 values, as the kernels that scan a tile apply it (test_all_sim_filter_gpu.py, test_tri_walk_gpu.py)

def tile_keep(t, row0, col0, bound, row_empty=None, col_empty=None, cap=17000):
    """(keep, key): entry (r, c) of the tile stands for proteins i = row0 + r and j = col0 + c; key = min(L1, cap), cap for a row or
    column flagged empty; an entry is kept when j > i and key <= bound."""
    key = np.minimum(t.astype(np.int64) & 0xffffffff, cap)    # (a negative value counts as cap)
    if row_empty is not None:
        key[np.asarray(row_empty, dtype=bool)] = cap
    if col_empty is not None:
        key[:, np.asarray(col_empty, dtype=bool)] = cap
    i = row0 + np.arange(t.shape[0])[:, None]
    j = col0 + np.arange(t.shape[1])[None, :]
    return (j > i) & (key <= bound), key


def tile_filter(t, row0, col0, bound, row_empty=None, col_empty=None, cap=17000):
    """(count per row, i, j) of the kept entries."""
    keep, _ = tile_keep(t, row0, col0, bound, row_empty, col_empty, cap)
    r, c = np.nonzero(keep)                                   # (row-major: i ascending, then j)
    return keep.sum(axis=1), row0 + r, col0 + c


def random_tile(rng, n_rows, n_cols, bound):
    """Values on both sides of the bound and of 17000, 0x7fffffff and negative ones."""
    t = rng.integers(0, 17002, size=(n_rows, n_cols))
    near = rng.random((n_rows, n_cols))
    t[near < 0.2] = max(bound, 0)
    t[(near >= 0.2) & (near < 0.3)] = bound + 1
    t[(near >= 0.3) & (near < 0.4)] = 0x7fffffff
    t[(near >= 0.4) & (near < 0.45)] = 17000
    t[(near >= 0.45) & (near < 0.47)] = -5
    return t.astype(np.int32)
