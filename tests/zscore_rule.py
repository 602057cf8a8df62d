"""The rule of dct-sim --db --zscore, restated in plain numpy / Python: the oracle of test_zscore_host.py (where it is pinned on
hand-computed cases) and test_zscore_gpu.py.

A query protein a, a database of proteins b, one score: L1(a, b) = the smallest L1 over all fingerprint pairs of the two ('domain')
or the L1 of their two last fingerprints ('global') -- rbh_rule.protein_l1, NONE where a protein has no fingerprint.

The background of a is every b for which an L1 exists; the L1 is raw, NOT capped at 17000; the query counts like any other protein
if it is in the database.  n = the size of the background, S1 = the sum of its L1s, S2 = the sum of their squares: exact integers.
A hit with L1 = d has z = (S1 - n d) / sqrt(n S2 - S1^2) = (mean - d) / sigma with the population sigma: numerator and radicand
exact Python integers, math.sqrt of the radicand, one true division.  z is undefined for n < 2, for a radicand of 0, and for a hit
pair without an L1.  Its text is f'{z:.2f}', '-' where undefined."""

import math

import numpy as np

import rbh_rule as rrule

NONE = rrule.NONE


def moments(l1s):
    """(n, S1, S2) of a background given as its L1s -- Python integers, NONE entries (no L1) left out."""
    vals = [int(v) for v in l1s if int(v) != NONE]
    return len(vals), sum(vals), sum(v * v for v in vals)


def zscore(n, s1, s2, d):
    """z of a hit with L1 ``d`` (None or NONE: the pair has no L1) in the background (n, S1, S2); None where undefined."""
    if d is None or int(d) == NONE:
        return None
    n, s1, s2, d = int(n), int(s1), int(s2), int(d)
    radicand = n * s2 - s1 * s1
    if n < 2 or radicand == 0:
        return None
    return (s1 - n * d) / math.sqrt(radicand)


def text(z) -> str:
    return '-' if z is None else f'{z:.2f}'


def tile_moments(t, row0, col0, n_a, n_b, limit, row_empty=None, col_empty=None):
    """(row_mom, col_mom): uint64 (3, n_a) and (3, n_b), what dctfp_rect_moments adds to zeroed arrays for the int32 tile ``t`` at
    (row0, col0) -- an entry counts unless its row or column is flagged or its value, as an unsigned 32-bit number, is >= limit.
    Sums of squares are taken modulo 2^64 as the device words are (they never wrap within the export's limits)."""
    x = np.asarray(t).astype(np.int64) & 0xffffffff
    counts = x < limit
    if row_empty is not None:
        counts[np.asarray(row_empty, dtype=bool)] = False
    if col_empty is not None:
        counts[:, np.asarray(col_empty, dtype=bool)] = False
    v = np.where(counts, x, 0).astype(np.uint64)
    row_mom, col_mom = np.zeros((3, n_a), dtype=np.uint64), np.zeros((3, n_b), dtype=np.uint64)
    for k, plane in enumerate((counts.astype(np.uint64), v, v * v)):
        row_mom[k, row0:row0 + x.shape[0]] = plane.sum(axis=1, dtype=np.uint64)
        col_mom[k, col0:col0 + x.shape[1]] = plane.sum(axis=0, dtype=np.uint64)
    return row_mom, col_mom


def backgrounds(l1):
    """([(n, S1, S2)] per row of the protein L1 matrix ``l1``, the same per column)."""
    l1 = np.asarray(l1, dtype=np.int64)
    return [moments(row) for row in l1], [moments(col) for col in l1.T]


def search_z(l1, hits):
    """Per query (row of ``l1``) the list of z of its hits (``hits[q]`` = database indices): None where undefined."""
    rows, _ = backgrounds(l1)
    return [[zscore(*rows[q], l1[q, b]) for b in np.asarray(cols).tolist()] for q, cols in enumerate(hits)]
