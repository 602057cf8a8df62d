"""The rule of dct-sim --db --rbh, stated in numpy by brute force over all fingerprint pairs: the oracle of test_rbh_host.py (where
it is pinned on the reference's db_search text of the committed golden) and test_rbh_gpu.py.

A = the proteins of --dct, B = those of --db.  key(a, b) = min(L1(a, b), 17000), L1 = the smallest L1 over all fingerprint pairs of
the two proteins (score 'domain') or the L1 of their two last fingerprints (score 'global'); a protein without fingerprints has key
17000 against everything.  A pair is a hit when key <= bound (16999: similarity above 0).  best_b(a) = the hit of a smallest under
the strict order (key, b), best_a(b) the same under (key, a).  (a, b) is printed iff best_b(a) == b and best_a(b) == a, as db_search
prints a hit -- "{id a} {id b} {DCTdomain} {DCTglobal}" -- in ascending order of a."""

import gzip
import json
import os

import numpy as np

import golden_util as gu

HEADER = '#prot1 prot2 sim-domain sim-global'
CAP = 17000
DEFAULT_BOUND = CAP - 1                                        # every pair of similarity above 0
NONE = 0x7fffffff                                              # the L1 of a pair with a protein that has no fingerprint


def row_l1(a, b):
    """int64 (rows of a, rows of b): the L1 of every fingerprint pair."""
    a, b = np.asarray(a, dtype=np.int16), np.asarray(b, dtype=np.int16)
    out = np.zeros((len(a), len(b)), dtype=np.int64)
    for r in range(len(a)):
        out[r] = np.abs(b - a[r]).sum(axis=1, dtype=np.int64)
    return out


def protein_l1(a, ia, b, ib, score, dist=None):
    """int64 (n_a, n_b): the L1 of every protein pair under ``score``, NONE where a protein has no fingerprint."""
    ia, ib = np.asarray(ia, dtype=np.int64), np.asarray(ib, dtype=np.int64)
    dist = row_l1(a, b) if dist is None else dist
    out = np.full((len(ia) - 1, len(ib) - 1), NONE, dtype=np.int64)
    for p in range(len(ia) - 1):
        for q in range(len(ib) - 1):
            block = dist[ia[p]:ia[p + 1], ib[q]:ib[q + 1]]
            if block.size:
                out[p, q] = block.min() if score == 'domain' else block[-1, -1]
    return out


def keys(a, ia, b, ib, score):
    """int64 (n_a, n_b): key of every protein pair."""
    return np.minimum(protein_l1(a, ia, b, ib, score), CAP)


def _side(k, bound):
    """(index, key) of the best hit of every row of ``k``: the lowest column among the smallest keys <= bound, -1 in both for none."""
    if k.shape[1] == 0:
        none = np.full(k.shape[0], -1, dtype=np.int64)
        return none, none.copy()
    masked = np.where(k <= bound, k, NONE)
    col = masked.argmin(axis=1)                                # (the first of equal minima: the lowest index)
    val = masked[np.arange(len(col)), col]
    hit = val != NONE
    return np.where(hit, col, -1), np.where(hit, val, -1)


def best(k, bound=DEFAULT_BOUND):
    """((best_b, its key) per protein of A, (best_a, its key) per protein of B), -1 in both where a protein has no hit."""
    k = np.asarray(k, dtype=np.int64)
    return _side(k, bound), _side(k.T, bound)


def pairs(k, bound=DEFAULT_BOUND):
    """(a, b, key) of the reciprocal best hits, a ascending."""
    (best_b, key), (best_a, _) = best(k, bound)
    a = np.array([x for x in range(len(best_b)) if best_b[x] >= 0 and best_a[best_b[x]] == x], dtype=np.int64)
    return a, best_b[a], key[a]


def _score(l1):
    """1 - min(L1 / 17000, 1) with the reference's scalar arithmetic: the int 1 once L1 exceeds 17000."""
    return 1 - min(int(l1) / CAP, 1)


def text(sid_a, a, ia, sid_b, b, ib, score, bound=DEFAULT_BOUND, domains=False, labels=None, db_labels=None):
    """The result lines (a list of str, without the header).  ``domains``: two more fields, the fingerprint pair DCTdomain came from
    -- the smallest L1, ties to the lowest row of a, then of b; 1-based indices within the proteins unless ``labels`` / ``db_labels``
    (one name per fingerprint row) are given; "-" in both when no pair scores above 0."""
    ia, ib = np.asarray(ia, dtype=np.int64), np.asarray(ib, dtype=np.int64)
    dist = row_l1(a, b)
    pa, pb, _ = pairs(np.minimum(protein_l1(a, ia, b, ib, score, dist), CAP), bound)
    out = []
    for p, q in zip(pa.tolist(), pb.tolist()):
        block = dist[ia[p]:ia[p + 1], ib[q]:ib[q + 1]]
        mn, last = int(block.min()), int(block[-1, -1])
        dom = _score(mn)
        line = f'{sid_a[p]} {sid_b[q]} {dom if dom > 0 else 0} {_score(last)}'
        if domains:
            ra, rb = np.unravel_index(int(block.argmin()), block.shape)       # (row-major: the lowest row of a, then of b)
            if mn >= CAP:
                line += ' - -'
            else:
                line += f' {labels[ia[p] + ra] if labels is not None else ra + 1} {db_labels[ib[q] + rb] if db_labels is not None else rb + 1}'
        out.append(line)
    return out


# ---- the committed golden of the reference's db_search (tests/golden/protein_search)

GOLD = os.path.join(gu.GOLD, 'protein_search')


def golden_files():
    """[(sid, idx, dct) of the query file, the same of the database file] of the committed protein_search golden."""
    out = []
    for name in ('query', 'db'):
        with np.load(os.path.join(GOLD, name + '-dct.npz')) as data:
            out.append(([str(s) for s in data['sid']], np.asarray(data['idx'], dtype=np.int64), data['dct']))
    return out


def reference_lines():
    """The reference's db_search lines (top 5, threshold 0.25) of the golden, without the header."""
    with gzip.open(os.path.join(GOLD, 'expected.json.gz'), 'rt') as fh:
        runs = json.load(fh)['runs']
    run, = [r for r in runs if r['mode'] == 'db' and r['top'] == 5 and r['threshold'] == 0.25]
    lines = run['expected'].splitlines()
    assert lines[0] == HEADER
    return lines[1:]


def reference_rbh_lines():
    """(the reference's first line of every query, in query order; those of them the rule calls reciprocal)."""
    (sid, idx, dct), (db_sid, db_idx, db_dct) = golden_files()
    first = {}
    for line in reference_lines():
        first.setdefault(line.split()[0], line)
    a, _, _ = pairs(keys(dct, idx, db_dct, db_idx, 'global'))
    return first, [first[sid[x]] for x in a.tolist()]
