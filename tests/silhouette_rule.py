"""The rule of python -m dctdomain_amd.cluster_quality, stated in numpy and Python fractions: the oracle of test_silhouette_host.py
(where it is pinned on scikit-learn's silhouette_samples) and test_silhouette_gpu.py.

key(i, j) = min(L1(i, j), 17000), 17000 when either protein has no fingerprints; i == j never counts.  A clustering is one label per
protein.  For protein i of cluster A: Sa = the sum of key(i, j) over the other members of A, na = |A| - 1; for every other cluster B,
S(B) = the sum over its members, nb = |B|.  The neighbour cluster minimises S(B) / |B| as an exact fraction, ties to the cluster whose
first member comes first in the file.  s(i) = (Sb na - Sa nb) / max(Sa nb, Sb na): 0 when the maximum is 0, 0 for the member of a
singleton cluster, undefined for every protein when the file has fewer than two clusters."""

import math
from fractions import Fraction

import numpy as np

import all_sim_filter_rule as rule

CAP = 17000
PROTEIN_HEADER = b'#protein cluster size own other neighbour silhouette\n'
CLUSTER_HEADER = b'#cluster size mean_silhouette min_silhouette negative\n'


def key_matrices(dct, idx):
    """{'domain': .., 'global': ..}: int64 (n, n), the keys of a file under either score, the diagonal 0 (it never counts)."""
    n = len(idx) - 1
    keys = {'domain': np.zeros((n, n), dtype=np.int64), 'global': np.zeros((n, n), dtype=np.int64)}
    if n > 1:
        i, j, mn, last = rule.triangle_l1(dct, idx)
        for key, l1 in ((keys['domain'], mn), (keys['global'], last)):
            key[i, j] = key[j, i] = np.minimum(l1, CAP)
    return keys


def key_matrix(dct, idx, score):
    return key_matrices(dct, idx)[score]


def tile_keys(tile, row_empty=None, col_empty=None, cap=CAP):
    """The keys of an int32 tile as the tile scans form them: cap for a flagged row or column, a negative value or one >= cap."""
    return rule.tile_keep(tile, 0, 0, cap, row_empty, col_empty, cap)[1]


def dense(labels):
    """(cluster, first, size): the clusters numbered by their first member."""
    index, cluster, first = {}, [], []
    for i, label in enumerate(labels):
        if label not in index:
            index[label] = len(index)
            first.append(i)
        cluster.append(index[label])
    cluster = np.array(cluster, dtype=np.int64)
    return cluster, np.array(first, dtype=np.int64), np.bincount(cluster, minlength=len(first)) if len(first) else np.zeros(0, dtype=np.int64)


def kernel_arrays(labels):
    """(cid, size, first) as dctfp_silhouette_rows reads them: the clusters of two or more members numbered by first member, -1 for
    the member of a singleton."""
    cluster, first, size = dense(labels)
    multi = size >= 2
    ids = np.where(multi, np.cumsum(multi) - 1, -1)
    return ids[cluster].astype(np.int32), size[multi].astype(np.int32), first[multi].astype(np.int32)


def tile_sums(key, row0, col0, cid, size, first):
    """What the export writes for the rows of a tile of keys (``tile_keys``), taking ``cid`` / ``size`` / ``first`` at their word as it
    does: {global row index: (Sa, Sb, |B|, first of B)}, (.., 0, 0, -1) without another cluster.  Every multi-member cluster but the
    row's own is a candidate, also one without a column in the tile (sum 0); every singleton column j != i is the candidate
    (key, 1, j).  Python integers and fractions."""
    out = {}
    n_rows, n_cols = key.shape
    for r in range(n_rows):
        i = row0 + r
        total = [0] * len(size)
        lone = []
        for c in range(n_cols):
            j = col0 + c
            if j == i:
                continue
            if cid[j] >= 0:
                total[cid[j]] += int(key[r, c])
            else:
                lone.append((Fraction(int(key[r, c]), 1), j, int(key[r, c]), 1))
        own = int(cid[i])
        cands = lone + [(Fraction(total[g], int(size[g])), int(first[g]), total[g], int(size[g])) for g in range(len(size)) if g != own]
        best = min(cands, key=lambda t: (t[0], t[1])) if cands else None
        out[i] = (total[own] if own >= 0 else 0,) + ((best[2], best[3], best[1]) if best else (0, 0, -1))
    return out


def sums(key, labels):
    """(own_sum, near_sum, near_size, near_first), int64 (n), of a whole file from its key matrix."""
    n = len(labels)
    got = tile_sums(key, 0, 0, *kernel_arrays(labels)) if n else {}
    return tuple(np.array([got[i][k] for i in range(n)], dtype=np.int64) for k in range(4))


def values(four, labels):
    """float64 (n): the silhouettes, NaN everywhere with fewer than two clusters."""
    cluster, _first, size = dense(labels)
    if len(size) < 2:
        return np.full(len(labels), np.nan)
    out = []
    for i in range(len(labels)):
        na, sa, sb, nb = int(size[cluster[i]]) - 1, int(four[0][i]), int(four[1][i]), int(four[2][i])
        top = max(sa * nb, sb * na)
        out.append(0.0 if na == 0 or top == 0 else float(Fraction(sb * na - sa * nb, top)))
    return np.array(out, dtype=np.float64)


def _sim(total, count):
    return '-' if count == 0 else '%.4f' % (1 - int(total) / (int(count) * CAP))


def _fixed(v):
    return '-' if v is None or np.isnan(v) else '%.4f' % v


def last_line(four, labels):
    _cluster, _first, size = dense(labels)
    v = values(four, labels)
    ok = len(size) >= 2
    mean = _fixed(math.fsum(v) / len(v) if ok else None)
    return (f'# proteins={len(labels)} clusters={len(size)} singletons={int((size == 1).sum())} mean_silhouette={mean} '
            f'negative={int((v < 0).sum()) if ok else 0}\n').encode('utf8')


def text(sid, labels, four, per='protein'):
    """The result lines (without the header), the summary line last."""
    cluster, first, size = dense(labels)
    v = values(four, labels)
    ok = len(size) >= 2
    lines = []
    if per == 'protein':
        for i in range(len(labels)):
            sz, near = int(size[cluster[i]]), int(four[3][i])
            lines.append(f'{sid[i]} {labels[i]} {sz} {_sim(four[0][i], sz - 1)} {_sim(four[1][i], four[2][i] if near >= 0 else 0)} '
                         f'{labels[near] if near >= 0 else "-"} {_fixed(v[i])}\n')
    else:
        for c in range(len(size)):
            mine = v[cluster == c]
            lines.append(f'{labels[first[c]]} {size[c]} {_fixed(math.fsum(mine) / len(mine) if ok else None)} '
                         f'{_fixed(mine.min() if ok else None)} {int((mine < 0).sum()) if ok else 0}\n')
    return ''.join(lines).encode('utf8') + last_line(four, labels)
