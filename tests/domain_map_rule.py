"""The rule of dct-sim --domain-map, stated as a literal double loop in numpy: the oracle of test_domain_map_host.py and
test_domain_map_gpu.py.  It shares no code with the product.

Take a pair (P, Q) with fingerprint rows P_0 .. P_(k-1) and Q_0 .. Q_(m-1); all rows count, the whole-protein row included, exactly
as in DCTdomain's loop.  d(i, j) is their L1.  The counterpart of row i of P is the j with the smallest d(i, j), ties to the lowest
j; the counterpart of row j of Q the i with the smallest d(i, j), ties to the lowest i.  A row is matched when that minimum is at
most B = min(bound(X), 16999), where bound(X) is the largest L1 whose similarity 1 - min(L1 / 17000, 1) is not below X, found by
evaluating that expression on every L1 (no algebra: it is off by one at some X).  A similarity of 0 never matches."""

import numpy as np

NO_L1 = 0x7fffffff
NONE = -1
FULL_SCALE = 17000


def bound(x):
    """B of a similarity X."""
    largest = -1
    for l1 in range(FULL_SCALE + 1):
        if not (1 - min(l1 / FULL_SCALE, 1) < x):
            largest = l1
    return min(largest, FULL_SCALE - 1)


def row_best(p, q):
    """(l1_p, arg_p, l1_q, arg_q): per row of P its smallest L1 to a row of Q and that row, and the same per row of Q; NO_L1 and
    NONE where the other protein has no rows."""
    p, q = np.asarray(p, dtype=np.int64), np.asarray(q, dtype=np.int64)
    k, m = len(p), len(q)
    l1_p, arg_p = [NO_L1] * k, [NONE] * k
    l1_q, arg_q = [NO_L1] * m, [NONE] * m
    for i in range(k):
        for j in range(m):
            d = int(np.abs(p[i] - q[j]).sum())
            if d < l1_p[i]:                                     # (j ascending: the lowest j among equals stands)
                l1_p[i], arg_p[i] = d, j
            if d < l1_q[j]:                                     # (i ascending: the lowest i among equals stands)
                l1_q[j], arg_q[j] = d, i
    return l1_p, arg_p, l1_q, arg_q


def sides(p, q, b):
    """(first, second): the entries (row, counterpart, L1) of the matched rows of P and of Q, in row order."""
    l1_p, arg_p, l1_q, arg_q = row_best(p, q)
    first = [(i, arg_p[i], l1_p[i]) for i in range(len(l1_p)) if l1_p[i] <= b]
    second = [(j, arg_q[j], l1_q[j]) for j in range(len(l1_q)) if l1_q[j] <= b]
    return first, second


def pair_text(l1):
    """The text --pair, --db and --rbh print a similarity with: the reference's scalar arithmetic."""
    return str(1 - min(np.int64(l1) / FULL_SCALE, 1))


def all_text(l1):
    """The text the all-against-all prints a similarity with."""
    return '%.3f' % (1 - min(np.int64(l1) / FULL_SCALE, 1))


def field(p, q, b, names_p, names_q, text=pair_text):
    """The map field of the pair: side '/' side, a side '-' or its entries label=label:score joined by ';'."""
    out = []
    for entries, own, other in zip(sides(p, q, b), (names_p, names_q), (names_q, names_p)):
        out.append(';'.join('%s=%s:%s' % (own[r], other[c], text(v)) for r, c, v in entries) or '-')
    return out[0] + '/' + out[1]


def index_names(n):
    return [str(r + 1) for r in range(n)]


def file_field(dct_a, idx_a, names_a, dct_b, idx_b, names_b, i, j, b, text=pair_text):
    """``field`` of protein i of file a and protein j of file b; ``names`` = one label per fingerprint row of a file, or None for
    the 1-based indices."""
    a0, a1, b0, b1 = int(idx_a[i]), int(idx_a[i + 1]), int(idx_b[j]), int(idx_b[j + 1])
    na = names_a[a0:a1] if names_a is not None else index_names(a1 - a0)
    nb = names_b[b0:b1] if names_b is not None else index_names(b1 - b0)
    return field(dct_a[a0:a1], dct_b[b0:b1], b, na, nb, text)


def flat(dct_a, idx_a, dct_b, idx_b, pairs):
    """(row_off, l1, arg), int64 arrays: what dctfp_pair_row_best returns for the pairs -- per pair the rows of the protein of a,
    then those of the protein of b."""
    off, l1, arg = [0], [], []
    for i, j in pairs:
        l1_p, arg_p, l1_q, arg_q = row_best(dct_a[idx_a[i]:idx_a[i + 1]], dct_b[idx_b[j]:idx_b[j + 1]])
        l1 += l1_p + l1_q
        arg += arg_p + arg_q
        off.append(len(l1))
    return np.array(off, dtype=np.int64), np.array(l1, dtype=np.int64), np.array(arg, dtype=np.int64)
