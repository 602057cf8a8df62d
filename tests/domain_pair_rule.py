"""The rule of dct-sim --domains, stated in numpy: the oracle of test_domain_pairs_host.py (where it is pinned against a literal
restatement of the reference's loop) and test_domain_pairs_gpu.py.

The reference's domain_sim (src/dct-sim.py:42-50) runs over the fingerprints pi of the first protein, inside over the fingerprints
pj of the second, and replaces its running maximum -- started at 0 -- only when ``s > maxs``.  Similarity falls strictly with L1
below 17000 and is 0 from there on, so the pair the loop ends on is the one with the smallest L1, the first such in (pi, pj)
order, and there is none when that L1 is 17000 or more, or when a protein has no fingerprint."""

import numpy as np

NO_L1 = 0x7fffffff
FULL_SCALE = 17000
NONE = -1


def best_pair(a, b):
    """(min, last, arg_a, arg_b) of two fingerprint sets (rows = fingerprints)."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    if len(a) == 0 or len(b) == 0:
        return NO_L1, NO_L1, NONE, NONE
    d = np.abs(a[:, None, :] - b[None, :, :]).sum(axis=2)
    flat = int(np.argmin(d))                                    # (the first minimum in row-major order: lowest pi, then lowest pj)
    mn = int(d.flat[flat])
    pi, pj = divmod(flat, d.shape[1])
    return (mn, int(d[-1, -1])) + ((pi, pj) if mn < FULL_SCALE else (NONE, NONE))


def pair_args(dct_a, idx_a, dct_b, idx_b, i, j):
    """(min, last, arg_a, arg_b), int64 arrays: ``best_pair`` of the protein pairs (i[k] of a, j[k] of b)."""
    idx_a, idx_b = np.asarray(idx_a, dtype=np.int64), np.asarray(idx_b, dtype=np.int64)
    out = np.empty((4, len(i)), dtype=np.int64)
    for k, (p, q) in enumerate(zip(i, j)):
        out[:, k] = best_pair(dct_a[idx_a[p]:idx_a[p + 1]], dct_b[idx_b[q]:idx_b[q + 1]])
    return out[0], out[1], out[2], out[3]


def pair_facts(dct_a, idx_a, dct_b, idx_b, i, j):
    """(tied, whole) boolean arrays over the protein pairs that have an L1 at all: the smallest L1 is reached by more than one
    fingerprint pair; its first position is (last row, last row) -- whole protein x whole protein -- whatever its value."""
    idx_a, idx_b = np.asarray(idx_a, dtype=np.int64), np.asarray(idx_b, dtype=np.int64)
    tied, whole = np.zeros(len(i), dtype=bool), np.zeros(len(i), dtype=bool)
    for k, (p, q) in enumerate(zip(i, j)):
        a, b = np.asarray(dct_a[idx_a[p]:idx_a[p + 1]], dtype=np.int64), np.asarray(dct_b[idx_b[q]:idx_b[q + 1]], dtype=np.int64)
        if len(a) and len(b):
            d = np.abs(a[:, None, :] - b[None, :, :]).sum(axis=2)
            tied[k] = np.count_nonzero(d == d.min()) > 1
            whole[k] = int(np.argmin(d)) == d.size - 1
    return tied, whole


def triangle_args(dct, idx):
    """(i, j, min, last, arg_i, arg_j) over the upper triangle of one file in output order (i ascending, then j)."""
    i, j = np.triu_indices(len(idx) - 1, 1)
    return (i, j) + pair_args(dct, idx, dct, idx, i, j)


def labels(idx, doms=None, sid=None):
    """What is printed for every fingerprint row: its 1-based index within the protein, or -- ``doms`` = {pid: [names]} of the .dom
    file -- the names, ``whole`` for the unnamed last row of a protein with one name fewer than fingerprints."""
    out = []
    for p, k in enumerate(np.diff(np.asarray(idx, dtype=np.int64)).tolist()):
        if doms is None:
            out += [str(r + 1) for r in range(k)]
        elif k:
            names = list(doms[str(sid[p])])
            assert len(names) in (k, k - 1)
            out += names + ['whole'] * (k - len(names))
    return out


def label(names, first_row, arg):
    return '-' if arg < 0 else names[first_row + arg]


def read_dom(path):
    """{pid: [names]} of a .dom file whose pids hold no blank (the committed fixtures)."""
    doms = {}
    with open(path, encoding='utf8') as fh:
        for line in fh:
            pid, count, names = line.split()
            doms[pid] = names.split(';')
            assert len(doms[pid]) == int(count)
    return doms
