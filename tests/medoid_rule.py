"""The rule of dct-sim --cluster --rep medoid, stated in numpy: the oracle of test_medoid_host.py (where it is pinned on the committed
reference fixture) and test_medoid_gpu.py.

Inputs: the proteins 0 .. n - 1 of a file, their single-linkage labels (cluster_rule.labels: the smallest member of each cluster) and a
key per unordered pair, key(i, j) = min(L1(i, j), 17000) of the route's score -- DCTglobal's last-row L1 when a DCTglobal cut-off is
given (alone or beside the other), else DCTdomain's protein minimum.  A protein without a fingerprint has no L1 against anything
(all_sim_filter_rule.NO_L1): key 17000 to everyone.  A coverage cut-off decides the labels only: the keys stay the plain ones.

S(x) = the sum of key(x, y) over y != x with label[y] == label[x], an exact integer.  medoid(c) = the member x of cluster c with the
smallest S(x), ties to the lowest index; rep[x] = medoid(label[x]).  A singleton is its own medoid; in a cluster of two both sums are
equal, so the medoid is the first member.

The text is cluster_rule.text's with another first field: one line "{id of rep[k]} {id of k}" per protein k, clusters by their
smallest member, members by index."""

import numpy as np

import all_sim_filter_rule as rule

CAP = 17000
ROUTES = ('domain', 'global')


def route_of(min_global=None) -> str:
    """The score the keys come from at the cut-offs of a run."""
    return 'global' if min_global is not None else 'domain'


def key_matrix(dct, idx, route='domain', triangle=None):
    """int64 (n, n), symmetric, the diagonal 0: key(i, j) of the route.  ``triangle``: all_sim_filter_rule.triangle_l1 of the file,
    where the caller has it."""
    assert route in ROUTES
    n = len(idx) - 1
    i, j, mn, last = triangle if triangle is not None else rule.triangle_l1(dct, idx)
    key = np.zeros((n, n), dtype=np.int64)
    key[i, j] = np.minimum(mn if route == 'domain' else last, CAP)
    return key + key.T


def sums(key, labels):
    """S (int64, n) of a key matrix and labels."""
    key, labels = np.asarray(key, dtype=np.int64), np.asarray(labels)
    same = labels[:, None] == labels[None, :]
    np.fill_diagonal(same, False)
    return (key * same).sum(axis=1)


def tile_sums(t, row0, col0, labels, row_empty=None, col_empty=None, cap=CAP):
    """What one int32 tile adds to S (uint64, one per label entry), as dctfp_label_sums scans it: entry (r, c) stands for proteins
    i = row0 + r and j = col0 + c, key as all_sim_filter_rule.tile_keep forms it; an entry with j > i and label[i] == label[j]
    adds its key to S[i] and to S[j]."""
    labels = np.asarray(labels)
    upper, key = rule.tile_keep(t, row0, col0, cap, row_empty, col_empty, cap)      # (bound = cap: every entry right of the diagonal)
    i = row0 + np.arange(t.shape[0])
    j = col0 + np.arange(t.shape[1])
    r, c = np.nonzero(upper & (labels[i][:, None] == labels[j][None, :]))
    out = np.zeros(len(labels), dtype=np.uint64)
    np.add.at(out, i[r], key[r, c].astype(np.uint64))
    np.add.at(out, j[c], key[r, c].astype(np.uint64))
    return out


def medoids(key, labels):
    """rep (int32, n): a plain loop over the clusters."""
    labels = np.asarray(labels)
    s = sums(key, labels)
    rep = np.zeros(len(labels), dtype=np.int32)
    for c in np.unique(labels):
        members = np.flatnonzero(labels == c)                  # (ascending: argmin takes the first of equal sums)
        rep[members] = members[np.argmin(s[members])]
    return rep


def text(sid, labels, rep) -> bytes:
    """The result lines (without the header), by a stable sort of the proteins by label."""
    order = sorted(range(len(labels)), key=lambda k: int(labels[k]))      # (Python's sort is stable)
    return b''.join(f'{sid[int(rep[k])]} {sid[k]}\n'.encode('utf8') for k in order)
