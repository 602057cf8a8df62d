"""The rule of dct-sim --cluster --level domain, stated in numpy: the oracle of test_domain_cluster_host.py (where it is pinned on
the committed reference fixtures) and test_domain_cluster_gpu.py.

Nodes: every fingerprint row of the file; row r belongs to protein owner[r].  With ``whole=False`` (--no-whole) the last row of
every protein of more than one fingerprint -- its whole-protein row -- is no node.
Edges: rows a < b of different proteins, both nodes, whose own L1 passes the cut-off the way a protein pair's minimum passes it in
all_sim_filter_rule.kept: not (1 - min(L1 / 17000, 1) < min_domain).
label[r] = the smallest row in the component of r (cluster_rule.components), -1 for a row that is no node.
The text has one line "{id of the representative's protein} {id of the member's protein} {label of the representative row}
{label of the member row}" per node, clusters by representative row, members by row."""

import numpy as np

import all_sim_filter_rule as rule
import cluster_rule as crule

HEADER = b'#representative member dom1 dom2\n'


def owners(idx):
    idx = np.asarray(idx, dtype=np.int64)
    return np.repeat(np.arange(len(idx) - 1), np.diff(idx))


def nodes(idx, whole=True):
    idx = np.asarray(idx, dtype=np.int64)
    keep = np.ones(int(idx[-1]), dtype=bool)
    if not whole:
        for p in range(len(idx) - 1):
            if idx[p + 1] - idx[p] > 1:
                keep[idx[p + 1] - 1] = False
    return keep


def row_l1(dct):
    """(R, R) int64 L1 between all rows, a block of rows at a time."""
    rows = np.asarray(dct, dtype=np.int16)
    out = np.zeros((len(rows), len(rows)), dtype=np.int64)
    for r0 in range(0, len(rows), 32):
        out[r0:r0 + 32] = np.abs(rows[r0:r0 + 32, None, :] - rows[None, :, :]).sum(axis=2, dtype=np.int64)
    return out


def edges(dct, idx, min_domain, whole=True, skip=None):
    """(a, b) of every edge, a < b.  ``skip`` (bool per row) replaces the node rule of ``whole``."""
    idx = np.asarray(idx, dtype=np.int64)
    total = int(idx[-1])
    l1 = row_l1(np.asarray(dct)[:total])
    own = owners(idx)
    keep = nodes(idx, whole) if skip is None else ~np.asarray(skip, dtype=bool)
    passes = rule.kept(l1.ravel(), l1.ravel(), min_domain).reshape(l1.shape)
    ok = passes & (own[:, None] != own[None, :]) & keep[:, None] & keep[None, :] & (np.arange(total)[:, None] < np.arange(total)[None, :])
    return np.nonzero(ok)


def labels(dct, idx, min_domain, whole=True, skip=None):
    idx = np.asarray(idx, dtype=np.int64)
    a, b = edges(dct, idx, min_domain, whole, skip)
    label = crule.components(int(idx[-1]), a, b)
    label[~(nodes(idx, whole) if skip is None else ~np.asarray(skip, dtype=bool))] = -1
    return label


def project(label, idx):
    """Protein labels from row labels (all rows nodes): the row components with all rows of each protein joined as well, a protein
    without rows standing alone; label = the smallest protein of the component."""
    idx = np.asarray(idx, dtype=np.int64)
    n = len(idx) - 1
    own = owners(idx)
    rows = np.arange(len(own))
    return crule.components(n, own[rows], own[np.asarray(label)])


def text(sid, idx, label, row_labels) -> bytes:
    """The result lines (without the header), by a stable sort of the nodes by label."""
    own = owners(idx)
    order = sorted((r for r in range(len(label)) if label[r] >= 0), key=lambda r: int(label[r]))      # (Python's sort is stable)
    return b''.join(f'{sid[own[int(label[r])]]} {sid[own[r]]} {row_labels[int(label[r])]} {row_labels[r]}\n'.encode('utf8') for r in order)


def summary(label):
    """(clusters, size of the largest) among the nodes."""
    _, size = np.unique(label[label >= 0], return_counts=True)
    return len(size), int(size.max())
