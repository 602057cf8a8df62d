"""The rule of dct-sim --cluster, stated in numpy: the oracle of test_cluster_host.py (where it is pinned on the committed
reference golden) and test_cluster_gpu.py.

The clusters of a file at cut-offs are the connected components of the undirected graph whose nodes are all proteins and whose
edges are exactly the pairs the cut-offs keep (all_sim_filter_rule.kept over all_sim_filter_rule.triangle_l1).  label[i] = the
smallest index in the component of protein i, its representative.  The text has one line "{id of representative} {id of
member}" per protein, clusters by representative index, members by index."""

import numpy as np

import all_sim_filter_rule as rule

HEADER = b'#representative member\n'


def components(n, i, j):
    """label (int32, n) of the graph with edges (i[k], j[k]): a plain sequential union-find, the smaller root on top."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in zip(np.asarray(i).tolist(), np.asarray(j).tolist()):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(x) for x in range(n)], dtype=np.int32)


def labels(dct, idx, min_domain=None, min_global=None):
    """(label, number of edges) of a file at the cut-offs."""
    i, j, mn, last = rule.triangle_l1(dct, idx)
    keep = rule.kept(mn, last, min_domain, min_global)
    return components(len(idx) - 1, i[keep], j[keep]), int(keep.sum())


def text(sid, label) -> bytes:
    """The result lines (without the header), by a stable sort of the proteins by label."""
    order = sorted(range(len(label)), key=lambda k: int(label[k]))      # (Python's sort is stable)
    return b''.join(f'{sid[int(label[k])]} {sid[k]}\n'.encode('utf8') for k in order)


def summary(label):
    """(clusters, size of the largest, clusters with more than one member)."""
    _, size = np.unique(label, return_counts=True)
    return len(size), int(size.max()), int((size > 1).sum())
