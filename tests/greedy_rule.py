"""The rule of dct-sim --cluster --linkage greedy, stated in plain Python: the oracle of test_greedy_host.py (where it is worked
by hand and run on the committed reference golden) and test_greedy_gpu.py.

Nodes are the proteins of the file in file order, edges exactly the pairs the cut-offs keep (all_sim_filter_rule.kept over
all_sim_filter_rule.triangle_l1, as for cluster_rule).  Greedy incremental clustering in file order: a protein that no earlier
representative has an edge to becomes a representative, and every later uncovered protein it has an edge to gets it as its
label.  So the representatives are the lexicographically first maximal independent set, and every other protein carries the
lowest representative it has an edge to.  The text is cluster_rule's."""

import numpy as np

import all_sim_filter_rule as rule
from cluster_rule import HEADER, text  # noqa: F401  (the same lines from other labels)


def _neighbours(n, i, j):
    """Per node the sorted later ends of its edges; an edge may come either way round, i == j is none."""
    later = [set() for _ in range(n)]
    for a, b in zip(np.asarray(i).tolist(), np.asarray(j).tolist()):
        if a != b:
            later[min(a, b)].add(max(a, b))
    return [sorted(s) for s in later]


def greedy(n, i, j):
    """label (int32, n) of the graph with edges (i[k], j[k]): the loop of the rule."""
    later = _neighbours(n, i, j)
    label = [-1] * n
    for x in range(n):
        if label[x] == -1:                                    # not covered by an earlier representative
            label[x] = x                                      # x is a representative
            for y in later[x]:
                if label[y] == -1:
                    label[y] = x
    return np.array(label, dtype=np.int32)


def labels(dct, idx, min_domain=None, min_global=None):
    """(label, number of edges) of a file at the cut-offs."""
    i, j, mn, last = rule.triangle_l1(dct, idx)
    keep = rule.kept(mn, last, min_domain, min_global)
    return greedy(len(idx) - 1, i[keep], j[keep]), int(keep.sum())


def check(n, i, j, label):
    """The two properties, from the edges alone: every non-representative has an edge to its label -- a representative -- and to
    no lower representative; no edge joins two representatives."""
    label = np.asarray(label)
    assert label.shape == (n,)
    nodes = np.arange(n)
    assert ((label >= 0) & (label <= nodes)).all()
    is_rep = label == nodes
    assert is_rep[label].all()                                # every label is a representative
    around = [set() for _ in range(n)]
    for a, b in zip(np.asarray(i).tolist(), np.asarray(j).tolist()):
        if a != b:
            around[a].add(b)
            around[b].add(a)
            assert not (is_rep[a] and is_rep[b]), (a, b)      # no two representatives within the cut-off of each other
    for x in np.flatnonzero(~is_rep).tolist():
        reps = [y for y in around[x] if is_rep[y]]
        assert reps and min(reps) == label[x], (x, int(label[x]), sorted(reps))
