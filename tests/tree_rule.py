"""The rule of dct-sim --tree, stated in numpy: the oracle of test_tree_host.py (where it is pinned on the committed reference
golden) and test_tree_gpu.py.

Nodes are the proteins of a file.  Candidate edges are the pairs i < j with key(i, j) = min(L1, 17000) <= bound, L1 = the
smallest L1 over all fingerprint pairs (score 'domain') or the L1 of the two last fingerprints (score 'global'); a protein
without fingerprints has no L1 against anything (0x7fffffff: key 17000).  Edges are totally ordered by (key, i, j); the tree is the
minimum spanning forest under that order -- Kruskal over the sorted candidates; unique, because the order is strict.  The text
has one all-against-all line "{id i} {id j} {DCTdomain:.3f} {DCTglobal:.3f}" per tree edge, in that order."""

import numpy as np

import all_sim_filter_rule as rule
import cluster_rule as crule

HEADER = b'#prot1 prot2 sim-domain sim-global\n'
CAP = 17000
DEFAULT_BOUND = CAP - 1                                        # every pair of similarity above 0


def keys(mn, last, score):
    """key of every pair from its (min, last) L1."""
    return np.minimum(np.asarray(mn if score == 'domain' else last, dtype=np.int64), CAP)


def kruskal(n, i, j, key, bound):
    """(i, j, key) of the minimum spanning forest of the candidates with key <= bound, in (key, i, j) order."""
    i, j, key = (np.asarray(a, dtype=np.int64) for a in (i, j, key))
    order = np.lexsort((j, i, key))
    order = order[key[order] <= bound]
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    taken = []
    for k in order.tolist():
        a, b = find(int(i[k])), find(int(j[k]))
        if a != b:
            parent[max(a, b)] = min(a, b)
            taken.append(k)
    taken = np.asarray(taken, dtype=np.int64)
    return i[taken], j[taken], key[taken]


def edges(dct, idx, score='domain', bound=DEFAULT_BOUND, triangle=None):
    """(i, j, key) of the tree of a file; ``triangle`` = all_sim_filter_rule.triangle_l1 of it where the caller has it already."""
    i, j, mn, last = triangle if triangle is not None else rule.triangle_l1(dct, idx)
    return kruskal(len(idx) - 1, i, j, keys(mn, last, score), bound)


def _score(l1) -> float:
    return 1 - min(int(l1) / CAP, 1)


def text(sid, dct, idx, i, j) -> bytes:
    """The result lines (without the header) of the edges (i[k], j[k]), in the order given."""
    mn, last = rule.pair_l1(dct, idx, i, j)
    return b''.join(f'{sid[a]} {sid[b]} {max(_score(m), 0):.3f} {_score(g):.3f}\n'.encode('utf8')
                    for a, b, m, g in zip(np.asarray(i).tolist(), np.asarray(j).tolist(), mn.tolist(), last.tolist()))


def cut(n, i, j, key, b):
    """label (int32, n) of the components of the tree's edges with key <= b."""
    keep = np.asarray(key) <= b
    return crule.components(n, np.asarray(i)[keep], np.asarray(j)[keep])
