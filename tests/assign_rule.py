"""The rule of dct-sim --assign, stated in plain Python and numpy: the oracle of test_assign_host.py (where it is worked by hand
and checked against greedy_rule on the committed reference golden) and test_assign_gpu.py.

Inputs: a representative file R with m proteins, a query file N with n proteins, cut-offs.  Nodes are numbered 0 .. m - 1 for R
and m .. m + n - 1 for N, each file in its own order.  An edge joins a node of R u N to a later node of N exactly when the
cut-offs keep that protein pair (all_sim_filter_rule.kept over the pair's L1 values, as for greedy_rule).  Edges inside R do not
exist: every protein of R is a representative, whatever its distance to the others.  Then the greedy rule runs over N in file
order: a protein of N with an edge from a representative (of R, or an earlier new one) belongs to the lowest such node;
otherwise it becomes a representative itself.  This is greedy_rule.greedy on the concatenation with R forced.  The text has one
line per protein of N and none for the proteins of R."""

import numpy as np

import all_sim_filter_rule as rule

HEADER = b'#representative member\n'


def pair_values(rep_dct, rep_idx, dct, idx):
    """(i, j, min, last) of every pair that can be an edge: i < j, j >= m -- between R and N and inside N."""
    m, n = len(rep_idx) - 1, len(idx) - 1
    width = max([a.shape[1] for a in (np.asarray(rep_dct), np.asarray(dct)) if a.ndim == 2 and a.shape[0]], default=1)
    rows = [np.asarray(a, dtype=np.int64).reshape(-1, width) for a in (rep_dct, dct)]
    both = np.concatenate([rows[0][:int(rep_idx[-1])], rows[1][:int(idx[-1])]])
    both_idx = np.concatenate([np.asarray(rep_idx, dtype=np.int64), int(rep_idx[-1]) + np.asarray(idx, dtype=np.int64)[1:]])
    i, j = np.triu_indices(m + n, 1)
    wanted = j >= m
    i, j = i[wanted], j[wanted]
    return (i, j) + rule.pair_l1(both, both_idx, i, j)


def edges(rep_dct, rep_idx, dct, idx, min_domain=None, min_global=None, values=None):
    """(i, j) of the edges; ``values`` = ``pair_values`` of the files, computed once by a caller with several cut-offs."""
    i, j, mn, last = values if values is not None else pair_values(rep_dct, rep_idx, dct, idx)
    keep = rule.kept(mn, last, min_domain, min_global)
    return i[keep], j[keep]


def assign(m, n, i, j):
    """labels (int32, n) of the proteins of N, in the numbering above: greedy_rule.greedy's loop with the m first nodes forced
    to be representatives.  An edge may come either way round; one inside R is ignored."""
    later = [set() for _ in range(m + n)]
    for a, b in zip(np.asarray(i).tolist(), np.asarray(j).tolist()):
        if a != b and max(a, b) >= m:
            later[min(a, b)].add(max(a, b))
    label = list(range(m)) + [-1] * n
    for x in range(m + n):
        if label[x] == -1:
            label[x] = x
        if label[x] == x:                                     # a representative: of R, or a new one
            for y in sorted(later[x]):
                if label[y] == -1:
                    label[y] = x
    return np.array(label[m:], dtype=np.int32)


def labels(rep_dct, rep_idx, dct, idx, min_domain=None, min_global=None):
    i, j = edges(rep_dct, rep_idx, dct, idx, min_domain, min_global)
    return assign(len(rep_idx) - 1, len(idx) - 1, i, j)


def check(m, n, i, j, label):
    """The two properties, from the edges alone: every member has an edge to its label -- a representative -- and to no lower
    representative; no edge joins two new representatives."""
    label = np.asarray(label)
    assert label.shape == (n,)
    nodes = m + np.arange(n)
    assert ((label >= 0) & (label <= nodes)).all()
    full = np.concatenate([np.arange(m), label])
    is_rep = full == np.arange(m + n)
    assert is_rep[label].all()                                # every label is a representative
    around = [set() for _ in range(m + n)]
    for a, b in zip(np.asarray(i).tolist(), np.asarray(j).tolist()):
        if a != b and max(a, b) >= m:
            around[a].add(b)
            around[b].add(a)
            assert not (is_rep[a] and is_rep[b]), (a, b)      # no new representative within the cut-off of another one, old or new
    for x in np.flatnonzero(~is_rep).tolist():
        reps = [y for y in around[x] if is_rep[y]]
        assert reps and min(reps) == full[x], (x, int(full[x]), sorted(reps))


def text(rep_sid, sid, label) -> bytes:
    """One line per protein of N in the order of a stable sort by label: the clusters of the old representatives first, then
    the new representatives' clusters, each representative's own line first."""
    ids = [f'{s}' for s in rep_sid] + [f'{s}' for s in sid]
    m = len(rep_sid)
    order = np.argsort(np.asarray(label), kind='stable')
    return ''.join(f'{ids[int(label[k])]} {ids[m + int(k)]}\n' for k in order).encode('utf8')
