"""The rule of dct-sim --cluster --min-neighbors, stated in numpy: the oracle of test_density_host.py (where it is pinned on the
committed reference fixture and checked against a textbook sequential DBSCAN) and test_density_gpu.py.

G is the graph of cluster_rule: the proteins 0 .. n - 1 of a file and, as edges, exactly the pairs the cut-offs keep
(all_sim_filter_rule.kept over all_sim_filter_rule.triangle_l1, or coverage_rule.edges under a coverage).  deg(x) = the number of
edges at x; x itself is not counted.  With M = --min-neighbors, an integer >= 1:
- x is a core when deg(x) >= M; a cluster's cores are a connected component of the edges whose two ends are both cores;
- a non-core with at least one core neighbour is a border and joins the cluster of its LOWEST core neighbour;
- a non-core with no core neighbour is noise, a cluster of its own.
label[x] = the smallest index among all members of x's cluster, cores and borders alike.  The text is cluster_rule.text's."""

import numpy as np

import all_sim_filter_rule as rule
import cluster_rule

NOISE, BORDER, CORE = 0, 1, 2
NONE = 0x7fffffff


def nearest_core(n, i, j, core):
    """int64 (n): per protein the lowest core at the other end of one of its edges with exactly one core end (NONE: there is
    none) -- for a non-core its lowest core neighbour; a core keeps NONE."""
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    near = np.full(n, NONE, dtype=np.int64)
    a, b = core[i] & ~core[j], core[j] & ~core[i]
    np.minimum.at(near, j[a], i[a])
    np.minimum.at(near, i[b], j[b])
    return near


def clusters(n, i, j, m):
    """(label int32, kind uint8, deg int64) of the graph with edges (i[k], j[k]), each unordered pair once, at M = m."""
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    deg = np.bincount(i, minlength=n) + np.bincount(j, minlength=n)
    core = deg >= m
    both = core[i] & core[j]
    comp = cluster_rule.components(n, i[both], j[both]).astype(np.int64)     # a non-core is on none of these edges: itself
    near = nearest_core(n, i, j, core)
    border = ~core & (near != NONE)
    lab = comp.copy()
    lab[border] = comp[near[border]]
    first = np.full(n, n, dtype=np.int64)
    np.minimum.at(first, lab, np.arange(n))
    kind = np.where(core, CORE, np.where(border, BORDER, NOISE)).astype(np.uint8)
    return first[lab].astype(np.int32), kind, deg


def of_file(dct, idx, m, min_domain=None, min_global=None, triangle=None):
    """(label, kind, deg) of a file at the cut-offs; ``triangle``: all_sim_filter_rule.triangle_l1 of it, where the caller has it."""
    i, j, mn, last = triangle if triangle is not None else rule.triangle_l1(dct, idx)
    keep = rule.kept(mn, last, min_domain, min_global)
    return clusters(len(idx) - 1, i[keep], j[keep], m)


def counts(kind):
    """(cores, borders, noise)."""
    return int((kind == CORE).sum()), int((kind == BORDER).sum()), int((kind == NOISE).sum())


# ---- what one int32 tile contributes, as the two kernels scan it (entries as all_sim_filter_rule.tile_keep keeps them)

def tile_degrees(t, row0, col0, bound, row_empty=None, col_empty=None, cap=17000, n_nodes=None):
    """uint32 (n_nodes): what dctfp_tri_degree adds to deg -- 1 at both ends of every kept entry."""
    _, i, j = rule.tile_filter(t, row0, col0, bound, row_empty, col_empty, cap)
    n_nodes = n_nodes if n_nodes is not None else max(row0 + t.shape[0], col0 + t.shape[1])
    return (np.bincount(i, minlength=n_nodes) + np.bincount(j, minlength=n_nodes)).astype(np.uint32)


def tile_link_core(t, row0, col0, bound, core, row_empty=None, col_empty=None, cap=17000):
    """(label int32, nearest int32), one per entry of ``core``: what dctfp_tri_link_core leaves in a fresh forest (read as
    dctfp_cluster_labels reads it: the smallest member of every component of the kept core-core entries) and in a fresh nearest."""
    core = np.asarray(core).astype(bool)
    _, i, j = rule.tile_filter(t, row0, col0, bound, row_empty, col_empty, cap)
    both = core[i] & core[j]
    return cluster_rule.components(len(core), i[both], j[both]), nearest_core(len(core), i, j, core).astype(np.int32)
