"""The rule of dct-sim --min-coverage, stated in numpy: the oracle of test_coverage_host.py (where it is worked by hand and run on
the committed reference fixture) and test_coverage_gpu.py.

Weights.  A protein of one fingerprint row: that row weighs W.  A protein of k > 1 rows: the domain rows 0 .. k - 2 weigh w_r,
W is their sum, and the last row -- the whole-protein fingerprint -- weighs W.  In residues w_r is the number of residues the row's
name covers ("1-30,61-100" -> 70; for k = 1, W is that row's count), in domains every domain row weighs 1 (W = max(1, k - 1)).
Need.  need_p = min(W_p, max(1, ceil(c W_p - 1e-9))): dct_sim.coverage_need, the one place where it is computed.
Matched.  Row r of protein p is matched by protein q when min over all rows s of q of min(L1(r, s), 17000) <= B, B = the largest
L1 in 0 .. 17000 whose similarity is not below min_domain.  cov(p by q) = the sum of w_r over the matched rows r of p.
Edge.  p and q are an edge when DCTdomain(p, q) >= min_domain, cov(p by q) >= need_p, cov(q by p) >= need_q, and DCTglobal >=
min_global if that is given.  A protein without rows has W = 0 and need 0: nothing is asked of it, and it is an edge only where a
DCTdomain of 0 passes -- under a cut-off that keeps every pair; under any cut-off that cuts, it never passes.
The all-against-all prints the edges (all_sim_filter_rule's lines, filtered), --cluster takes their components (cluster_rule),
--cluster --linkage greedy its file-order rule on them (greedy_rule)."""

import numpy as np

import all_sim_filter_rule as rule
import cluster_rule
import greedy_rule

NO_L1 = rule.NO_L1
CAP = 17000


def residues(name):
    """The residues a domain name covers: the sum of b - a + 1 over its comma-separated ranges a-b."""
    total = 0
    for part in str(name).split(','):
        lo, hi = part.split('-')
        total += int(hi) - int(lo) + 1
    return total


def weights(idx, names=None, unit='residues'):
    """One weight per fingerprint row (int64); ``names``: one domain name per row, read for ``unit='residues'``."""
    idx = np.asarray(idx, dtype=np.int64)
    w = np.zeros(int(idx[-1]), dtype=np.int64)
    for lo, hi in zip(idx[:-1].tolist(), idx[1:].tolist()):
        k = hi - lo
        if k == 0:
            continue
        parts = range(lo, hi - 1) if k > 1 else range(lo, hi)
        for r in parts:
            w[r] = residues(names[r]) if unit == 'residues' else 1
        if k > 1:
            w[hi - 1] = w[lo:hi - 1].sum()
    return w


def protein_weights(idx, w):
    """W per protein: the weight of its last row; 0 for a protein without rows."""
    idx = np.asarray(idx, dtype=np.int64)
    return np.array([w[hi - 1] if hi > lo else 0 for lo, hi in zip(idx[:-1].tolist(), idx[1:].tolist())], dtype=np.int64)


def need(W, c):
    from dctdomain_amd.dct_sim import coverage_need
    return np.array([coverage_need(int(v), c) for v in W], dtype=np.int64)


def bound_of(cut):
    """The largest L1 in 0 .. 17000 whose similarity is not below ``cut`` (-1: none)."""
    return int(np.count_nonzero(~(rule.similarity(np.arange(CAP + 1)) < cut))) - 1


def row_l1(a, b, chunk=64):
    """int64 (rows of a, rows of b): the L1 distances."""
    a, b = np.asarray(a, dtype=np.int16), np.asarray(b, dtype=np.int16)
    out = np.zeros((len(a), len(b)), dtype=np.int64)
    for r0 in range(0, len(a), chunk):
        out[r0:r0 + chunk] = np.abs(a[r0:r0 + chunk, None, :] - b[None, :, :]).sum(axis=2, dtype=np.int64)
    return out


def cover_tile(a, idx_a, w_a, need_a, b, idx_b, w_b, need_b, bound, cap=None, dist=None):
    """What dctfp_protein_cover computes, and why.  Returns a dict of (npa, npb) arrays: ``min`` (the protein minimum, NO_L1 where a
    protein has no rows), ``cov_a`` / ``cov_b`` (cov(pa by pb) / cov(pb by pa)), ``ok_a`` / ``ok_b`` (the coverage of that side
    reaches its need), ``whole`` (the last row of a protein of several rows is matched, on either side), ``out`` (``min`` where
    both are ok, else NO_L1).  A row is matched when its smallest L1 to the other protein's rows -- ``cap``: min(L1, cap) -- is
    <= ``bound``.  ``dist``: ``row_l1`` of the two sets' rows, where the caller has it."""
    idx_a, idx_b = np.asarray(idx_a, dtype=np.int64), np.asarray(idx_b, dtype=np.int64)
    w_a, w_b = np.asarray(w_a, dtype=np.int64), np.asarray(w_b, dtype=np.int64)
    npa, npb = len(idx_a) - 1, len(idx_b) - 1
    if dist is None:
        dist = row_l1(np.asarray(a)[:int(idx_a[-1])], np.asarray(b)[:int(idx_b[-1])])
    near_a = np.full((dist.shape[0], npb), NO_L1, dtype=np.int64)      # row of a x protein of b
    near_b = np.full((dist.shape[1], npa), NO_L1, dtype=np.int64)      # row of b x protein of a
    for q in range(npb):
        if idx_b[q + 1] > idx_b[q] and dist.shape[0]:
            near_a[:, q] = dist[:, idx_b[q]:idx_b[q + 1]].min(axis=1)
    for p in range(npa):
        if idx_a[p + 1] > idx_a[p] and dist.shape[1]:
            near_b[:, p] = dist[idx_a[p]:idx_a[p + 1], :].min(axis=0)
    hit_a = (near_a if cap is None else np.minimum(near_a, cap)) <= bound
    hit_b = (near_b if cap is None else np.minimum(near_b, cap)) <= bound
    mn = np.full((npa, npb), NO_L1, dtype=np.int64)
    cov_a, cov_b = np.zeros((npa, npb), dtype=np.int64), np.zeros((npa, npb), dtype=np.int64)
    whole = np.zeros((npa, npb), dtype=bool)
    for p in range(npa):
        lo, hi = idx_a[p], idx_a[p + 1]
        if hi > lo:
            mn[p] = near_a[lo:hi].min(axis=0)
            cov_a[p] = (w_a[lo:hi, None] * hit_a[lo:hi]).sum(axis=0)
            if hi - lo > 1:
                whole[p] |= hit_a[hi - 1]
    for q in range(npb):
        lo, hi = idx_b[q], idx_b[q + 1]
        if hi > lo:
            cov_b[:, q] = (w_b[lo:hi, None] * hit_b[lo:hi]).sum(axis=0)
            if hi - lo > 1:
                whole[:, q] |= hit_b[hi - 1]
    ok_a = cov_a >= np.asarray(need_a, dtype=np.int64)[:, None]
    ok_b = cov_b >= np.asarray(need_b, dtype=np.int64)[None, :]
    return {'min': mn, 'cov_a': cov_a, 'cov_b': cov_b, 'ok_a': ok_a, 'ok_b': ok_b, 'whole': whole,
            'out': np.where(ok_a & ok_b, mn, NO_L1), 'dist': dist}


def edges(dct, idx, w, min_domain, c, min_global=None, dist=None):
    """(i, j, min, last, keep) over the upper triangle in output order: ``keep`` marks the edges."""
    idx = np.asarray(idx, dtype=np.int64)
    n = len(idx) - 1
    nd = need(protein_weights(idx, w), c)
    t = cover_tile(dct, idx, w, nd, dct, idx, w, nd, bound_of(min_domain), cap=CAP, dist=dist)
    i, j = np.triu_indices(n, 1)
    mn = t['min'][i, j]
    last = np.full(len(i), NO_L1, dtype=np.int64)
    has = (idx[1:] > idx[:-1])
    both = has[i] & has[j]
    last[both] = t['dist'][idx[1:][i[both]] - 1, idx[1:][j[both]] - 1]
    keep = rule.kept(mn, last, min_domain, min_global) & (t['ok_a'] & t['ok_b'])[i, j]
    return i, j, mn, last, keep


def components(n, i, j, keep):
    return cluster_rule.components(n, i[keep], j[keep])


def greedy(n, i, j, keep):
    return greedy_rule.greedy(n, i[keep], j[keep])
