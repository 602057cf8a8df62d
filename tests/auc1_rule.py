"""The rule of dct-sim --auc1, stated in numpy: the oracle of test_auc1_host.py (where it is worked by hand and pinned on the
committed reference fixture) and test_auc1_gpu.py.

The file has proteins 0 .. n - 1 and every protein x has a family fam[x].  key(x, y) = min(L1(x, y), 17000) of the score --
DCTdomain's protein minimum or DCTglobal's last-row L1 -- and 17000 where either protein has no fingerprint
(medoid_rule.key_matrix).  y != x is a HIT of x when key(x, y) <= bound; bound = 16999, every pair of similarity above 0, unless the
score's cut-off gives dct_sim.sim_bound(cut).  The hits of x are ranked by (key, y): ties go to the lower index in the file.

Per protein x, with word(y) = key(x, y) << 32 | y:
- first_fp[x] = the smallest word over the hits y with fam[y] != fam[x]; NONE (all ones) when there is none;
- tp[x]       = the number of hits y with fam[y] == fam[x] and word(y) < first_fp[x];
- auc1[x]     = tp[x] / (size(fam[x]) - 1), and 0 for a family of one (the ZeroDivisionError branch of the reference's
                bench/cathdb/plot_results.py).

The best hit of x is a true positive exactly when tp[x] >= 1.  If the overall best hit b of x is of another family, b is itself the
smallest word among the false positives, so first_fp[x] = word(b) and no hit ranks before it: tp[x] = 0.  If b is of x's family,
word(b) is below every other word, first_fp[x] included, so b is counted: tp[x] >= 1.  And without any hit tp[x] = 0 and there is no
best hit.  So the top-1 rates need no third pass (test_auc1_host.py checks this against an independently computed best hit).

Summary over the QUERIES, the proteins whose family has at least two members: the mean AUC1; Qraw = the share of queries with
tp >= 1; Qnorm = the mean over those families of each family's share.  (Without a query all three are 0.)

The reference's script reads the same numbers out of ranked text: it ranks fingerprint rows with faiss and keeps 300 hits per
query, where this rule ranks proteins by dct-sim's own scores and has no hit limit."""

import numpy as np

import all_sim_filter_rule as rule
import medoid_rule as mr

CAP = 17000
BOUND_ALL = CAP - 1                 # every pair of similarity above 0
NONE = 0xffffffffffffffff          # first_fp: no false positive


def word(key, y) -> int:
    return int(key) << 32 | int(y)


def of_keys(K, fam, bound=BOUND_ALL):
    """(tp int32, fp_index int32, fp_key int32) of a symmetric key matrix K (n x n, the diagonal is not read) by brute force, the
    reference's read_results restated: per query sort (key, y), skip the query itself, walk the list and stop at the first hit of
    another family.  fp_index -1 and fp_key 17000: the walk met no false positive."""
    K = np.asarray(K, dtype=np.int64)
    n = len(fam)
    tp, fp_index, fp_key = np.zeros(n, dtype=np.int32), np.full(n, -1, dtype=np.int32), np.full(n, CAP, dtype=np.int32)
    for x in range(n):
        hits = sorted((int(K[x, y]), y) for y in range(n) if y != x and K[x, y] <= bound)
        for key, y in hits:
            if fam[y] != fam[x]:
                fp_index[x], fp_key[x] = y, key
                break
            tp[x] += 1
    return tp, fp_index, fp_key


def of_file(dct, idx, fam, score='domain', min_cut=None, triangle=None):
    """of_keys of a file: the keys of ``score``, the bound of ``min_cut`` (None: BOUND_ALL)."""
    from dctdomain_amd.dct_sim import sim_bound
    bound = BOUND_ALL if min_cut is None else sim_bound(min_cut)
    return of_keys(mr.key_matrix(dct, idx, score, triangle), fam, bound)


def auc1(tp, fam):
    """float64 (n): a plain loop."""
    fam = list(fam)
    out = np.zeros(len(fam), dtype=np.float64)
    for x, f in enumerate(fam):
        size = fam.count(f)
        out[x] = tp[x] / (size - 1) if size > 1 else 0.0
    return out


def summary(tp, fam) -> dict:
    """queries, families, mean_auc1, top1_raw, top1_norm: plain loops over the queries and over their families."""
    fam = list(fam)
    a = auc1(tp, fam)
    queries = [x for x, f in enumerate(fam) if fam.count(f) > 1]
    if not queries:
        return {'queries': 0, 'families': 0, 'mean_auc1': 0.0, 'top1_raw': 0.0, 'top1_norm': 0.0}
    shares = []
    for f in dict.fromkeys(fam[x] for x in queries):
        members = [x for x in queries if fam[x] == f]
        shares.append(sum(1 for x in members if tp[x] >= 1) / len(members))
    return {'queries': len(queries), 'families': len(shares), 'mean_auc1': sum(a[x] for x in queries) / len(queries),
            'top1_raw': sum(1 for x in queries if tp[x] >= 1) / len(queries), 'top1_norm': sum(shares) / len(shares)}


HEADER = b'#query family members tp auc1 first_fp fp_score\n'


def score_text(key: int) -> str:
    """A similarity as the pair lines print it: '%.3f' of 1 - min(L1 / 17000, 1) (all_sim_filter_rule.similarity)."""
    return '%.3f' % float(rule.similarity(key))


def text(sid, fam, tp, fp_index, fp_key) -> bytes:
    """The result lines (without the header) and the summary line."""
    fam = list(fam)
    a = auc1(tp, fam)
    lines = []
    for x in range(len(fam)):
        fp = (f'{sid[int(fp_index[x])]}', score_text(fp_key[x])) if fp_index[x] >= 0 else ('-', '-')
        lines.append(f'{sid[x]} {fam[x]} {fam.count(fam[x])} {int(tp[x])} {a[x]:.4f} {fp[0]} {fp[1]}\n')
    s = summary(tp, fam)
    lines.append(f"# queries={s['queries']} families={s['families']} mean_auc1={s['mean_auc1']:.4f} top1_raw={s['top1_raw']:.4f} "
                 f"top1_norm={s['top1_norm']:.4f}\n")
    return ''.join(lines).encode('utf8')


# ---- what one int32 tile contributes, as the two kernels scan it (entries as all_sim_filter_rule.tile_filter keeps them)

def _kept(t, row0, col0, bound, row_empty, col_empty, cap):
    """(i, j, key) of the kept entries: tile_filter's entries with tile_keep's keys, in the same row-major order."""
    _, i, j = rule.tile_filter(t, row0, col0, bound, row_empty, col_empty, cap)
    _, key = rule.tile_keep(t, row0, col0, bound, row_empty, col_empty, cap)
    return i, j, key[i - row0, j - col0]


def tile_first_fp(t, row0, col0, bound, fam, row_empty=None, col_empty=None, cap=CAP, first=None):
    """uint64 (one per entry of ``fam``): what dctfp_tri_first_fp leaves in ``first`` (NONE everywhere when not given) -- a kept
    entry (i, j) of two families lowers first[i] to key << 32 | j and first[j] to key << 32 | i."""
    fam = np.asarray(fam)
    out = np.full(len(fam), NONE, dtype=np.uint64) if first is None else np.array(first, dtype=np.uint64)
    i, j, key = _kept(t, row0, col0, bound, row_empty, col_empty, cap)
    other = fam[i] != fam[j]
    i, j, key = i[other].astype(np.uint64), j[other].astype(np.uint64), key[other].astype(np.uint64)
    np.minimum.at(out, i.astype(np.int64), key << np.uint64(32) | j)
    np.minimum.at(out, j.astype(np.int64), key << np.uint64(32) | i)
    return out


def tile_tp_before(t, row0, col0, bound, fam, first, row_empty=None, col_empty=None, cap=CAP):
    """(uint32 per entry of ``fam``: what dctfp_tri_tp_before adds to tp; the number of kept entries of one family that count for
    exactly one of their two ends).  A kept entry (i, j) of one family adds 1 to tp[i] when key << 32 | j < first[i] and,
    independently, 1 to tp[j] when key << 32 | i < first[j]."""
    fam, first = np.asarray(fam), np.asarray(first, dtype=np.uint64)
    i, j, key = _kept(t, row0, col0, bound, row_empty, col_empty, cap)
    same = fam[i] == fam[j]
    i, j, key = i[same], j[same], key[same].astype(np.uint64)
    at_i = (key << np.uint64(32) | j.astype(np.uint64)) < first[i]
    at_j = (key << np.uint64(32) | i.astype(np.uint64)) < first[j]
    out = np.bincount(i[at_i], minlength=len(fam)) + np.bincount(j[at_j], minlength=len(fam))
    return out.astype(np.uint32), int((at_i != at_j).sum())
