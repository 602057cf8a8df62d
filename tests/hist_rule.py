"""The rule of dct-sim --hist, stated in numpy and plain Python: the oracle of test_hist_host.py (where it is worked by hand and
pinned on the committed reference fixture) and test_hist_gpu.py.  Written without a look at dct_sim.

Every unordered pair i < j of the proteins of a file has a key = min(L1, 17000) -- L1 the smallest over all fingerprint pairs
(DCTdomain) or that of the two last fingerprints (DCTglobal), 0x7fffffff where a protein has none -- and, with a family per protein,
a class: 0 when the two are of one family, 1 when not (one class, 0, without families).  With bound = 16999, or the bound of a
cut-off when that is lower:
- hist[cls][key] counts the pairs of key <= bound, rest[cls] the others;
- cut-off b of `bins` is the text '%.4f' % ((bins - 1 - b) / bins); a pair is kept at it unless similarity < float(text), the
  reference's own comparison (all_sim_filter_rule.kept); the last, 0.0000, keeps every pair; with a cut-off X of the run the lines
  below X are left out, except the last;
- roc_auc = P(a same-family pair scores above an other-family pair) + P(tie) / 2, the pairs of `rest` tied at the bottom;
- best_f1 = the largest 2 kept_same / (kept_same + kept_other + same) over the integer bounds 0 .. bound, ties to the lowest."""

from fractions import Fraction

import numpy as np

import all_sim_filter_rule as rule

CAP = 17000
BOUND_ALL = CAP - 1


# ---- what one int32 tile contributes, as the kernel scans it (entries as all_sim_filter_rule.tile_keep keeps them)

def tile_hist(t, row0, col0, bound, fam=None, row_empty=None, col_empty=None, cap=CAP):
    """uint64 (1 or 2, cap + 1): what dctfp_tri_hist adds to hist -- 1 at [cls, key] for every kept entry."""
    keep, key = rule.tile_keep(t, row0, col0, bound, row_empty, col_empty, cap)
    r, c = np.nonzero(keep)
    if fam is None:
        cls, classes = np.zeros(len(r), dtype=np.int64), 1
    else:
        fam = np.asarray(fam)
        cls, classes = (fam[row0 + r] != fam[col0 + c]).astype(np.int64), 2
    out = np.zeros((classes, cap + 1), dtype=np.uint64)
    np.add.at(out, (cls, key[r, c]), np.uint64(1))
    return out


# ---- the counts of a file from the keys of its pairs

def sim_edge(threshold: float) -> int:
    """The largest L1 in 0 .. 17000 that is kept at a cut-off (-1: none), by the reference's comparison on every L1."""
    return int(np.count_nonzero(~(rule.similarity(np.arange(CAP + 1)) < threshold))) - 1


def of_keys(key, cls=None, min_cut=None):
    """(hist, rest) of the pairs with keys ``key`` (any L1 values) and classes ``cls`` (None: one class): uint64 (classes, bound + 1)
    and uint64 (classes)."""
    key = np.minimum(np.asarray(key, dtype=np.int64), CAP)
    bound = BOUND_ALL if min_cut is None else min(sim_edge(min_cut), BOUND_ALL)
    classes = 1 if cls is None else 2
    cls = np.zeros(len(key), dtype=np.int64) if cls is None else np.asarray(cls, dtype=np.int64)
    hist = np.zeros((classes, max(bound + 1, 0)), dtype=np.uint64)
    rest = np.zeros(classes, dtype=np.uint64)
    for c in range(classes):
        mine = key[cls == c]
        within = mine[mine <= bound]
        hist[c] = np.bincount(within, minlength=bound + 1).astype(np.uint64) if bound >= 0 else hist[c]
        rest[c] = len(mine) - len(within)
    return hist, rest


def of_file(dct, idx, fam=None, score='domain', min_cut=None, triangle=None):
    """(hist, rest) of a file; ``triangle``: all_sim_filter_rule.triangle_l1 of it, where the caller has it."""
    i, j, mn, last = triangle if triangle is not None else rule.triangle_l1(dct, idx)
    cls = None if fam is None else (np.asarray(fam)[i] != np.asarray(fam)[j])
    return of_keys(mn if score == 'domain' else last, cls, min_cut)


# ---- the table and the summary from the counts

def cut_texts(bins: int) -> list:
    return ['%.4f' % ((bins - 1 - b) / bins) for b in range(bins)]


def table(hist, rest, bins: int, min_cut=None):
    """[(text, kept per class)]: the pairs not below each printed cut-off, as Python integers."""
    classes, width = hist.shape
    total = [int(hist[c].sum()) + int(rest[c]) for c in range(classes)]
    out = []
    for b, text in enumerate(cut_texts(bins)):
        if b == bins - 1:
            out.append((text, total))
            continue
        if min_cut is not None and float(text) < min_cut:
            continue
        edge = min(sim_edge(float(text)), width - 1)
        out.append((text, [int(hist[c][:edge + 1].sum()) for c in range(classes)]))
    return out


def roc_auc(hist, rest):
    """Mann-Whitney with ties counted half, over the bins and the rest as one last bin; None when a class is empty."""
    same = [int(v) for v in hist[0]] + [int(rest[0])]
    other = [int(v) for v in hist[1]] + [int(rest[1])]
    if sum(same) == 0 or sum(other) == 0:
        return None
    wins, behind = Fraction(0), 0                                 # (behind = the other-family pairs of a larger key)
    for s, o in zip(reversed(same), reversed(other)):
        wins += s * (behind + Fraction(o, 2))
        behind += o
    return float(wins / (sum(same) * sum(other)))


def best_f1(hist, rest):
    """(F1, bound) of the best integer bound, ties to the lowest; (None, None) without a same-family pair or a bound."""
    n_same = int(hist[0].sum()) + int(rest[0])
    if n_same == 0 or hist.shape[1] == 0:
        return None, None
    ks, ko = np.cumsum(hist[0].astype(np.int64)), np.cumsum(hist[1].astype(np.int64))
    f1 = [Fraction(2 * int(a), int(a) + int(b) + n_same) for a, b in zip(ks, ko)]
    b = max(range(len(f1)), key=lambda k: (f1[k], -k))
    return float(f1[b]), b


def at_text(b: int) -> str:
    return '%.6f' % (1 - (b + 0.5) / CAP)


def summary(hist, rest) -> dict:
    pairs = int(hist.sum()) + int(rest.sum())
    if hist.shape[0] == 1:
        return {'pairs': pairs, 'scored': int(hist.sum())}
    f1, b = best_f1(hist, rest)
    return {'pairs': pairs, 'same': int(hist[0].sum()) + int(rest[0]), 'other': int(hist[1].sum()) + int(rest[1]), 'roc_auc': roc_auc(hist, rest),
            'best_f1': f1, 'at': None if b is None else at_text(b)}


def header(score: str, families: bool) -> bytes:
    return (f'#min-{score} same other kept-same kept-other recall precision fpr\n' if families else f'#min-{score} pairs kept\n').encode()


def _rate(a, b):
    return '%.4f' % (a / b) if b else '-'


def text(hist, rest, bins: int, min_cut=None) -> bytes:
    """The lines behind the header."""
    classes = hist.shape[0]
    total = [int(hist[c].sum()) + int(rest[c]) for c in range(classes)]
    lines, before = [], [0] * classes
    for cut, kept in table(hist, rest, bins, min_cut):
        step = [k - p for k, p in zip(kept, before)]
        if classes == 1:
            lines.append(f'{cut} {step[0]} {kept[0]}')
        else:
            lines.append(' '.join([cut, str(step[0]), str(step[1]), str(kept[0]), str(kept[1]), _rate(kept[0], total[0]),
                                   _rate(kept[0], kept[0] + kept[1]), _rate(kept[1], total[1])]))
        before = kept
    s = summary(hist, rest)
    if classes == 1:
        lines.append(f'# pairs={s["pairs"]} scored={s["scored"]}')
    else:
        auc = '-' if s['roc_auc'] is None else '%.4f' % s['roc_auc']
        f1 = '-' if s['best_f1'] is None else '%.4f' % s['best_f1']
        lines.append(f'# pairs={s["pairs"]} same={s["same"]} other={s["other"]} roc_auc={auc} best_f1={f1} at={s["at"] or "-"}')
    return ('\n'.join(lines) + '\n').encode()
