"""The rule of dct-sim --hac, stated in numpy and Python ints: the oracle of test_linkage_host.py and test_linkage_gpu.py.

Nodes = the n proteins; key(i, j) = min(L1, 17000), L1 = DCTdomain's (the smallest L1 over all fingerprint pairs) or DCTglobal's (the
last fingerprints'); a protein without fingerprints has key 17000 against everything.  A cluster is named by its lowest member
and has a size c.  complete: D(A, B) = max key over the member pairs; average: S(A, B) = the sum, height = S / (cA cB), compared as
an exact fraction (``Fraction`` of Python ints: never floating point).

``rounds``: the definition.  Per round every live cluster a takes nn(a) = the live b != a with D(a, b) <= bound that minimises
(D(a, b), id b); every pair with nn(a) = b and nn(b) = a merges, all at once, under the lower id; the distances of the next round
are the max / the sum over the pre-round clusters.  It ends with the round that merges nothing.
``serial``: the textbook algorithm -- merge the smallest pair under (height, a, b), repeat.
Both return merges as tuples (a, b, num, den, size, round), a < b, height = num / den (den = 1 for complete)."""

from fractions import Fraction

import numpy as np

CAP = 17000
METHODS = ('average', 'complete')
QUOTED = set("(),:;'[]")


def keys_of(dct, idx, score):
    """int64 (n, n) of key(i, j); the diagonal is not used."""
    dct = np.asarray(dct, dtype=np.int64)
    idx = np.asarray(idx, dtype=np.int64)
    n = len(idx) - 1
    key = np.full((n, n), CAP, dtype=np.int64)
    for p in range(n):
        a = dct[idx[p]:idx[p + 1]]
        if not len(a):
            continue
        for q in range(p + 1, n):
            b = dct[idx[q]:idx[q + 1]]
            if not len(b):
                continue
            if score == 'global':
                d = int(np.abs(a[-1] - b[-1]).sum())
            else:
                d = int(np.abs(a[:, None, :] - b[None, :, :]).sum(axis=2).min())
            key[p, q] = key[q, p] = min(d, CAP)
    return key


def _combine(method):
    return np.maximum if method == 'complete' else np.add


def _exact_min(values, weights, ids):
    """The index into ``ids`` of the smallest (values / weights, ids) -- exact: a float64 pass keeps the entries within 1e-12 of the
    smallest quotient (float64 is good to 2e-16), Python ints decide among them."""
    q = values / weights
    near = np.flatnonzero(q <= q.min() * (1 + 1e-12) + 1e-300)
    best = near[0]
    for k in near[1:]:
        l, r = int(values[k]) * int(weights[best]), int(values[best]) * int(weights[k])
        if l < r or (l == r and ids[k] < ids[best]):
            best = k
    return best


def _merge_into(V, size, alive, a, b, comb):
    """Rows, then columns: (a, y) takes (a, y), (b, y) and -- through y's own merge, done the same way -- (a, py), (b, py)."""
    V[a, :] = comb(V[a, :], V[b, :])
    V[:, a] = comb(V[:, a], V[:, b])
    size[a] += size[b]
    size[b] = 0
    alive[b] = False


def rounds(key, bound, method):
    """(merges in the order they were made, number of rounds that merged something)."""
    key = np.asarray(key, dtype=np.int64)
    n = len(key)
    V = key.copy()
    size = np.ones(n, dtype=np.int64)
    alive = np.ones(n, dtype=bool)
    comb = _combine(method)
    merges, rnd = [], 0
    if n < 2 or bound < 0:
        return merges, 0
    while True:
        rnd += 1
        if rnd > n:
            raise RuntimeError('more than n - 1 merging rounds')
        live = np.flatnonzero(alive)
        nn = np.full(n, -1, dtype=np.int64)
        w = size[live] if method == 'average' else np.ones(len(live), dtype=np.int64)
        for r, a in enumerate(live):
            vals = V[a, live]
            ok = (live != a) & (vals <= bound * w[r] * w)
            if ok.any():
                c = np.flatnonzero(ok)
                nn[a] = live[c[_exact_min(vals[c], w[c], live[c])]]
        pairs = [(a, nn[a]) for a in live if nn[a] > a and nn[nn[a]] == a]
        if not pairs:
            return merges, rnd - 1
        made = []
        for a, b in pairs:
            den = int(size[a] * size[b]) if method == 'average' else 1
            made.append((int(a), int(b), int(V[a, b]), den, int(size[a] + size[b]), rnd))
        for a, b in pairs:                      # (all pairs at once: V of a later pair is not read before every row has been merged)
            V[a, :] = comb(V[a, :], V[b, :])
        for a, b in pairs:
            V[:, a] = comb(V[:, a], V[:, b])
            size[a] += size[b]
            size[b] = 0
            alive[b] = False
        merges += made


def serial(key, bound, method):
    """The merges of the textbook algorithm, in the order they are made (round = the merge's number)."""
    key = np.asarray(key, dtype=np.int64)
    n = len(key)
    V = key.copy()
    size = np.ones(n, dtype=np.int64)
    alive = np.ones(n, dtype=bool)
    comb = _combine(method)
    merges = []
    while n >= 2 and bound >= 0:
        live = np.flatnonzero(alive)
        w = size[live] if method == 'average' else np.ones(len(live), dtype=np.int64)
        sub = V[np.ix_(live, live)]
        W = w[:, None] * w[None, :]
        r, c = np.nonzero(np.triu(sub <= bound * W, 1))         # (row-major: (a, b) ascending)
        if not len(r):
            break
        k = _exact_min(sub[r, c], W[r, c], np.arange(len(r)))
        a, b = live[r[k]], live[c[k]]
        merges.append((int(a), int(b), int(V[a, b]), int(W[r[k], c[k]]), int(size[a] + size[b]), len(merges) + 1))
        _merge_into(V, size, alive, a, b, comb)
    return merges


def height(m):
    return Fraction(m[2], m[3])


def ordered(merges):
    """Merge order: (height exact, round, a)."""
    return sorted(merges, key=lambda m: (height(m), m[5], m[0]))


def labels_at(n, merges, bound):
    """labels[i] = the lowest member of i's cluster after the merges of height <= bound (a replay in merge order)."""
    lab = np.arange(n, dtype=np.int64)
    for a, b, num, den, _size, _rnd in ordered(merges):
        if num <= bound * den:
            la, lb = lab[a], lab[b]
            lab[lab == max(la, lb)] = min(la, lb)
    return lab


def sizes_of(labels):
    return sorted(np.bincount(labels)[np.unique(labels)].tolist(), reverse=True)


def similarity_text(num, den):
    return f'{1 - num / (CAP * den):.4f}'


def text(sid, merges) -> bytes:
    lines = ['#rep1 rep2 similarity size']
    for a, b, num, den, size, _rnd in ordered(merges):
        lines.append(f'{sid[a]} {sid[b]} {similarity_text(num, den)} {size}')
    return ''.join(x + '\n' for x in lines).encode('utf8')


def flat_text(sid, labels) -> bytes:
    order = np.argsort(labels, kind='stable')
    return ''.join(f'{sid[labels[i]]} {sid[i]}\n' for i in order).encode('utf8')


def quoted(name) -> str:
    name = str(name)
    if any(ch in QUOTED or ch.isspace() for ch in name):
        return "'" + name.replace("'", "''") + "'"
    return name


def newick(sid, merges) -> bytes:
    """One tree per line in id order; (A:la,B:lb) with the lower id first, branch = (height - the child's height) / 17000."""
    n = len(sid)
    node = {i: (quoted(sid[i]), Fraction(0)) for i in range(n)}
    for m in ordered(merges):
        a, b, h = m[0], m[1], height(m)
        (ta, ha), (tb, hb) = node[a], node.pop(b)
        la, lb = (h - ha) / CAP, (h - hb) / CAP
        node[a] = (f'({ta}:{la.numerator / la.denominator:.6f},{tb}:{lb.numerator / lb.denominator:.6f})', h)
    return ''.join(node[i][0] + ';\n' for i in sorted(node)).encode('utf8')
