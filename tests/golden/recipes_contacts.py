"""Seed-defined synthetic contact maps (float32, symmetric) for the domain-prediction tests."""

import numpy as np


def make_contacts(recipe: str, L: int, seed: int, nb: int = 3) -> np.ndarray:
    rng = np.random.default_rng(seed)
    i = np.arange(L)[:, None]
    j = np.arange(L)[None, :]
    near = 0.9 * np.exp(-np.abs(i - j) / 12.0)
    if recipe in ('blocks', 'interleaved'):
        nb = max(1, nb)
        lab = (np.arange(L) * nb // max(L, 1))
        if recipe == 'interleaved' and nb >= 3:
            lab = np.where(lab == nb - 1, 0, lab)          # last block folds onto the first: discontinuous domain
        same = lab[i] == lab[j]
        if recipe == 'interleaved':
            p = 0.6 * near + 0.9 * (rng.random((L, L)) < 0.12) * same * (0.6 + 0.4 * rng.random((L, L)))
        else:
            p = near + 0.3 * rng.random((L, L)) * same
    elif recipe == 'ties':
        p = np.round((near + 0.3 * rng.random((L, L))) * 8) / 8.0
    elif recipe == 'sparse':
        p = near * (np.abs(i - j) < 30) * (rng.random((L, L)) < 0.2)
    elif recipe == 'flat':
        p = np.full((L, L), 0.25)
    elif recipe == 'negzero':
        p = np.where(rng.random((L, L)) < 0.5, -0.0, 0.0) + (rng.random((L, L)) < 0.05) * 0.5
    else:
        raise KeyError(recipe)
    p = 0.5 * (p + p.T)
    return np.ascontiguousarray(p, dtype=np.float32)


def fuzz_graphs(seed: int = 20240, n: int = 120):
    """Random block / interleaved contact graphs (blocks merged at random: discontinuous domains), as the selection of
    writece would pass them on: yields (L, i, j, v) with at most int(2.6 L) contacts, strongest first."""
    rng = np.random.default_rng(seed)
    for _ in range(n):
        L = int(rng.integers(22, 360))
        nb = int(rng.integers(1, 8))
        bounds = np.sort(rng.choice(np.arange(1, L), size=min(nb - 1, L - 1), replace=False)) if nb > 1 else []
        lab = np.zeros(L, int)
        for b in bounds:
            lab[b:] += 1
        for _m in range(int(rng.integers(0, 3))):
            if nb >= 3:
                a, b = sorted(rng.choice(nb, 2, replace=False))
                lab[lab == b] = a
        same = lab[:, None] == lab[None, :]
        p = rng.random((L, L)) * (same * rng.uniform(0.5, 1.0) + (~same) * rng.uniform(0.0, 0.3))
        mask = np.triu(rng.random((L, L)) < rng.uniform(0.02, 0.3), 5)
        ii, jj = np.nonzero(mask)
        t = int(2.6 * L)
        if len(ii) > t:
            order = np.argsort(-p[ii, jj], kind='stable')[:t]
            ii, jj = ii[order], jj[order]
        yield L, ii, jj, p[ii, jj].astype(np.float32)


def weight_class_graphs(seed: int = 4711, n: int = 60):
    """Block contact graphs whose weights leave 0 .. 255, the range of a probability: some contacts negative (weight below 0,
    or rounded to 0 from just under 0) and some at 2.555 and above (weight 256 and up), all finite.  Yields (L, i, j, v) as
    fuzz_graphs does, up to 4 L contacts, strongest first; what the reference's cutter makes of such a .ce file is
    tests/golden/reccut_weights_golden.json."""
    rng = np.random.default_rng(seed)
    for g in range(n):
        L = int(rng.integers(22, 300))
        nb = int(rng.integers(1, 6))
        bounds = np.sort(rng.choice(np.arange(1, L), size=min(nb - 1, L - 1), replace=False)) if nb > 1 else []
        lab = np.zeros(L, int)
        for b in bounds:
            lab[b:] += 1
        same = lab[:, None] == lab[None, :]
        p = rng.random((L, L)) * (same * rng.uniform(0.5, 1.0) + (~same) * rng.uniform(0.0, 0.3))
        mask = np.triu(rng.random((L, L)) < rng.uniform(0.05, 0.3), 1)
        ii, jj = np.nonzero(mask)
        t = int(rng.uniform(1.0, 4.0) * L)
        if len(ii) > t:
            order = np.argsort(-p[ii, jj], kind='stable')[:t]
            ii, jj = ii[order], jj[order]
        v = p[ii, jj]
        u = rng.random(len(v))
        neg, big = (0.05, 0.3) if g % 3 else (0.3, 0.05)
        v = np.where(u < neg, -rng.uniform(0.0, 1.5, len(v)), v)                               # below 0 (and -0.0149 .. 0: weight 0)
        v = np.where((u >= neg) & (u < neg + big), 2.555 + rng.uniform(0.0, 40.0, len(v)), v)  # weight 256 and up
        v = np.where((u >= neg + big) & (u < neg + big + 0.02), -rng.uniform(0.0, 0.0149, len(v)), v)
        yield L, ii.astype(np.int32), jj.astype(np.int32), v.astype(np.float32)
