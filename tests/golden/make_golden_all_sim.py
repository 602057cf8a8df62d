"""Writes the all-against-all golden: a synthetic ``-dct.npz`` and what the reference's ``src/dct-sim.py`` prints for
``all_sim`` on it (the file its main() leaves in --output: the header, then every pair of the upper triangle).

    python tests/golden/make_golden_all_sim.py /path/to/DCTdomain-checkout

The reference module is imported on the CPU through importlib and run as it stands.  Every fingerprint byte lies in
[-63, 63], so the reference's int8 differences cannot wrap.  The data covers what the streamed GPU text must reproduce:
duplicated proteins (ties), planted L1 values of exactly 17000, 17001 and far above, planted values on both sides of a
last-digit rounding boundary of ``.3f`` (1 - L1 / 17000 crosses x.xxx5 between L1 = 17 k + 8 and 17 k + 9), and ids that are
non-ASCII, one byte long and 300 bytes or more.  Every protein has at least one fingerprint (the reference's domain_sim has
no answer for an empty one).  Output: tests/golden/all_sim/ -- all-dct.npz and expected.txt.gz."""

from __future__ import annotations

import contextlib
import gzip
import io
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden_protein_search import load_reference, save_npz  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'all_sim')
D = 480

#: planted L1 values from one base protein: the 17000 edge, far beyond it, and .3f rounding boundaries (17 k + 8 / 17 k + 9)
PLANTED = [17000, 17001, 17002, 25000, 0, 8, 9, 25, 26, 8500, 8508, 8509, 12750, 12758, 12759, 16983, 16991, 16992, 16999]


def plant(q: np.ndarray, l1: int) -> np.ndarray:
    """A row at exactly L1 = l1 from q (|q| <= 10): every byte moved across zero and away, within [-63, 63]."""
    base, rem = divmod(int(l1), D)
    mags = base + (np.arange(D) < rem)
    out = q.astype(np.int64) + np.where(q < 0, 1, -1) * mags
    assert np.abs(out).max() <= 63 and np.abs(out - q).sum() == l1
    return out.astype(np.int8)


def make_data(seed: int = 23):
    rng = np.random.default_rng(seed)
    centers = rng.integers(-40, 41, size=(6, D))

    def family_row(f):
        return np.clip(centers[f] + rng.integers(-9, 10, size=D), -63, 63).astype(np.int8)

    prots, names = [], []
    for k in range(110):
        if k % 7 == 6:                                       # unrelated proteins
            prots.append(rng.integers(-63, 64, size=(1 + rng.integers(0, 3), D)).astype(np.int8))
        else:
            prots.append(np.stack([family_row(k % 6) for _ in range(int(rng.integers(0, 4)) + 1)]))
        names.append(f'p{k:03d}')
    for k in (2, 9, 50):                                     # exact duplicates: ties
        prots.append(prots[k].copy())
        names.append(f'dup{k:03d}')
    q = rng.integers(-10, 11, size=D).astype(np.int8)
    prots.append(q[None, :])
    names.append('base')
    for l1 in PLANTED:
        dom = plant(q, l1 + 40 if l1 < 17000 else 17001)     # a domain further away than the whole protein
        prots.append(np.stack([dom, plant(q, l1)]))
        names.append(f'pl{l1}')
    for name in ('x', 'é', 'protéine_αβγ', '蛋白質', 'L' * 300, 'M' * 150 + 'ü' * 100):
        prots.append(np.stack([family_row(len(name) % 6) for _ in range(2)]))
        names.append(name)
    order = np.random.default_rng(seed + 1).permutation(len(prots))   # odd ids and plants spread over the triangle
    return [names[k] for k in order], [prots[k] for k in order]


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) != 1:
        raise SystemExit(__doc__)
    ref = load_reference(argv[0])
    os.makedirs(OUT, exist_ok=True)
    names, prots = make_data()
    npz = os.path.join(OUT, 'all-dct.npz')
    save_npz(npz, names, prots)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'out.txt')
        with open(path, 'w', encoding='utf8') as fh:
            fh.write('#prot1 prot2 sim-domain sim-global\n')
        with contextlib.redirect_stdout(io.StringIO()):
            ref.all_sim(npz, path)
        text = open(path, 'rb').read()
    with open(os.path.join(OUT, 'expected.txt.gz'), 'wb') as fh:
        fh.write(gzip.compress(text, mtime=0))
    print(len(names), 'proteins', text.count(b'\n') - 1, 'lines')


if __name__ == '__main__':
    main()
