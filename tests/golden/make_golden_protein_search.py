"""Writes the protein-search goldens: two synthetic ``-dct.npz`` files (queries, database), a pair list, and what the
reference's ``src/dct-sim.py`` prints for ``db_search`` and ``pair_sim`` on them.

    python tests/golden/make_golden_protein_search.py /path/to/DCTdomain-checkout

The reference module is imported on the CPU through importlib (its file name has a hyphen) and run as it stands.  The data
covers what the GPU path must reproduce: exact L1 ties (duplicated proteins), L1 beyond 17000 (similarity 0, database order),
a hit at exactly the 0.25 bound (L1 12750, sim 0.25) next to one just past it (12751), top larger than the database, and the
thresholds 0, 0.25 and 1.5.  Every protein has at least one fingerprint: the reference's domain_sim has no answer for an
empty one.  Output: tests/golden/protein_search/ -- the two npz files and expected.json.gz (the pair list, and per run its
arguments and the reference's output text; compressed, since two of the runs print every query x database pair)."""

from __future__ import annotations

import contextlib
import gzip
import importlib.util
import io
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'protein_search')
D = 480

#: (top, threshold) of every db_search golden
RUNS = [(5, 0.25), (5, 0.0), (5, 1.5), (1000, 0.25), (3, 0.5)]


def plant(q: np.ndarray, l1: int) -> np.ndarray:
    """A row at exactly L1 = l1 from q (|q| <= 60, l1 <= 480 * 67): every byte moved away from its bound."""
    base, rem = divmod(int(l1), D)
    mags = base + (np.arange(D) < rem)
    signs = np.where(q < 0, 1, -1)
    out = q.astype(np.int64) + signs * mags
    assert np.abs(out).max() <= 127 and np.abs(out - q).sum() == l1
    return out.astype(np.int8)


def make_data(seed: int = 11):
    rng = np.random.default_rng(seed)
    centers = rng.integers(-60, 61, size=(8, D))

    def family_row(f):
        return np.clip(centers[f] + rng.integers(-9, 10, size=D), -60, 60).astype(np.int8)

    def protein(f, n_dom):
        return np.stack([family_row(f) for _ in range(n_dom)] + [family_row(f)])

    db, db_names = [], []
    for k in range(150):                                   # family members and unrelated wide-range proteins
        if k % 5 == 4:
            p = rng.integers(-128, 128, size=(1 + rng.integers(0, 4), D)).astype(np.int8)
        else:
            p = protein(k % 8, int(rng.integers(0, 5)))
        db.append(p)
        db_names.append(f'db{k:03d}')
    for k in (3, 17, 40):                                   # exact duplicates: ties on every query
        db.append(db[k].copy())
        db_names.append(f'dup{k:03d}')
    queries, q_names = [], []
    for k in range(24):
        queries.append(protein(k % 8, int(rng.integers(0, 4))))
        q_names.append(f'q{k:02d}')
    for k in range(4):                                      # planted last-row distances around the bounds
        q = rng.integers(-60, 61, size=D).astype(np.int8)
        queries.append(np.stack([q]))
        q_names.append(f'planted{k}')
        for l1 in (3000, 5000, 5000, 9000, 12749, 12750, 12751, 16999, 17000, 17001, 20000):
            last = plant(q, l1)
            dom = plant(q, max(0, l1 - 2000 - 97 * k))      # a domain closer than the whole protein
            db.append(np.stack([dom, last]))
            db_names.append(f'pl{k}_{l1}_{len(db)}')
    return (q_names, queries), (db_names, db)


def save_npz(path, names, prots):
    idx = np.concatenate([[0], np.cumsum([len(p) for p in prots])]).astype(np.int64)
    dct = np.concatenate(prots).astype(np.int8)
    np.savez(path, sid=np.array(names), idx=idx, dom=np.array(['1-9'] * len(dct)), dct=dct)


def load_reference(checkout: str):
    spec = importlib.util.spec_from_file_location('ref_dct_sim', os.path.join(checkout, 'src', 'dct-sim.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_quiet(fn, *args):
    with contextlib.redirect_stdout(io.StringIO()):
        fn(*args)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) != 1:
        raise SystemExit(__doc__)
    ref = load_reference(argv[0])
    os.makedirs(OUT, exist_ok=True)
    (qn, qp), (dn, dp) = make_data()
    qf, dbf = os.path.join(OUT, 'query-dct.npz'), os.path.join(OUT, 'db-dct.npz')
    save_npz(qf, qn, qp)
    save_npz(dbf, dn, dp)
    rng = np.random.default_rng(5)
    lines = ['# pairs of db-dct.npz: repeats, a protein with itself, unknown ids\n']
    for _ in range(300):
        i, j = rng.integers(0, len(dn), size=2)
        lines.append(f'{dn[i]} {dn[j]}\n')
    lines += [f'{dn[7]} {dn[7]}\n', f'{dn[7]} {dn[7]}\n', f'nosuch {dn[1]}\n', f'{dn[2]} nosuch extra words\n', '# end\n']
    runs = []
    with tempfile.TemporaryDirectory() as tmp:
        def output(fn, *args):
            """What the reference's main() leaves in --output: the header, then the mode's lines (appended)."""
            path = os.path.join(tmp, 'out.txt')
            with open(path, 'w') as fh:
                fh.write('#prot1 prot2 sim-domain sim-global\n')
            run_quiet(fn, *args, path)
            return open(path).read()
        for top, thr in RUNS:
            runs.append({'mode': 'db', 'top': top, 'threshold': thr, 'expected': output(ref.db_search, qf, dbf, top, thr)})
        pairf, found = os.path.join(tmp, 'db.pair'), os.path.join(tmp, 'found.txt')
        with open(pairf, 'w') as fh:
            fh.writelines(lines)
        text = output(ref.pair_sim, dbf, pairf, found)
        runs.append({'mode': 'pair', 'expected': text, 'pairfound': open(found).read()})
    blob = json.dumps({'pairs': ''.join(lines), 'runs': runs}, indent=1).encode()
    with open(os.path.join(OUT, 'expected.json.gz'), 'wb') as fh:
        fh.write(gzip.compress(blob, mtime=0))
    for r in runs:
        print(r['mode'], r.get('top'), r.get('threshold'), r['expected'].count('\n'), 'lines')


if __name__ == '__main__':
    main()
