"""dct-sim --auc1 without a GPU: the numpy rule (auc1_rule.py) worked by hand and pinned on the committed reference fixture, the
top-1 argument against an independently computed best hit, the summary, the family readers, the command-line rules, the text,
and the new exports' place in the build."""

import contextlib
import io
import os
import re

import numpy as np
import pytest

import all_sim_filter_rule as rule
import auc1_rule as ar
import cluster_rule
import golden_util as gu
import medoid_rule as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G6PD = os.path.join(gu.GOLD, 'ref_fixtures', 'G6PD-dct.npz')


@pytest.fixture(scope='module')
def g6pd():
    with np.load(G6PD) as data:
        sid, idx, dct = [str(s) for s in data['sid']], data['idx'], data['dct']
    tri = rule.triangle_l1(dct, idx)
    return sid, idx, dct, tri, cluster_rule.labels(dct, idx, min_global=0.6)[0]


# ---- 1. the rule

X = 17000            # no hit: a pair of similarity 0, or a protein without fingerprints
HAND_FAM = ['a', 'b', 'a', 'a', 'b', 'c']
HAND_KEYS = np.array([[0, 500, 200, 700, X, 200],
                      [500, 0, 400, X, X, X],
                      [200, 400, 0, 400, X, 800],
                      [700, X, 400, 0, X, X],
                      [X, X, X, X, 0, X],
                      [200, X, 800, X, X, 0]])
HAND_SID = ['p0', 'p1', 'p2', 'p3', 'p4', 'p5']


def test_the_rule_by_hand():
    """Six proteins, families a = {0, 2, 3}, b = {1, 4}, c = {5}; protein 4 has no fingerprints (17000 to everyone).
    0: hits (200, 2) (200, 5) (500, 1) (700, 3).  2 is of its family and 5 is not, at the SAME key: the lower index goes first,
       so 2 is counted and 5 is the first false positive -- tp 1 of 2, AUC1 0.5.
    1: hits (400, 2) (500, 0), both of family a: first false positive 2, tp 0; its only relative, 4, is no hit.
    2: hits (200, 0) (400, 1) (400, 3) (800, 5).  1 is of another family and 3 of its own, at the same key, the other way round by
       index: 1 goes first and ends the walk, 3 is not counted -- tp 1, first false positive 1 at 400.
    3: hits (400, 2) (700, 0), both of its family and nobody else: no false positive, tp 2, AUC1 1.
    4: no hit at all: tp 0, no false positive; still a query (its family has two members): AUC1 0.
    5: a family of one: hits (200, 0) (800, 2), tp 0, AUC1 0 and no query."""
    assert np.array_equal(HAND_KEYS, HAND_KEYS.T)
    tp, fp_index, fp_key = ar.of_keys(HAND_KEYS, HAND_FAM)
    assert tp.tolist() == [1, 0, 1, 2, 0, 0]
    assert fp_index.tolist() == [5, 2, 1, -1, -1, 0]
    assert fp_key.tolist() == [200, 400, 400, X, X, 200]
    assert ar.auc1(tp, HAND_FAM).tolist() == [0.5, 0.0, 0.5, 1.0, 0.0, 0.0]
    s = ar.summary(tp, HAND_FAM)
    assert s['queries'] == 5 and s['families'] == 2
    assert s['mean_auc1'] == pytest.approx(0.4) and s['top1_raw'] == pytest.approx(0.6) and s['top1_norm'] == pytest.approx(0.5)
    # a cut-off: bound 450 leaves 0: (200, 2) (200, 5); 1: (400, 2); 2: (200, 0) (400, 1) (400, 3); 3: (400, 2); 5: (200, 0)
    tp, fp_index, fp_key = ar.of_keys(HAND_KEYS, HAND_FAM, 450)
    assert tp.tolist() == [1, 0, 1, 1, 0, 0] and fp_index.tolist() == [5, 2, 1, -1, -1, 0]
    # bound 17000: everybody is a hit of everybody, protein 4 included
    tp, fp_index, fp_key = ar.of_keys(HAND_KEYS, HAND_FAM, X)
    assert tp.tolist() == [1, 0, 1, 2, 0, 0] and fp_index.tolist() == [5, 2, 1, 1, 0, 0] and fp_key.tolist() == [200, 400, 400, X, X, 200]
    # below 0: nobody
    tp, fp_index, fp_key = ar.of_keys(HAND_KEYS, HAND_FAM, -1)
    assert not tp.any() and (fp_index == -1).all() and (fp_key == X).all()


def test_the_tile_rules_add_up_to_the_brute_force():
    """The two per-tile rules over the whole triangle in one tile (rows 0 .. n - 2 against columns 1 .. n - 1) are of_keys."""
    fam = np.array([0, 1, 0, 0, 1, 2])
    t = HAND_KEYS[:5, 1:].astype(np.int32)
    for bound in (ar.BOUND_ALL, 450, X, -1):
        first = ar.tile_first_fp(t, 0, 1, bound, fam)
        tp, split = ar.tile_tp_before(t, 0, 1, bound, fam, first)
        want = ar.of_keys(HAND_KEYS, fam, bound)
        none = first == np.uint64(ar.NONE)
        assert np.array_equal(tp, want[0])
        assert np.array_equal(np.where(none, -1, first & np.uint64(0xffffffff)).astype(np.int64), want[1])
        assert np.array_equal(np.where(none, X, first >> np.uint64(32)).astype(np.int64), want[2])
    # the pairs (0, 3) at 700 and (2, 3) at 400 count for 3 (no false positive) and not for 0 (first false positive (200, 5)) or
    # 2 ((400, 1)): the two ends of an entry are decided separately
    first = ar.tile_first_fp(t, 0, 1, ar.BOUND_ALL, fam)
    assert ar.tile_tp_before(t, 0, 1, ar.BOUND_ALL, fam, first)[1] == 2


def test_the_rule_on_the_reference_fixture(g6pd):
    sid, idx, dct, tri, fam = g6pd
    assert sorted(np.bincount(fam)[np.unique(fam)].tolist()) == [1, 6, 7, 13]
    tp, fp_index, fp_key = ar.of_file(dct, idx, fam, 'global', triangle=tri)
    s = ar.summary(tp, fam)
    assert s['queries'] == 26 and s['families'] == 3
    assert '%.4f' % s['mean_auc1'] == '1.0000' and '%.4f' % s['top1_raw'] == '1.0000'
    tp, fp_index, fp_key = ar.of_file(dct, idx, fam, 'domain', triangle=tri)
    s = ar.summary(tp, fam)
    assert s['queries'] == 26 and s['families'] == 3
    assert '%.4f' % s['mean_auc1'] == '0.7596' and '%.4f' % s['top1_raw'] == '0.9615'
    assert tp[:6].tolist() == [6, 5, 5, 8, 8, 8] and tp[17] == 0 and fp_index[0] == 6
    # the tie rule is exercised: 29 pairs of neighbours in the ranked lists share a key
    K = mr.key_matrix(dct, idx, 'domain', tri)
    ties = 0
    for x in range(27):
        ranked = sorted(int(K[x, y]) for y in range(27) if y != x and K[x, y] <= ar.BOUND_ALL)
        ties += sum(1 for a, b in zip(ranked, ranked[1:]) if a == b)
    assert ties == 29
    # a cut-off: only the hits within it
    for score, cut in (('domain', 0.8), ('global', 0.6), ('domain', 1.5)):
        from dctdomain_amd.dct_sim import sim_bound
        got = ar.of_file(dct, idx, fam, score, min_cut=cut, triangle=tri)
        assert (got[2][got[1] >= 0] <= sim_bound(cut)).all()
        assert (got[0] <= ar.of_file(dct, idx, fam, score, triangle=tri)[0]).all()
    assert not ar.of_file(dct, idx, fam, 'domain', min_cut=1.5, triangle=tri)[0].any()


def _random_case(rng, n, families, ties=True):
    K = rng.integers(0, 40 if ties else 16000, size=(n, n)) * (400 if ties else 1)
    K[rng.random((n, n)) < 0.15] = X
    K = np.triu(K, 1)
    K = K + K.T
    if n:
        K[0, :] = K[:, 0] = X                                     # (a protein without fingerprints: no hit at all)
    return K, rng.integers(0, families, size=n)


def test_tp_of_one_means_the_best_hit_is_of_the_family():
    rng = np.random.default_rng(3)
    seen = set()
    for n, families, bound in ((30, 4, ar.BOUND_ALL), (30, 12, 8000), (17, 2, 6000), (25, 25, ar.BOUND_ALL), (25, 1, ar.BOUND_ALL), (40, 6, 3000)):
        K, fam = _random_case(rng, n, families)
        tp, fp_index, fp_key = ar.of_keys(K, fam, bound)
        for x in range(n):
            # the best hit on its own: the smallest (key, y) over y != x within the bound
            best = min(((int(K[x, y]), y) for y in range(n) if y != x and K[x, y] <= bound), default=None)
            good = best is not None and fam[best[1]] == fam[x]
            assert (tp[x] >= 1) == good
            seen.add((best is None, good))
            if best is not None and not good:
                assert (fp_key[x], fp_index[x]) == best
    assert seen == {(True, False), (False, True), (False, False)}


def test_the_summary_arithmetic():
    from dctdomain_amd import dct_sim
    rng = np.random.default_rng(11)
    for n, families in ((30, 4), (40, 25), (12, 12), (9, 1), (1, 1), (0, 1)):
        K, fam = _random_case(rng, n, families)
        tp = ar.of_keys(K, fam)[0]
        dense, names = dct_sim.dense_families([f'f{v}' for v in fam])
        assert dense.dtype == np.int32 and [names[c] for c in dense] == [f'f{v}' for v in fam] and len(names) == len(set(fam.tolist()))
        want, got = ar.summary(tp, fam), dct_sim.auc1_summary(tp, dense)
        assert set(got) == {'queries', 'families', 'mean_auc1', 'top1_raw', 'top1_norm'}
        assert got['queries'] == want['queries'] and got['families'] == want['families']
        for k in ('mean_auc1', 'top1_raw', 'top1_norm'):
            assert got[k] == pytest.approx(want[k], abs=1e-12), k
        a = dct_sim.auc1_of_counts(tp, dense)
        assert a.dtype == np.float64 and np.allclose(a, ar.auc1(tp, fam), atol=1e-15)
    # Qnorm weighs families, Qraw queries: a family of 4 all right and a family of 2 all wrong; the family of one is no query
    tp, fam = np.array([1, 2, 3, 1, 0, 0, 5]), np.array([0, 0, 0, 0, 1, 1, 2])
    s = dct_sim.auc1_summary(tp, fam)
    assert s['queries'] == 6 and s['families'] == 2 and s['top1_raw'] == pytest.approx(4 / 6) and s['top1_norm'] == pytest.approx(0.5)
    assert s['mean_auc1'] == pytest.approx((1 / 3 + 2 / 3 + 1 + 1 / 3) / 6)
    assert dct_sim.auc1_of_counts(tp, fam)[6] == 0.0


# ---- 2. the families

def test_the_family_file(tmp_path):
    from dctdomain_amd import dct_sim
    sid = np.array(['p0', 'p1', 'p2'])
    path = tmp_path / 'fam.txt'
    path.write_text('# id family\n\np1\t3.30.930.10\n  p0   1.10.8.10  \nother 9.9.9.9\np2 1.10.8.10\np1 3.30.930.10\n')
    assert dct_sim.read_families(str(path), sid) == ['1.10.8.10', '3.30.930.10', '1.10.8.10']
    path.write_text('p0 a\np2 a\nq b\n')
    with pytest.raises(ValueError, match='gives no family for p1'):
        dct_sim.read_families(str(path), sid)
    path.write_text('p0 a\np1 a\np2 a\np1 b\n')
    with pytest.raises(ValueError, match='line 4: p1 is given two families, a and b'):
        dct_sim.read_families(str(path), sid)
    path.write_text('p0 a\np1\n')
    with pytest.raises(ValueError, match='line 2: a line is "id family"'):
        dct_sim.read_families(str(path), sid)
    path.write_text('p0 a\np1 a b\n')
    with pytest.raises(ValueError, match='line 2'):
        dct_sim.read_families(str(path), sid)


def test_the_family_in_the_id():
    from dctdomain_amd import dct_sim
    assert dct_sim.families_from_ids(np.array(['16vpA00|3.30.930.10', '1abcA01|1.10.8.10|x']), '|') == ['3.30.930.10', '1.10.8.10|x']
    assert dct_sim.families_from_ids(['a__f1', 'b__f2'], '__') == ['f1', 'f2']
    with pytest.raises(ValueError, match='the id 1abcA01 has no'):
        dct_sim.families_from_ids(['16vpA00|3.30.930.10', '1abcA01'], '|')
    with pytest.raises(ValueError, match='at least one character'):
        dct_sim.families_from_ids(['a|b'], '')


# ---- 3. the command line

def _parse(argv):
    from dctdomain_amd import dct_sim
    parser = dct_sim.build_parser()
    err = io.StringIO()
    try:
        with contextlib.redirect_stderr(err):
            return vars(parser.parse_args(['--dct', 'x'] + argv))
    except SystemExit as stop:
        assert stop.code == 2
        return err.getvalue().rstrip('\n').rsplit('\n', 1)[-1].split(': error: ', 1)[1]


SEP = ['--family-sep', '|']
DOES = '--auc1 measures the AUC1 and the top-1 rates of --dct: not with '


@pytest.mark.parametrize('argv, message', [
    (['--auc1'], '--auc1 needs the family of every protein: --families FILE or --family-sep C'),
    (['--auc1', 'global'], '--auc1 needs the family of every protein'),
    (['--auc1', '--families', 'f'] + SEP, '--auc1 takes the families from one place: --families or --family-sep, not both'),
    (['--auc1', '--family-sep', ''], '--family-sep is the text between id and family: at least one character'),
    (['--families', 'f'], '--families says which family a protein belongs to, for --auc1 to judge the hits by: it needs --auc1'),
    (SEP, '--family-sep says which family a protein belongs to, for --auc1 to judge the hits by: it needs --auc1'),
    (['--cluster', '--min-domain', '0.5', '--families', 'f'], '--families says which family'),
    (['--auc1', '--min-global', '0.5'] + SEP, '--auc1 domain ranks the hits by DCTdomain: its cut-off is --min-domain, not --min-global'),
    (['--auc1', 'global', '--min-domain', '0.5'] + SEP, '--auc1 global ranks the hits by DCTglobal: its cut-off is --min-global, not --min-domain'),
    (['--auc1', 'global', '--min-domain', '0.5', '--min-global', '0.5'] + SEP, '--auc1 global ranks the hits by DCTglobal'),
    (['--auc1', 'best'] + SEP, 'argument --auc1: invalid choice'),
])
def test_the_parser_refuses(argv, message):
    got = _parse(argv)
    assert isinstance(got, str) and got.startswith(message), got


@pytest.mark.parametrize('flag, argv', [
    ('--pair', ['--pair', 'p']), ('--db', ['--db', 'y']), ('--cluster', ['--cluster', '--min-domain', '0.5']), ('--rank', ['--rank', 'domain']),
    ('--linkage', ['--linkage', 'single']), ('--level', ['--level', 'protein']), ('--no-whole', ['--no-whole']), ('--reps-out', ['--reps-out', 'f']),
    ('--domains', ['--domains']), ('--dom', ['--dom', 'f']), ('--db-dom', ['--db-dom', 'f']), ('--min-coverage', ['--min-coverage', '0.5']),
    ('--cov-unit', ['--cov-unit', 'domains']), ('--rep', ['--rep', 'first']), ('--min-neighbors', ['--min-neighbors', '3'])])
def test_it_refuses_what_the_tree_refuses(flag, argv):
    got = _parse(['--auc1'] + SEP + argv)
    assert got == DOES + flag, got
    assert _parse(['--tree'] + argv) == '--tree prints the single-linkage tree of --dct: not with ' + flag


@pytest.mark.parametrize('argv, mode', [(['--tree'], '--tree'), (['--db', 'y', '--rbh'], '--rbh'), (['--assign', 'r', '--min-domain', '0.5'], '--assign')])
def test_the_three_modes_refuse_it(argv, mode):
    got = _parse(argv + ['--auc1'] + SEP)
    assert isinstance(got, str) and got.startswith(mode + ' ') and got.endswith(': not with --auc1'), got
    # and the family options stay errors without --auc1, beside any mode
    got = _parse(argv + SEP)
    assert isinstance(got, str) and got.startswith('--family-sep says which family'), got


def test_the_parser_accepts():
    plain = _parse([])
    assert not {'auc1', 'families', 'family_sep'} & set(plain)
    assert _parse(['--auc1'] + SEP) == dict(plain, auc1='domain', family_sep='|')
    assert _parse(['--auc1', 'domain', '--families', 'f', '--min-domain', '0.5', '--output', 'o']) == \
        dict(plain, auc1='domain', families='f', min_domain=0.5, output='o')
    assert _parse(['--auc1', 'global', '--min-global', '0.6'] + SEP) == dict(plain, auc1='global', family_sep='|', min_global=0.6)
    assert _parse(['--family-sep', '__', '--auc1']) == dict(plain, auc1='domain', family_sep='__')


def test_auc1_sim_refuses_what_the_parser_refuses(tmp_path):
    from dctdomain_amd import dct_sim
    out = str(tmp_path / 'out.txt')
    for kw in ({}, {'families': 'f', 'family_sep': '|'}, {'family_sep': '|', 'score': 'best'}, {'family_sep': '|', 'min_global': 0.5},
               {'family_sep': '|', 'score': 'global', 'min_domain': 0.5}):
        with pytest.raises(ValueError):
            dct_sim.auc1_sim(G6PD, out, **kw)
    with pytest.raises(ValueError, match='has no'):
        dct_sim.auc1_sim(G6PD, out, family_sep='|')                 # (the fixture's ids carry no family)
    with pytest.raises(ValueError, match='one entry per protein'):
        dct_sim.Auc1(['a', 'b'], [0, 0, 0], np.zeros((0, 8), dtype=np.int8), ['f'])
    with pytest.raises(ValueError):
        dct_sim.Auc1(['a'], [0, 0], np.zeros((0, 8), dtype=np.int8), ['f'], score='best')


# ---- 4. the text, and what needs no device

HAND_TEXT = (b'p0 a 3 1 0.5000 p5 0.988\n'
             b'p1 b 2 0 0.0000 p2 0.976\n'
             b'p2 a 3 1 0.5000 p1 0.976\n'
             b'p3 a 3 2 1.0000 - -\n'
             b'p4 b 2 0 0.0000 - -\n'
             b'p5 c 1 0 0.0000 p0 0.988\n'
             b'# queries=5 families=2 mean_auc1=0.4000 top1_raw=0.6000 top1_norm=0.5000\n')


@pytest.mark.parametrize('ids', ['array', 'list', 'unicode'])
def test_the_lines_of_the_hand_case(ids):
    from dctdomain_amd import dct_sim
    sid = {'array': np.array(HAND_SID), 'list': HAND_SID, 'unicode': np.array(['p0', 'p1', 'pé', 'p3', 'p4', 'p5'])}[ids]
    counts = ar.of_keys(HAND_KEYS, HAND_FAM)
    fam, names = dct_sim.dense_families(HAND_FAM)
    assert names == ['a', 'b', 'c'] and fam.tolist() == [0, 1, 0, 0, 1, 2]
    want = ar.text(list(sid), HAND_FAM, *counts)
    if ids != 'unicode':
        assert want == HAND_TEXT
    for chunk_bytes in (1 << 24, 30, 1):
        parts = [bytes(memoryview(t)) for t in dct_sim.auc1_lines(sid, fam, names, *counts, score='domain', chunk_bytes=chunk_bytes)]
        assert b''.join(parts) == want and all(p.endswith(b'\n') for p in parts)
        assert chunk_bytes > 30 or len(parts) > 3
    assert b''.join(bytes(memoryview(t)) for t in dct_sim.auc1_lines(sid, fam, names, *counts, score='global')) == want
    # no protein at all: the summary line alone
    empty = np.zeros(0, dtype=np.int32)
    assert b''.join(bytes(memoryview(t)) for t in dct_sim.auc1_lines([], empty, [], empty, empty, empty)) == ar.text([], [], empty, empty, empty)


def test_the_score_text_is_the_pair_lines(g6pd):
    from dctdomain_amd import dct_sim
    table = dct_sim.score_table()
    for key in (0, 1, 199, 200, 8500, 16999, 17000):
        assert bytes(table[0][key]).decode() == bytes(table[1][key]).decode() == ar.score_text(key)


def test_what_needs_no_tile_needs_no_device(tmp_path, g6pd):
    """Fewer than two proteins or a bound below 0: nobody has a hit -- tp 0 and no false positive for everybody."""
    from dctdomain_amd import dct_sim
    sid, idx, dct, tri, fam = g6pd
    job = dct_sim.Auc1(sid, idx, dct, fam.tolist(), score='domain', min_cut=1.5)
    tp, fp_index, fp_key = job.counts()
    assert (tp.dtype, fp_index.dtype, fp_key.dtype) == (np.int32,) * 3
    assert not tp.any() and (fp_index == -1).all() and (fp_key == 17000).all()
    assert job.auc1().dtype == np.float64 and not job.auc1().any()
    assert job.summary() == {'queries': 26, 'families': 3, 'mean_auc1': 0.0, 'top1_raw': 0.0, 'top1_norm': 0.0}
    one = dct_sim.Auc1(sid[:1], idx[:2], dct, ['f'], score='global')
    assert [v.tolist() for v in one.counts()] == [[0], [-1], [17000]] and one.summary()['queries'] == 0
    none = dct_sim.Auc1([], idx[:1], dct, [])
    assert [v.tolist() for v in none.counts()] == [[], [], []] and none.auc1().tolist() == []
    # the command line, end to end: --families, a cut-off above 1
    fam_file = tmp_path / 'fam.txt'
    fam_file.write_text(''.join(f'{s} fam{f}\n' for s, f in zip(sid, fam)))
    out = str(tmp_path / 'out.txt')
    dct_sim.main(['--dct', G6PD, '--auc1', '--families', str(fam_file), '--min-domain', '1.5', '--output', out])
    with open(out, 'rb') as fh:
        got = fh.read()
    assert got == ar.HEADER + ar.text(sid, [f'fam{f}' for f in fam], tp, fp_index, fp_key)
    assert got.splitlines()[1] == f'{sid[0]} fam0 13 0 0.0000 - -'.encode() and got.splitlines()[-1].startswith(b'# queries=26 families=3 mean_auc1=0.0000')


# ---- 5. the build

def test_the_exports_are_declared_bound_and_built():
    import ctypes

    import build_ext
    from dctdomain_amd import _lib, similarity
    with open(os.path.join(ROOT, 'include', 'dctfp.h')) as fh:
        header = fh.read()
    assert int(re.search(r'#define DCTFP_VERSION (\d+)', header).group(1)) >= 114
    sizes = {'dctfp_tri_first_fp': 15, 'dctfp_tri_tp_before': 16}      # ctx, the ten tile values, the arrays, n_nodes, stream
    for name, n_args in sizes.items():
        decl = re.search(r'\nint %s\(([^;]*)\);' % name, header)
        assert decl and decl.group(1).count(',') == n_args - 1, name
        assert 'int64_t n_nodes, void* stream' in re.sub(r'\s+', ' ', decl.group(1))
        assert name in _lib.EXPORTS
        for path in (_lib.LIB_PATH, _lib.EXPERIMENTS_LIB_PATH):
            assert hasattr(ctypes.CDLL(path), name)
        fn = getattr(_lib._configure(ctypes.CDLL(_lib.LIB_PATH)), name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == n_args and fn.argtypes[:11] == _lib._TRI_TILE
        with open(os.path.join(ROOT, 'dctdomain_amd', 'csrc', 'launch.h')) as fh:
            assert 'void launch_%s(' % name[len('dctfp_'):] in fh.read()
        with open(os.path.join(ROOT, 'INTEGRATION.md')) as fh:
            assert name in fh.read()
    assert ctypes.CDLL(_lib.LIB_PATH).dctfp_version() >= 114
    assert callable(similarity.tri_first_fp) and callable(similarity.tri_tp_before)
    assert 'k_auc.hip' in build_ext.UNITS


def _code(path):
    with open(path) as fh:
        return '\n'.join(line.split('//', 1)[0] for line in fh.read().splitlines())


def test_the_unit_touches_its_arrays_through_agent_scope_atomics_alone():
    csrc = os.path.join(ROOT, 'dctdomain_amd', 'csrc')
    unit, walk = _code(os.path.join(csrc, 'k_auc.hip')), _code(os.path.join(csrc, 'band_walk.hip.h'))
    assert '#include "band_walk.hip.h"' in unit and 'asm' not in unit and 'asm' not in walk
    assert '__hip_atomic_fetch_add(' in unit and '__hip_atomic_fetch_min(' in walk and '__hip_atomic_load(' in walk
    # add_count here; lower_hit's load and minimum in the walk's header, where lower_hit and hit_word are defined once
    assert unit.count('__ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT') == 1 and walk.count('__ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT') == 2
    assert 'void lower_hit(' in walk and 'hit_word(' in walk and 'void lower_hit(' not in unit and 'long hit_word(' not in unit
    one = unit[unit.index('struct FirstFpPass'):unit.index('struct TpBeforePass')]
    two = unit[unit.index('struct TpBeforePass'):unit.index('__global__')]
    kernels = unit[unit.index('__global__'):unit.index('namespace dctfp_host')]
    assert 'void tri_first_fp_kernel(const TriTile t, ' in kernels and 'band_walk(t, n_bands, n_steps, FirstFpPass{fam, first});' in kernels
    assert 'void tri_tp_before_kernel(const TriTile t, ' in kernels and 'band_walk(t, n_bands, n_steps, TpBeforePass{fam, first, tp});' in kernels
    for body in (one, two):
        assert 'kBounded = true' in body
    # pass 1 never reads or writes first, and pass 2 never tp, but through the helpers, in the two flushes; pass 2 reads first through
    # _first_of alone and both read fam through _family alone -- in side(), which the walk calls once per column and job and once per
    # row and band (test_cluster_host.py checks the walk); wants() sees the two families before the entry is loaded
    assert not re.search(r'\b(first|tp|fam)\s*\[', one + two + kernels)
    assert len(re.findall(r'\b(first|tp|fam)\s*\[', unit)) == 2                 # (_family's and _first_of's)
    assert len(re.findall(r'lower_hit\(first \+ ', one)) == 2 and len(re.findall(r'add_count\(tp \+ ', two)) == 2
    for body, helper in ((one, r'lower_hit\(first \+ '), (two, r'add_count\(tp \+ ')):
        assert re.search(r'void row_out\([^)]*\) const \{ ' + helper, body) and re.search(r'void col_out\([^)]*\) const \{ ' + helper, body)
    assert not re.search(r'\bwhile\b|\bfor\b', one + two + kernels)
    assert 'Side side(int64_t x) const { return _family(fam, x); }' in one and 'Side side(int64_t x) const { return {_family(fam, x), _first_of(first, x)}; }' in two
    assert len(re.findall(r'_family\(', one)) == 1 and len(re.findall(r'_family\(', two)) == 1 and len(re.findall(r'_first_of\(', two)) == 1
    assert 'wants(Side row_fam, Side col_fam) { return row_fam != col_fam; }' in one
    assert 'wants(const Side& row, const Side& col) { return row.fam == col.fam; }' in two
