"""dct-sim --hist without a GPU: the numpy rule (hist_rule.py) worked by hand and pinned on the committed reference fixture -- against
the lines of the reference's own all-against-all output --, the cut-offs of the table, the summary, the host side of
dct_sim.Histogram on counts handed to it, the command-line rules, and the new export's place in the build."""

import contextlib
import io
import os
import re

import numpy as np
import pytest

import all_sim_filter_rule as rule
import cluster_rule
import golden_util as gu
import hist_rule as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G6PD = os.path.join(gu.GOLD, 'ref_fixtures', 'G6PD-dct.npz')
G6PD_TEXT = os.path.join(gu.GOLD, 'ref_fixtures', 'G6PD-dctsim.txt')
X = 17000


@pytest.fixture(scope='module')
def g6pd():
    with np.load(G6PD) as data:
        sid, idx, dct = [str(s) for s in data['sid']], data['idx'], data['dct']
    tri = rule.triangle_l1(dct, idx)
    return sid, idx, dct, tri, cluster_rule.labels(dct, idx, min_global=0.6)[0]


@pytest.fixture(scope='module')
def printed():
    """(sim-domain, sim-global) of the 351 lines the reference printed for the fixture."""
    lines = rule.read_lines(G6PD_TEXT)[1:]
    return np.array([[float(v) for v in line.split()[2:4]] for line in lines])


# ---- 1. the rule

def test_the_rule_on_a_tile_by_hand():
    """Two rows (proteins 0, 1) x three columns (proteins 1, 2, 3), families 0 0 1 0, bound 10:
         (0, 1) = 5      one family              -> [0, 5]
         (0, 2) = 5      two families            -> [1, 5]
         (0, 3) = 17000  above the bound
         (1, 1) = 99     the diagonal: no pair
         (1, 2) = -1     a negative value is the cap: above the bound
         (1, 3) = 7      one family              -> [0, 7]"""
    t = np.array([[5, 5, X], [99, -1, 7]], dtype=np.int32)
    fam = [0, 0, 1, 0]
    got = hr.tile_hist(t, 0, 1, 10, fam)
    assert got.shape == (2, X + 1) and got.dtype == np.uint64 and got.sum() == 3
    assert got[0, 5] == 1 and got[1, 5] == 1 and got[0, 7] == 1
    one = hr.tile_hist(t, 0, 1, 10)
    assert one.shape == (1, X + 1) and one[0, 5] == 2 and one[0, 7] == 1 and one.sum() == 3
    # the bound itself counts, the one below does not; -1 counts nothing
    assert hr.tile_hist(t, 0, 1, 7, fam).sum() == 3 and hr.tile_hist(t, 0, 1, 6, fam).sum() == 2 and hr.tile_hist(t, 0, 1, -1, fam).sum() == 0
    # the cap as the bound: the two entries of key 17000 count too, (0, 3) of one family and (1, 2) of two
    full = hr.tile_hist(t, 0, 1, X, fam)
    assert full.sum() == 5 and full[0, X] == 1 and full[1, X] == 1
    # column 0 (protein 1) flagged: (0, 1) becomes the cap; row 1 flagged: (1, 3) does
    assert hr.tile_hist(t, 0, 1, 10, fam, col_empty=[True, False, False])[0].sum() == 1
    assert hr.tile_hist(t, 0, 1, 10, fam, row_empty=[False, True])[0, 7] == 0
    # moved left of the diagonal nothing counts; moved right of it everything within the bound does (99 is above it)
    assert hr.tile_hist(t, 5, 0, X, [0] * 7).sum() == 0 and hr.tile_hist(t, 0, 5, 10, [0] * 8).sum() == 3


def test_the_counts_and_the_summary_by_hand():
    """Five pairs of one family with keys 0 0 100 300 17000 and five of two with keys 100 200 300 300 0x7fffffff.
    Same above other: 0 0 beat all five; 100 beats four and ties one; 300 beats one (the pair without L1) and ties two; the pair of
    similarity 0 ties the other one at the bottom: (5 + 5 + 4.5 + 2 + 0.5) / 25 = 0.68.
    F1 at bound 0: 2 * 2 / (2 + 0 + 5) = 4/7; at 100: 2 * 3 / (3 + 1 + 5) = 6/9; at 300: 2 * 4 / (4 + 4 + 5) = 8/13: best at 100."""
    key = [0, 0, 100, 300, X, 100, 200, 300, 300, 0x7fffffff]
    cls = [0] * 5 + [1] * 5
    hist, rest = hr.of_keys(key, cls)
    assert hist.shape == (2, X) and rest.tolist() == [1, 1] and hist[0, 0] == 2 and hist[1, 300] == 2
    s = hr.summary(hist, rest)
    assert s['pairs'] == 10 and s['same'] == 5 and s['other'] == 5 and abs(s['roc_auc'] - 0.68) < 1e-15
    assert hr.best_f1(hist, rest) == (6 / 9, 100) and s['at'] == '%.6f' % (1 - 100.5 / 17000) == '0.994088'
    one = hr.of_keys(key)
    assert hr.summary(*one) == {'pairs': 10, 'scored': 8}
    # a cut-off of the run: the bins end at its bound and the rest grows
    hist, rest = hr.of_keys(key, cls, min_cut=0.99)                 # (bound 170)
    assert hist.shape == (2, 171) and rest.tolist() == [2, 4]
    assert hr.text(hist, rest, 4, 0.99) == b'0.0000 5 5 5 5 1.0000 0.5000 1.0000\n# pairs=10 same=5 other=5 roc_auc=0.7400 best_f1=0.6667 at=0.994088\n'
    # an empty class: no ROC AUC; no pair of one family: no F1 either
    assert hr.summary(*hr.of_keys([5, 6], [1, 1]))['roc_auc'] is None and hr.summary(*hr.of_keys([5, 6], [1, 1]))['best_f1'] is None
    assert hr.summary(*hr.of_keys([5, 6], [0, 0]))['roc_auc'] is None and hr.summary(*hr.of_keys([5, 6], [0, 0]))['best_f1'] == 1.0
    assert hr.text(*hr.of_keys([5, X], [1, 1]), 2) == (b'0.5000 0 1 0 1 - 0.0000 0.5000\n0.0000 0 1 0 2 - 0.0000 1.0000\n'
                                                      b'# pairs=2 same=0 other=2 roc_auc=- best_f1=- at=-\n')


@pytest.mark.parametrize('score', ['domain', 'global'])
@pytest.mark.parametrize('bins', [7, 10, 100])
def test_kept_is_the_number_of_lines_the_reference_printed(g6pd, printed, score, bins):
    sid, idx, dct, tri, fam = g6pd
    hist, rest = hr.of_file(dct, idx, None, score, triangle=tri)
    assert hist.shape == (1, X) and int(hist.sum()) + int(rest.sum()) == len(printed) == 351
    column = printed[:, 0 if score == 'domain' else 1]
    table = hr.table(hist, rest, bins)
    assert len(table) == bins and table[-1] == ('0.0000', [351])
    for text, kept in table:
        assert kept == [int((column >= float(text)).sum())], text
    if bins == 10:
        kept = [k[0] for _, k in table]
        assert kept[:5] == [31, 125, 241, 328, 351] if score == 'domain' else kept[:8] == [5, 28, 49, 78, 109, 118, 243, 351]
    # with families the two classes add up to the same
    both = hr.table(*hr.of_file(dct, idx, fam, score, triangle=tri), bins)
    assert [sum(k) for _, k in both] == [k[0] for _, k in table]


def test_the_summary_of_the_reference_fixture(g6pd):
    sid, idx, dct, tri, fam = g6pd
    assert sorted(np.bincount(fam)[np.bincount(fam) > 0].tolist(), reverse=True) == [13, 7, 6, 1]
    hist, rest = hr.of_file(dct, idx, fam, 'domain', triangle=tri)
    s = hr.summary(hist, rest)
    assert (s['pairs'], s['same'], s['other']) == (351, 114, 237)
    assert '%.4f' % s['roc_auc'] == '0.7467' and '%.4f' % s['best_f1'] == '0.7006' and hr.best_f1(hist, rest)[1] == 2584 and s['at'] == '0.847971'
    assert hr.text(hist, rest, 10).splitlines()[-1] == b'# pairs=351 same=114 other=237 roc_auc=0.7467 best_f1=0.7006 at=0.847971'
    hist, rest = hr.of_file(dct, idx, fam, 'global', triangle=tri)
    s = hr.summary(hist, rest)
    assert '%.4f' % s['roc_auc'] == '1.0000' and '%.4f' % s['best_f1'] == '1.0000' and hr.best_f1(hist, rest)[1] == 8633
    # the ROC AUC is what the pairwise definition gives on the scores themselves
    i, j, mn, last = tri
    key = np.minimum(mn, X)
    same, other = key[fam[i] == fam[j]], key[fam[i] != fam[j]]
    wins = (same[:, None] < other[None, :]).sum() + 0.5 * (same[:, None] == other[None, :]).sum()
    assert abs(hr.roc_auc(*hr.of_file(dct, idx, fam, 'domain', triangle=tri)) - wins / (len(same) * len(other))) < 1e-12


def test_the_edges_come_from_sim_bound_and_not_from_algebra():
    from dctdomain_amd import dct_sim
    for b in (0, 1, 2584, 8633, 16998, 16999):
        assert dct_sim.sim_bound(float(hr.at_text(b))) == b == hr.sim_edge(float(hr.at_text(b)))
    texts, bounds = dct_sim.hist_cuts(100)
    assert texts == hr.cut_texts(100) and texts[0] == '0.9900' and texts[-1] == '0.0000' and bounds[-1] == X
    assert bounds == [dct_sim.sim_bound(float(t)) for t in texts] == [hr.sim_edge(float(t)) for t in texts]
    off = [b for b in range(99) if bounds[b] != (b + 1) * 170]
    assert len(off) == 20 and all(bounds[b] == (b + 1) * 170 - 1 for b in off)
    # cut-off 0.9300 (b = 6): 1 - 1190 / 17000 is 0.92999999999999994 in float64, below 0.93 -- L1 1190 is not kept there
    assert 6 in off and texts[6] == '0.9300' and bounds[6] == 1189 and (1 - 1190 / 17000) < 0.93
    for bins in (1, 7, 1000):
        texts, bounds = dct_sim.hist_cuts(bins)
        assert texts == hr.cut_texts(bins) and bounds == [hr.sim_edge(float(t)) for t in texts] and len(set(texts)) == bins


# ---- 2. the host side of Histogram, on counts handed to it

def _with_counts(job, counts):
    job._counts = counts
    return job


@pytest.mark.parametrize('score, cut', [('domain', None), ('global', None), ('domain', 0.8), ('global', 0.55), ('domain', 0.0)])
def test_table_summary_and_text_from_given_counts(g6pd, score, cut):
    from dctdomain_amd import dct_sim
    sid, idx, dct, tri, fam = g6pd
    for families in (None, [f'fam{f}' for f in fam]):
        counts = hr.of_file(dct, idx, None if families is None else fam, score, min_cut=cut, triangle=tri)
        job = _with_counts(dct_sim.Histogram(sid, idx, dct, families, score=score, min_cut=cut), counts)
        assert job.bound == counts[0].shape[1] - 1 and job.totals() == tuple(int(counts[0][c].sum()) + int(counts[1][c]) for c in range(len(counts[1])))
        for bins in (1, 7, 10, 100):
            texts, kept = job.table(bins)
            want = hr.table(*counts, bins, cut)
            assert texts == [t for t, _ in want] and kept.tolist() == [k for _, k in want] and kept.dtype == np.int64
            assert ('\n'.join(job.lines(bins)) + '\n').encode() == hr.text(*counts, bins, cut)
        got, want = job.summary(), hr.summary(*counts)
        assert got.keys() == want.keys() and all(got[k] == want[k] for k in want if k not in ('roc_auc', 'best_f1'))
        if families is not None:
            assert abs(got['roc_auc'] - want['roc_auc']) < 1e-15 and got['best_f1'] == want['best_f1']
        sink = []
        job.write(sink.append, 10)
        assert b''.join(bytes(m) for m in sink) == hr.text(*counts, 10, cut)
    if cut == 0.8:
        assert texts[-2:] == ['0.8000', '0.0000'] and len(texts) == 21


def test_what_needs_no_tile_needs_no_device(g6pd):
    """Fewer than two proteins or a bound below 0: no bin, every pair in the rest."""
    from dctdomain_amd import dct_sim
    sid, idx, dct, tri, fam = g6pd
    job = dct_sim.Histogram(sid, idx, dct, fam.tolist(), score='domain', min_cut=1.5)
    hist, rest = job.counts()
    assert hist.shape == (2, 0) and hist.dtype == np.uint64 and rest.dtype == np.uint64 and rest.tolist() == [114, 237]
    assert job.lines(2) == ['0.0000 114 237 114 237 1.0000 0.3248 1.0000', '# pairs=351 same=114 other=237 roc_auc=0.5000 best_f1=- at=-']
    assert ('\n'.join(job.lines(2)) + '\n').encode() == hr.text(*hr.of_file(dct, idx, fam, 'domain', min_cut=1.5, triangle=tri), 2, 1.5)
    one = dct_sim.Histogram(sid[:1], idx[:2], dct, score='global')
    assert one.counts()[0].shape == (1, X) and not one.counts()[0].any() and one.counts()[1].tolist() == [0]
    assert one.lines(3) == ['0.6667 0 0', '0.3333 0 0', '0.0000 0 0', '# pairs=0 scored=0']
    none = dct_sim.Histogram([], idx[:1], dct, [])
    assert none.summary() == {'pairs': 0, 'same': 0, 'other': 0, 'roc_auc': None, 'best_f1': None, 'at': None}
    with pytest.raises(ValueError, match='one entry per protein'):
        dct_sim.Histogram(['a', 'b'], [0, 0, 0], np.zeros((0, 8), dtype=np.int8), ['f'])
    with pytest.raises(ValueError):
        dct_sim.Histogram(['a'], [0, 0], np.zeros((0, 8), dtype=np.int8), score='best')
    # a cut-off of 0 or below asks for the cap as the bound: the host stays at 16999 and derives the last bin
    assert dct_sim.Histogram(sid, idx, dct, score='domain', min_cut=0.0).bound == X - 1


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
DOES = '--hist bins the scores of all pairs of --dct: not with '


@pytest.mark.parametrize('argv, message', [
    (['--hist', '--families', 'f'] + SEP, '--hist takes the families from one place: --families or --family-sep, not both'),
    (['--hist', '--family-sep', ''], '--family-sep is the text between id and family: at least one character'),
    (['--hist', '--min-global', '0.5'], '--hist domain bins the pairs by DCTdomain: its cut-off is --min-domain, not --min-global'),
    (['--hist', 'global', '--min-domain', '0.5'], '--hist global bins the pairs by DCTglobal: its cut-off is --min-global, not --min-domain'),
    (['--hist', 'global', '--min-domain', '0.5', '--min-global', '0.5'], '--hist global bins the pairs by DCTglobal'),
    (['--hist', 'best'], 'argument --hist: invalid choice'),
    (['--bins', '10'], '--bins says how many cut-offs the table of --hist has: it needs --hist'),
    (['--cluster', '--min-domain', '0.5', '--bins', '10'], '--bins says how many cut-offs'),
    (['--hist', '--bins', '0'], '--bins is a number of cut-offs: 1 .. 1000'),
    (['--hist', '--bins', '1001'], '--bins is a number of cut-offs: 1 .. 1000'),
    (['--hist', '--bins', 'ten'], 'argument --bins: invalid int value'),
    (['--hist', '--auc1'] + SEP, '--auc1 measures the AUC1 and the top-1 rates of --dct: not with --hist'),
    # without --hist and --auc1 the family options keep their message
    (['--families', 'f'], '--families says which family a protein belongs to, for --auc1 to judge the hits by: it needs --auc1'),
    (SEP, '--family-sep says which family a protein belongs to, for --auc1 to judge the hits by: it needs --auc1'),
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
    assert _parse(['--tree'] + argv) == '--tree prints the single-linkage tree of --dct: not with ' + flag
    assert _parse(['--hist', '--auc1'] + SEP) == '--auc1 measures the AUC1 and the top-1 rates of --dct: not with --hist'
    # (a mode, checked after the other four; --bins and the family flags are its options, no modes of their own)
    for mode, line in (('--tree', ['--tree']), ('--rbh', ['--db', 'y', '--rbh']), ('--assign', ['--assign', 'r', '--min-domain', '0.5']),
                       ('--auc1', ['--auc1'] + SEP)):
        assert _parse(line + ['--hist']).startswith(mode + ' ')
    assert _parse(['--hist', '--bins', '10'] + SEP)['hist'] == 'domain'
    assert _parse(['--hist'] + argv) == DOES + flag


@pytest.mark.parametrize('argv, mode', [(['--tree'], '--tree'), (['--db', 'y', '--rbh'], '--rbh'), (['--assign', 'r', '--min-domain', '0.5'], '--assign'),
                                        (['--auc1'] + SEP, '--auc1')])
def test_the_four_modes_refuse_it(argv, mode):
    # --hist is the last flag they name: beside any other flag the mode refuses, that one is named
    for flag, more in (('--pair', ['--pair', 'p']), ('--cluster', ['--cluster']), ('--rank', ['--rank', 'domain']), ('--linkage', ['--linkage', 'single']),
                       ('--level', ['--level', 'protein']), ('--no-whole', ['--no-whole']), ('--min-coverage', ['--min-coverage', '0.5']),
                       ('--cov-unit', ['--cov-unit', 'domains']), ('--rep', ['--rep', 'first']), ('--min-neighbors', ['--min-neighbors', '3'])):
        assert _parse(argv + ['--hist'] + more) == _parse(argv + more) and _parse(argv + more).endswith(': not with ' + flag)
    got = _parse(argv + ['--hist'])
    assert isinstance(got, str) and got.startswith(mode + ' ') and got.endswith(': not with --hist'), got


def test_the_parser_accepts():
    plain = _parse([])
    assert not {'hist', 'bins', 'families', 'family_sep'} & set(plain)
    assert _parse(['--hist']) == dict(plain, hist='domain')
    assert _parse(['--hist', 'global', '--bins', '1000', '--min-global', '0.6']) == dict(plain, hist='global', bins=1000, min_global=0.6)
    assert _parse(['--hist', 'domain', '--families', 'f', '--min-domain', '0.5', '--output', 'o', '--bins', '1']) == \
        dict(plain, hist='domain', families='f', min_domain=0.5, output='o', bins=1)
    assert _parse(['--family-sep', '__', '--hist']) == dict(plain, hist='domain', family_sep='__')


def test_hist_sim_refuses_what_the_parser_refuses(tmp_path):
    from dctdomain_amd import dct_sim
    out = str(tmp_path / 'out.txt')
    for kw in ({'families': 'f', 'family_sep': '|'}, {'score': 'best'}, {'min_global': 0.5}, {'score': 'global', 'min_domain': 0.5},
               {'bins': 0}, {'bins': 1001}, {'bins': 2.5}, {'family_sep': ''}):
        with pytest.raises(ValueError):
            dct_sim.hist_sim(G6PD, out, **kw)
        assert not os.path.exists(out) or kw == {'family_sep': ''}
    with pytest.raises(ValueError, match='has no'):
        dct_sim.hist_sim(G6PD, out, family_sep='|')                 # (the fixture's ids carry no family)


def test_cli_without_a_tile(tmp_path, g6pd):
    """The command line end to end where no device is needed: a cut-off above 1."""
    from dctdomain_amd import dct_sim
    sid, idx, dct, tri, fam = g6pd
    fam_file = tmp_path / 'fam.txt'
    fam_file.write_text(''.join(f'{s} fam{f}\n' for s, f in zip(sid, fam)))
    out = str(tmp_path / 'out.txt')
    dct_sim.main(['--dct', G6PD, '--hist', '--families', str(fam_file), '--min-domain', '1.5', '--bins', '4', '--output', out])
    with open(out, 'rb') as fh:
        got = fh.read()
    assert got == hr.header('domain', True) + hr.text(*hr.of_file(dct, idx, fam, 'domain', min_cut=1.5, triangle=tri), 4, 1.5)
    dct_sim.hist_sim(G6PD, out, score='global', bins=3, min_global=2.0)
    with open(out, 'rb') as fh:
        assert fh.read() == b'#min-global pairs kept\n0.0000 351 351\n# pairs=351 scored=0\n'


# ---- 4. the build

def test_the_export_is_declared_bound_and_built():
    import ctypes

    import build_ext
    from dctdomain_amd import _lib, similarity
    with open(os.path.join(ROOT, 'include', 'dctfp.h')) as fh:
        header = fh.read()
    assert int(re.search(r'#define DCTFP_VERSION (\d+)', header).group(1)) >= 115
    name = 'dctfp_tri_hist'
    decl = re.search(r'\nint %s\(([^;]*)\);' % name, header)
    assert decl and decl.group(1).count(',') == 15 - 1                  # ctx, the ten tile values, fam, n_nodes, hist, stream
    assert 'const int32_t* fam, int64_t n_nodes, uint64_t* hist, void* stream' in re.sub(r'\s+', ' ', decl.group(1))
    assert name in _lib.EXPORTS
    for path in (_lib.LIB_PATH, _lib.EXPERIMENTS_LIB_PATH):
        assert hasattr(ctypes.CDLL(path), name)
    fn = getattr(_lib._configure(ctypes.CDLL(_lib.LIB_PATH)), name)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 15 and fn.argtypes[:11] == _lib._TRI_TILE
    with open(os.path.join(ROOT, 'dctdomain_amd', 'csrc', 'launch.h')) as fh:
        assert 'int launch_tri_hist(const TriTile& t, ' in fh.read()
    with open(os.path.join(ROOT, 'INTEGRATION.md')) as fh:
        assert name in fh.read()
    assert ctypes.CDLL(_lib.LIB_PATH).dctfp_version() >= 115
    assert callable(similarity.tri_hist)
    assert 'k_hist.hip' in build_ext.UNITS


def _code(path):
    with open(path) as fh:
        return '\n'.join(line.split('//', 1)[0] for line in fh.read().splitlines())


def test_the_unit_touches_hist_through_agent_scope_atomics_alone():
    csrc = os.path.join(ROOT, 'dctdomain_amd', 'csrc')
    unit = _code(os.path.join(csrc, 'k_hist.hip'))
    # it stands on its own: the tile's description and the launchers' header, neither walk
    assert re.findall(r'#include "([^"]+)"', unit) == ['launch.h', 'tri_tile.hip.h'] and 'asm' not in unit
    with open(os.path.join(csrc, 'k_hist.hip')) as fh:
        assert 'NOT a pass of band_walk' in fh.read()
    kernel = unit[unit.index('__global__'):unit.index('namespace dctfp_host')]
    assert 'void tri_hist_kernel(const TriTile t, const int32_t* __restrict__ fam, unsigned long long* bins_out,' in kernel
    # the output array: named once behind the head, in the flush, and only as the base of an address handed to add_bin
    assert len(re.findall(r'\bbins_out\b', kernel)) == 2 and 'add_bin(bins_out + ' in kernel
    assert not re.search(r'bins_out\s*\[|(?<!long)\*\s*\(?\s*bins_out', kernel)     # (`unsigned long long* bins_out` declares)
    assert unit.count('__ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT') == 1 and unit.count('__HIP_MEMORY_SCOPE_AGENT') == 1
    helper = unit[unit.index('void add_bin('):unit.index('__global__')]
    assert '__hip_atomic_fetch_add(slot, (unsigned long long)count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);' in helper
    # a zero bin is not sent, and the flush stands behind the job loop and a barrier
    jobs, flush = kernel.index('for (int64_t job = blockIdx.x;'), kernel.index('if (count != 0) add_bin(')
    assert jobs < kernel.rindex('__syncthreads();') < flush and not re.search(r'\bwhile\b|for \(;;\)', unit)
    # the counters of a workgroup are LDS words, added to at workgroup scope; the job left of the diagonal is left before any load
    assert 'extern __shared__ uint32_t s_bins[];' in kernel and unit.count('__HIP_MEMORY_SCOPE_WORKGROUP') == 2
    assert kernel.index('- 1 <= i_lo) continue;') < kernel.index('col_empty[') < kernel.index('fam[j]') < kernel.index('column[')
    # fam: once per column and job, once per row -- never inside the wave's add
    assert len(re.findall(r'\bfam\s*\[', kernel)) == 2 and 'fam' not in unit[unit.index('void wave_count('):unit.index('void add_bin(')]
    # why the 32-bit counters cannot overflow is asserted where it is written
    assert 'static_assert(kHistJobsPerBlock * kHistRows * kHistCols < ((int64_t)1 << 32)' in unit
    host = unit[unit.index('namespace dctfp_host'):]
    assert 'most * kHistJobsPerBlock / n_steps' in host and 'min(bands * n_steps, most)' in host
    with open(os.path.join(csrc, 'dctfp_sim.hip')) as fh:
        text = fh.read()
    body = text[text.index('\nint dctfp_tri_hist('):text.index('DCTFP_GUARD("dctfp_tri_hist")')]
    assert 'check_band_tile(' not in body and 'check_tri_tile(' not in body and 'ld < n_cols' in body and 'tri_hist_max_cap()' in body
