"""CPU-side checks of dct-sim --min-coverage: the rule (coverage_rule.py) worked by hand and on the committed reference fixture,
the weights and the need, the command line, and dctfp_protein_cover in the library and its header."""

import contextlib
import ctypes
import io
import os
import re

import numpy as np
import pytest

import all_sim_filter_rule as rule
import coverage_rule as cr
import golden_util as gu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G6PD = os.path.join(gu.GOLD, 'ref_fixtures', 'G6PD-dct.npz')

# ---- the rule by hand: families of identical rows 320 apart (8 bytes x 40), cut-off 0.99 = bound 170

CUT = 0.99


def _fam(*values):
    return np.array([np.full(8, v, dtype=np.int8) for v in values])


def _edge(dct, idx, w, c, p=0, q=1):
    i, j, _, _, keep = cr.edges(dct, idx, w, CUT, c)
    return bool(keep[(i == p) & (j == q)][0])


def test_the_bound_of_the_hand_worked_cut_off():
    assert cr.bound_of(CUT) == 170 and cr.bound_of(0.5) == 8500 and cr.bound_of(0) == 17000 and cr.bound_of(1.5) == -1


def test_a_single_domain_protein_covers_a_third_of_a_three_domain_protein():
    """A = domains f1 f2 f3 + its whole row, B = f2 alone.  B's only row is matched: B is covered in full.  Of A only the f2 row is:
    1 of 3 domains, 80 of 200 residues."""
    dct = np.concatenate([_fam(-120, -80, -40, 120), _fam(-80)])
    idx = [0, 4, 5]
    names = ['1-60', '61-140', '141-200', '1-200', '1-80']
    by_dom, by_res = cr.weights(idx, None, 'domains'), cr.weights(idx, names, 'residues')
    assert by_dom.tolist() == [1, 1, 1, 3, 1] and by_res.tolist() == [60, 80, 60, 200, 80]
    nd = cr.need(cr.protein_weights(idx, by_res), 0.3)
    t = cr.cover_tile(dct, idx, by_res, nd, dct, idx, by_res, nd, 170, cap=cr.CAP)
    assert t['cov_a'][0, 1] == 80 and t['cov_b'][0, 1] == 80 and t['min'][0, 1] == 0 and nd.tolist() == [60, 24]
    for w in (by_dom, by_res):
        assert _edge(dct, idx, w, 0.3) and not _edge(dct, idx, w, 0.5)
    assert _edge(dct, idx, by_res, 0.4) and not _edge(dct, idx, by_res, 0.41)     # (80 of 200)


def test_two_of_three_shared_domains_are_an_edge_at_0_6_in_domains():
    """P = f1 f2 f3 + whole, Q = f1 f2 f4 + whole, the whole rows far from everything: 2 of 3 domains on both sides."""
    dct = np.concatenate([_fam(-120, -80, -40, 80), _fam(-120, -80, 0, 120)])
    idx = [0, 4, 8]
    w = cr.weights(idx, None, 'domains')
    assert _edge(dct, idx, w, 0.6) and _edge(dct, idx, w, 0.66) and not _edge(dct, idx, w, 0.7)
    # ... and through the whole row alone: R = a row equal to P's whole row covers P in full
    dct3 = np.concatenate([dct, _fam(80)])
    idx3, w3 = [0, 4, 8, 9], cr.weights([0, 4, 8, 9], None, 'domains')
    assert _edge(dct3, idx3, w3, 1.0, 0, 2) and not _edge(dct3, idx3, w3, 0.01, 1, 2)


def test_a_protein_without_rows_is_an_edge_only_where_the_cut_off_keeps_every_pair():
    dct, idx = _fam(0, 0), [0, 1, 1, 2]
    w = cr.weights(idx, None, 'domains')
    assert cr.protein_weights(idx, w).tolist() == [1, 0, 1] and cr.need([1, 0, 1], 0.5).tolist() == [1, 0, 1]
    assert cr.edges(dct, idx, w, 0.5, 0.5)[4].tolist() == [False, True, False]
    assert cr.edges(dct, idx, w, 0.0, 0.5)[4].tolist() == [True, True, True]


# ---- weights and need

def test_weights_of_discontinuous_names_single_rows_and_whole_rows():
    from dctdomain_amd import dct_sim
    sid = np.array(['P1', 'P2', 'EMPTY', 'P3'])
    idx = [0, 3, 4, 4, 6]
    names = ['1-30,61-100', '31-60', 'anything', '5-104', '1-7', '8-9']
    w = dct_sim.coverage_weights(sid, idx, names, 'residues')
    assert w.dtype == np.int64 and w.tolist() == [70, 30, 100, 100, 7, 7]        # (P1's whole row carries 70 + 30; P3 has two rows: a domain and the whole)
    assert (w == cr.weights(idx, names, 'residues')).all()
    assert dct_sim.coverage_weights(sid, idx, None, 'domains').tolist() == [1, 1, 2, 1, 1, 1]
    assert (cr.weights(idx, None, 'domains') == dct_sim.coverage_weights(sid, idx, names, 'domains')).all()
    assert dct_sim._residues('1-30,61-100') == 70 and dct_sim._residues('whole') == 0 and dct_sim._residues('9-3') == 0
    with pytest.raises(ValueError, match='unit'):
        dct_sim.coverage_weights(sid, idx, names, 'atoms')


def test_missing_or_unreadable_names_raise_naming_the_protein():
    from dctdomain_amd import dct_sim
    sid, idx = np.array(['EMPTY', 'P2', 'P3']), [0, 0, 1, 3]
    with pytest.raises(ValueError, match=r'protein P2 .*--cov-unit domains'):
        dct_sim.coverage_weights(sid, idx, None, 'residues')
    with pytest.raises(ValueError, match=r"protein P3: 'x-y' .*--cov-unit domains"):
        dct_sim.coverage_weights(sid, idx, ['1-5', 'x-y', '1-9'], 'residues')
    with pytest.raises(ValueError, match='2\\^30'):
        dct_sim.coverage_weights(sid, idx, ['1-5', f'1-{1 << 30}', '1-9'], 'residues')
    assert dct_sim.coverage_weights(sid, idx, ['1-5', f'1-{(1 << 30) - 1}', 'whole'], 'residues')[2] == (1 << 30) - 1


def test_need_is_an_integer_ceiling_that_forgives_float_noise():
    from dctdomain_amd.dct_sim import coverage_need
    assert coverage_need(10, 0.7) == 7 and isinstance(coverage_need(10, 0.7), int)      # (0.7 x 10 = 7.000000000000001)
    for W in (1, 3, 10, 779, (1 << 30) - 1):
        assert coverage_need(W, 1.0) == W
    assert coverage_need(3, 0.01) == 1 and coverage_need(3, 0.34) == 2 and coverage_need(0, 0.5) == 0
    assert coverage_need(np.array([10, 3, 0, 200]), 0.3).tolist() == [3, 1, 0, 60]


def test_a_job_computes_a_coverage_only_where_it_can_exclude_a_pair():
    from dctdomain_amd import dct_sim
    sid, idx, fps = ['a', 'b', 'c'], [0, 2, 2, 3], np.zeros((3, 480), np.int8)
    w = dct_sim.coverage_weights(sid, idx, None, 'domains')
    job = dct_sim.FilteredPairs(sid, idx, fps, min_domain=0.5, min_global=0.25, min_coverage=0.8, weights=w)
    assert job.route == 'domain' and job.bound == 8500 and job.bound_global == 12750
    assert job.cover[0].tolist() == [1, 1, 1] and job.cover[1].tolist() == [1, 0, 1] and job.cover[0].dtype == job.cover[1].dtype == np.int32
    for cut in (0.0, 1.5):                                      # every row is matched / none is
        job = dct_sim.FilteredPairs(sid, idx, fps, min_domain=cut, min_global=0.25, min_coverage=0.8, weights=w)
        assert job.cover is None and job.route == 'global'
    c = dct_sim.Clusters(sid, idx, fps, min_domain=0.5).with_coverage(0.8, w)
    assert isinstance(c, dct_sim.Clusters) and c.cover is not None and c._plain_labels() is None
    assert dct_sim.Representatives(sid, idx, fps, min_domain=0.0).with_coverage(0.8, w)._plain_labels().tolist() == [0, 0, 0]
    assert dct_sim.Clusters(sid, idx, fps, min_domain=1.5).with_coverage(0.8, w)._plain_labels().tolist() == [0, 1, 2]
    for bad in ({'min_coverage': 0.0, 'weights': w}, {'min_coverage': 1.01, 'weights': w}, {'min_coverage': 0.5},
                {'min_coverage': 0.5, 'weights': w[:2]}):
        with pytest.raises(ValueError):
            dct_sim.FilteredPairs(sid, idx, fps, min_domain=0.5, **bad)
    with pytest.raises(ValueError, match='min_domain'):
        dct_sim.FilteredPairs(sid, idx, fps, min_global=0.5, min_coverage=0.5, weights=w)


# ---- the command line

def _parse(argv):
    from dctdomain_amd import dct_sim
    err = io.StringIO()
    try:
        with contextlib.redirect_stderr(err):
            return vars(dct_sim.build_parser().parse_args(['--dct', 'x.npz'] + argv)), None
    except SystemExit as stop:
        assert stop.code == 2
        return None, err.getvalue().rstrip('\n').rsplit('\n', 1)[-1].split(': error: ', 1)[1]


@pytest.mark.parametrize('argv,said', [
    (['--min-coverage', '0.8'], '--min-coverage counts the fingerprints within the DCTdomain cut-off: it needs --min-domain'),
    (['--min-coverage', '0.8', '--min-global', '0.5'], '--min-coverage counts the fingerprints within the DCTdomain cut-off: it needs --min-domain'),
    (['--min-domain', '0.5', '--min-coverage', '0'], '--min-coverage is a share of a protein: above 0 and at most 1'),
    (['--min-domain', '0.5', '--min-coverage', '1.01'], '--min-coverage is a share of a protein: above 0 and at most 1'),
    (['--min-domain', '0.5', '--min-coverage', 'nan'], '--min-coverage is a share of a protein: above 0 and at most 1'),
    (['--min-domain', '0.5', '--cov-unit', 'domains'], '--cov-unit says what --min-coverage counts: it needs --min-coverage'),
    (['--min-domain', '0.5', '--min-coverage', '0.8', '--pair', 'p.txt'], '--min-coverage applies to all-against-all only, not to --pair or --db'),
    (['--min-domain', '0.5', '--min-coverage', '0.8', '--db', 'y.npz'], '--min-coverage applies to all-against-all only, not to --pair or --db'),
    (['--min-domain', '0.5', '--min-coverage', '0.8', '--db', 'y.npz', '--rbh'],
     '--rbh prints the reciprocal best hits of --dct and --db: not with --min-coverage'),
    (['--min-domain', '0.5', '--min-coverage', '0.8', '--assign', 'r.npz'],
     '--assign places the proteins of --dct on a fixed set of representatives: not with --min-coverage'),
    (['--min-domain', '0.5', '--min-coverage', '0.8', '--tree'], '--tree prints the single-linkage tree of --dct: not with --min-coverage'),
    (['--min-domain', '0.5', '--cov-unit', 'domains', '--tree'], '--tree prints the single-linkage tree of --dct: not with --cov-unit'),
    (['--min-domain', '0.5', '--min-coverage', '0.8', '--cluster', '--level', 'domain'],
     '--min-coverage is a share of a protein: not with --level domain, which joins single fingerprints'),
    (['--min-domain', '0.5', '--min-coverage', '0.8', '--cluster', '--dom', 'x.dom', '--domains'],
     '--domains (--dom, --db-dom) explains the scores of result lines: not with --cluster'),
    (['--min-domain', '0.5', '--cluster', '--dom', 'x.dom'], '--domains (--dom, --db-dom) explains the scores of result lines: not with --cluster'),
])
def test_parser_refuses(argv, said):
    ns, error = _parse(argv)
    assert ns is None and error == said and error.startswith('--')


def test_parser_knows_two_units():
    ns, error = _parse(['--min-domain', '0.5', '--min-coverage', '0.8', '--cov-unit', 'atoms'])
    assert ns is None and 'invalid choice' in error and "'residues', 'domains'" in error


def test_parser_accepts_and_leaves_other_namespaces_alone():
    plain, _ = _parse(['--min-domain', '0.5'])
    assert 'min_coverage' not in plain and 'cov_unit' not in plain
    ns, _ = _parse(['--min-domain', '0.5', '--min-coverage', '0.8'])
    assert ns == dict(plain, min_coverage=0.8)
    ns, _ = _parse(['--min-domain', '0.5', '--min-coverage', '1', '--cov-unit', 'domains', '--min-global', '0.2'])
    assert ns == dict(plain, min_coverage=1.0, cov_unit='domains', min_global=0.2)
    # in the all-against-all --dom still implies --domains; beside --cluster it gives the residues and implies nothing
    ns, _ = _parse(['--min-domain', '0.5', '--min-coverage', '0.8', '--dom', 'x.dom'])
    assert ns['domains'] is True and ns['dom'] == 'x.dom'
    for more in ([], ['--linkage', 'greedy', '--reps-out', 'r.npz']):
        ns, error = _parse(['--min-domain', '0.5', '--min-coverage', '0.8', '--cluster', '--dom', 'x.dom'] + more)
        assert error is None and 'domains' not in ns and ns['dom'] == 'x.dom' and ns['cluster'] is True


def test_cluster_sim_takes_the_coverage_at_protein_level_only(tmp_path):
    from dctdomain_amd import dct_sim
    report = dct_sim.Report(str(tmp_path / 'out.txt'), dct_sim.CLUSTER_HEADER)
    with pytest.raises(ValueError, match='min_domain alone'):
        dct_sim.cluster_sim(G6PD, report, min_domain=0.5, level='domain', min_coverage=0.8)
    with pytest.raises(ValueError, match='dom without min_coverage'):
        dct_sim.cluster_sim(G6PD, report, min_domain=0.5, dom='x.dom')


# ---- the library

def test_library_exports_protein_cover_and_header_documents_it():
    from dctdomain_amd import _lib
    with open(os.path.join(ROOT, 'include', 'dctfp.h')) as fh:
        header = fh.read()
    decl = re.search(r'/\*((?:(?!\*/).)*)\*/\s*int dctfp_protein_cover\(([^;]*)\);', header, re.S)
    assert decl, 'dctfp_protein_cover is not declared with a comment in include/dctfp.h'
    doc, params = decl.group(1), ' '.join(decl.group(2).split())
    assert params == ('dctfp_ctx* ctx, const int8_t* a, int64_t lda, const int64_t* idx_a, int64_t npa, const int32_t* w_a, '
                      'const int32_t* need_a, const int8_t* b, int64_t ldb, const int64_t* idx_b, int64_t npb, const int32_t* w_b, '
                      'const int32_t* need_b, int32_t d, int32_t bound, int32_t* out, int64_t ldo, void* stream')
    for word in ('0x7fffffff', '0x7ffffffe', 'DCTFP_ERR_LIMIT', '512', 'dctfp_protein_min', 'byte for byte', 'need_a', 'w_b'):
        assert word in doc
    version = int(re.search(r'#define DCTFP_VERSION (\d+)', header).group(1))
    assert version >= 111
    for path in (_lib.LIB_PATH, _lib.EXPERIMENTS_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert hasattr(lib, 'dctfp_protein_cover') and lib.dctfp_version() == version
    assert 'dctfp_protein_cover' in _lib.EXPORTS
    assert len(_lib.load().dctfp_protein_cover.argtypes) == 18


# ---- the committed reference fixture

def test_g6pd_at_0_5_and_0_8_in_residues_keeps_109_of_351_pairs_in_4_clusters():
    from dctdomain_amd import dct_sim
    with np.load(G6PD) as data:
        sid, idx, dct, dom = data['sid'], data['idx'], data['dct'], data['dom']
    w = dct_sim.coverage_weights(sid, idx, dom, 'residues')
    assert (w == cr.weights(idx, dom, 'residues')).all() and w[:7].tolist() == [34, 185, 188, 69, 56, 249, 781]
    i, j, mn, last, keep = cr.edges(dct, idx, w, 0.5, 0.8)
    within = rule.kept(mn, last, 0.5, None)
    assert len(i) == 351 and int(within.sum()) == 351 and int(keep.sum()) == 109 and not (keep & ~within).any()
    label = cr.components(len(sid), i, j, keep)
    assert len(set(label.tolist())) == 4
    assert len(set(cr.components(len(sid), i, j, within).tolist())) == 1          # (the README's one cluster without the coverage)
    rep = cr.greedy(len(sid), i, j, keep)
    assert (rep[rep] == rep).all() and len(set(rep.tolist())) >= 4
