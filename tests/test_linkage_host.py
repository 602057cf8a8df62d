"""dct-sim --hac without a GPU: the rule of linkage_rule.py (the oracle of test_linkage_gpu.py) against the textbook serial
algorithm and against scipy, the properties the feature promises (a complete-linkage cluster's diameter, monotone heights, the
cut property), the README's G6PD figures, the three texts on hand-worked trees, the command line, and the native pieces as far
as they can be seen from here (the header, the exports of both libraries, the untouched main header)."""

import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import golden_util as gu
import linkage_rule as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPZ = os.path.join(gu.GOLD, 'all_sim', 'all-dct.npz')
G6PD = os.path.join(gu.GOLD, 'ref_fixtures', 'G6PD-dct.npz')
BOUNDS = (16999, 8500, 6800, 3000)

_CACHE = {}


def _fixture(path, score):
    """(sid, key matrix) of a committed fixture: computed once, shared, read-only."""
    if (path, score) not in _CACHE:
        with np.load(path) as data:
            sid, idx, dct = [str(s) for s in data['sid']], np.asarray(data['idx'], dtype=np.int64), data['dct']
        key = lr.keys_of(dct, idx, score)
        key.setflags(write=False)
        _CACHE[path, score] = (sid, key)
    return _CACHE[path, score]


def _same_merges(a, b):
    return sorted(m[:5] for m in a) == sorted(m[:5] for m in b)


def test_the_bounds_are_the_cut_offs_they_stand_for():
    from dctdomain_amd.dct_sim import sim_bound
    assert (sim_bound(0.5), sim_bound(0.6)) == (8500, 6800)


# ---- the rule against the serial algorithm, the cut property, the promises

@pytest.mark.parametrize('method', lr.METHODS)
@pytest.mark.parametrize('score', ['domain', 'global'])
@pytest.mark.parametrize('path', [NPZ, G6PD], ids=['all', 'g6pd'])
def test_rule_against_serial_on_the_fixtures(path, score, method):
    sid, key = _fixture(path, score)
    n = len(sid)
    runs = {}
    for bound in BOUNDS:
        made, rounds = lr.rounds(key, bound, method)
        runs[bound] = made
        assert _same_merges(made, lr.serial(key, bound, method)), bound
        assert 0 <= rounds <= max(0, n - 1) and (rounds > 0) == bool(made)
        heights = [lr.height(m) for m in lr.ordered(made)]
        assert heights == sorted(heights) and all(h <= bound for h in heights)
        # a child is made in an earlier round than its parent, and a parent is not lower than its children
        born = {}
        for a, b, num, den, size, rnd in lr.ordered(made):
            for child in (a, b):
                if child in born:
                    assert born[child][0] < rnd and born[child][1] <= Fraction(num, den)
            born.pop(b, None)
            born[a] = (rnd, Fraction(num, den))
        lab = lr.labels_at(n, made, bound)
        if method == 'complete':                                 # the diameter guarantee: every pair inside a cluster is within the bound
            same = lab[:, None] == lab[None, :]
            np.fill_diagonal(same, False)
            assert (key[same] <= bound).all()
    for small in BOUNDS[1:]:                                     # the cut property: a run at a smaller bound = the larger run cut there
        assert np.array_equal(lr.labels_at(n, runs[small], small), lr.labels_at(n, runs[BOUNDS[0]], small))
        assert _same_merges(runs[small], [m for m in runs[BOUNDS[0]] if m[2] <= small * m[3]])


def _tie_heavy(seed):
    rng = np.random.default_rng(seed)
    n, values = int(rng.integers(3, 12)), int(rng.integers(2, 6))
    levels = np.sort(rng.choice(np.arange(1, 17000), size=values, replace=False))
    key = np.triu(levels[rng.integers(0, values, size=(n, n))], 1)
    return n, key + key.T, levels


def test_rule_against_serial_on_tie_heavy_matrices():
    """300 seeded matrices of 3 .. 11 nodes with 2 .. 5 distinct key values: the same merges as the serial algorithm, and the cut
    property at every level of the matrix."""
    for seed in range(300):
        n, key, levels = _tie_heavy(seed)
        for method in lr.METHODS:
            top, _ = lr.rounds(key, 16999, method)
            assert _same_merges(top, lr.serial(key, 16999, method)), (seed, method)
            for bound in levels:
                made, _ = lr.rounds(key, int(bound), method)
                assert _same_merges(made, lr.serial(key, int(bound), method)), (seed, method, bound)
                assert np.array_equal(lr.labels_at(n, made, bound), lr.labels_at(n, top, bound)), (seed, method, bound)


def test_rule_against_scipy_on_a_tie_free_matrix():
    """150 x 150 distinct integers: scipy's linkage gives the same merged sets and sizes; complete heights exactly, average heights
    within 1e-12 relative -- scipy's float64 Lance-Williams updates are good to about n eps = 3e-14, and two distinct exact heights
    of this size differ by 2e-12 relative or more, so the order cannot flip."""
    hierarchy = pytest.importorskip('scipy.cluster.hierarchy')
    from scipy.spatial.distance import squareform
    rng = np.random.default_rng(150)
    n = 150
    vals = rng.choice(np.arange(1, 17000), size=n * (n - 1) // 2, replace=False)
    key = squareform(vals).astype(np.int64)
    for method in lr.METHODS:
        made, rounds = lr.rounds(key, 16999, method)
        made = lr.ordered(made)
        assert len(made) == n - 1 and 1 <= rounds <= n - 1
        Z = hierarchy.linkage(squareform(key.astype(np.float64)), method=method)
        members = {i: frozenset([i]) for i in range(n)}
        ours = {i: frozenset([i]) for i in range(n)}
        for k, (a, b, num, den, size, _rnd) in enumerate(made):
            za, zb = members[int(Z[k, 0])], members[int(Z[k, 1])]
            members[n + k] = za | zb
            assert {za, zb} == {ours[a], ours[b]} and int(Z[k, 3]) == size == len(za | zb)
            ours[a] = ours[a] | ours.pop(b)
            if method == 'complete':
                assert Z[k, 2] == num and den == 1
            else:
                assert abs(Z[k, 2] - num / den) <= 1e-12 * (num / den)


def test_g6pd_cluster_sizes():
    """The figures of the README's table: where single linkage chains the 27 proteins, complete linkage splits them."""
    sid, glob = _fixture(G6PD, 'global')
    _, dom = _fixture(G6PD, 'domain')
    n = len(sid)

    def sizes(key, bound, method):
        return lr.sizes_of(lr.labels_at(n, lr.rounds(key, bound, method)[0], bound))
    assert sizes(glob, 6800, 'complete') == [7, 7, 6, 5, 1, 1] == sizes(glob, 6800, 'average')
    assert sizes(dom, 6800, 'complete') == [18, 8, 1] and sizes(dom, 6800, 'average') == [27]
    assert sizes(dom, 8500, 'complete') == [27]
    sid_all, key_all = _fixture(NPZ, 'domain')
    for method, merges, rounds in (('complete', 122, 15), ('average', 138, 32)):
        made, r = lr.rounds(key_all, 16999, method)
        assert (len(made), r) == (merges, rounds)


# ---- the three texts on hand-worked trees

def _four():
    """Four leaves: b and c at 1700, a joins them at 3400 (complete: max(3400, 3400); average: (3400 + 3400) / 2), d'x at 17000."""
    key = np.array([[0, 3400, 3400, 17000], [3400, 0, 1700, 17000], [3400, 1700, 0, 17000], [17000, 17000, 17000, 0]], dtype=np.int64)
    return ['a', 'b c', "d'x", 'e'], key


def test_hand_worked_texts():
    sid, key = _four()
    for method, den in (('complete', 1), ('average', 2)):
        made, rounds = lr.rounds(key, 16999, method)
        assert rounds == 2 and lr.ordered(made) == [(1, 2, 1700, 1, 2, 1), (0, 1, 3400 * den, den, 3, 2)]
        assert lr.text(sid, made) == b"#rep1 rep2 similarity size\nb c d'x 0.9000 2\na b c 0.8000 3\n"
        assert lr.flat_text(sid, lr.labels_at(4, made, 16999)) == b"a a\na b c\na d'x\ne e\n"
        # a forest of two trees; ids with a blank and with a quote are quoted, the quote doubled
        assert lr.newick(sid, made) == b"(a:0.200000,('b c':0.100000,'d''x':0.100000):0.100000);\ne;\n"
        assert lr.flat_text(sid, lr.labels_at(4, made, 1700)) == b"a a\nb c b c\nb c d'x\ne e\n"
    # average linkage at a height that is no integer: S = 5001 over 2 x 1 pairs -- as text, one rounded division
    made = [(0, 1, 10, 1, 2, 1), (0, 2, 5001, 2, 3, 2)]
    assert lr.text(['x', 'y', 'z'], made).split(b'\n')[2] == b'x z 0.8529 3' and f'{1 - 5001 / 34000:.4f}' == '0.8529'
    assert lr.newick(['x', 'y', 'z'], made) == b'((x:0.000588,y:0.000588):0.146500,z:0.147088);\n'


def test_the_product_composes_the_same_texts():
    """dct_sim.Dendrogram's composers on given merges (no device): the rule's bytes."""
    from dctdomain_amd import dct_sim
    sid, key = _four()
    for method in lr.METHODS:
        made, _ = lr.rounds(key, 16999, method)
        tree = dct_sim.Dendrogram(sid, np.arange(5), np.zeros((4, 3), dtype=np.int8), method=method)
        tree._merges = tuple(np.array(v, dtype=np.int64) for v in zip(*lr.ordered(made)))
        got = []
        tree.write(got.append)
        assert b'#rep1 rep2 similarity size\n' + b''.join(got) == lr.text(sid, made) and dct_sim.HAC_HEADER == '#rep1 rep2 similarity size'
        assert tree.newick().encode() == lr.newick(sid, made)
        assert tree.heights() == [(m[2], m[3]) for m in lr.ordered(made)]
        for bound_cut in (None, 0.9, 0.85):
            bound = 16999 if bound_cut is None else dct_sim.sim_bound(bound_cut)
            lab = tree.labels(bound_cut)
            assert np.array_equal(lab, lr.labels_at(4, made, bound))
            assert b''.join(bytes(p) for p in dct_sim.cluster_lines(sid, lab)) == lr.flat_text(sid, lab)
        low = dct_sim.Dendrogram(sid, np.arange(5), np.zeros((4, 3), dtype=np.int8), method=method, min_cut=0.9)
        low._merges = tree._merges
        with pytest.raises(ValueError, match='bound 1700'):
            low.labels(0.5)


def test_dendrogram_of_nothing_needs_no_device():
    from dctdomain_amd import dct_sim
    fps = np.zeros((1, 8), dtype=np.int8)
    for sid, idx in (([], [0]), (['only'], [0, 1])):
        for method in lr.METHODS:
            tree = dct_sim.Dendrogram(sid, np.array(idx), fps, method=method)
            assert all(len(v) == 0 for v in tree.merges()) and len(tree.merges()) == 6 and tree.rounds == 0
            assert tree.labels().tolist() == list(range(len(sid))) and tree.heights() == []
            assert tree.newick() == ''.join(f'{s};\n' for s in sid)
    tree = dct_sim.Dendrogram(['a', 'b'], np.array([0, 1, 2]), np.zeros((2, 8), dtype=np.int8), min_cut=1.5)      # bound -1: nothing can merge
    assert tree.bound == -1 and len(tree.merges()[0]) == 0 and tree.labels().tolist() == [0, 1]
    with pytest.raises(ValueError):
        dct_sim.Dendrogram([], np.array([0]), fps, method='single')
    with pytest.raises(ValueError):
        dct_sim.Dendrogram([], np.array([0]), fps, score='both')


def test_too_many_proteins_is_a_value_error_that_names_the_limit():
    from dctdomain_amd import dct_sim
    n = 46341
    tree = dct_sim.Dendrogram(None, np.zeros(n + 1, dtype=np.int64), np.zeros((0, 8), dtype=np.int8), method='complete')
    with pytest.raises(ValueError, match='46340'):
        tree.merges()
    assert tree.matrix_bytes() == n * n * 4
    assert dct_sim.Dendrogram(None, np.zeros(11, dtype=np.int64), np.zeros((0, 8), dtype=np.int8)).matrix_bytes() == 800


# ---- the command line

def _parse(argv):
    from dctdomain_amd import dct_sim
    return vars(dct_sim.build_parser().parse_args(['--dct', 'x-dct.npz'] + argv))


def _refused(argv, capsys):
    with pytest.raises(SystemExit):
        _parse(argv)
    return capsys.readouterr().err.strip().splitlines()[-1].split('error: ', 1)[1]


def test_parser_accepts(capsys):
    base = _parse([])
    assert not {'hac', 'method', 'flat', 'newick'} & set(base)    # absent unless given: every older command line parses as before
    assert _parse(['--hac']) == dict(base, hac='domain')
    assert _parse(['--hac', 'global']) == dict(base, hac='global')
    assert _parse(['--hac', '--method', 'complete']) == dict(base, hac='domain', method='complete')
    assert _parse(['--hac', '--method', 'average', '--min-domain', '0.5']) == dict(base, hac='domain', method='average', min_domain=0.5)
    assert _parse(['--hac', 'global', '--min-global', '0.6', '--flat']) == dict(base, hac='global', min_global=0.6, flat=True)
    assert _parse(['--hac', '--newick', 't.nwk', '--output', 'o']) == dict(base, hac='domain', newick='t.nwk', output='o')
    assert _parse(['--hac', 'domain', '--min-domain', '0.5', '--flat', '--newick', 't.nwk', '--method', 'complete']) == dict(
        base, hac='domain', min_domain=0.5, flat=True, newick='t.nwk', method='complete')


def test_parser_refuses(capsys):
    hac = '--hac prints the average- or complete-linkage tree of --dct: not with '
    for flag, rest in (('--pair', ['p']), ('--db', ['d']), ('--cluster', []), ('--assign', ['r']), ('--rank', ['domain']),
                       ('--linkage', ['single']), ('--level', ['protein']), ('--no-whole', []), ('--reps-out', ['f']), ('--domains', []),
                       ('--dom', ['f']), ('--db-dom', ['f']), ('--domain-map', []), ('--min-coverage', ['0.5']), ('--cov-unit', ['domains']),
                       ('--rep', ['medoid']), ('--min-neighbors', ['2']), ('--zscore', []), ('--min-z', ['1'])):
        got = _refused(['--hac', flag] + rest, capsys)
        if flag == '--assign':                                   # (a mode of its own, checked before --hac: it refuses --hac)
            assert got == '--assign places the proteins of --dct on a fixed set of representatives: not with --hac'
        else:
            assert got == hac + flag, flag
    # the other modes refuse --hac and what goes with it
    assert _refused(['--hac', '--tree'], capsys) == '--tree prints the single-linkage tree of --dct: not with --hac'
    assert _refused(['--hac', '--hist'], capsys) == '--hist bins the scores of all pairs of --dct: not with --hac'
    assert _refused(['--hac', '--auc1', '--family-sep', '|'], capsys) == '--auc1 measures the AUC1 and the top-1 rates of --dct: not with --hac'
    assert _refused(['--hac', '--db', 'd', '--rbh'], capsys) == '--rbh prints the reciprocal best hits of --dct and --db: not with --hac'
    for mode in (['--tree'], ['--hist'], ['--assign', 'r', '--min-domain', '0.5'], ['--db', 'd', '--rbh'], ['--auc1', '--family-sep', '|']):
        for flag, rest in (('--method', ['complete']), ('--flat', []), ('--newick', ['f'])):
            assert _refused(mode + [flag] + rest, capsys).endswith(': not with ' + flag), (mode, flag)
    # the three options need --hac
    assert _refused(['--method', 'complete'], capsys) == '--method says which linkage the tree of --hac is built by: it needs --hac'
    assert _refused(['--cluster', '--min-domain', '0.5', '--flat'], capsys) == '--flat prints the clusters of --hac at its cut-off: it needs --hac'
    assert _refused(['--newick', 'f'], capsys) == '--newick writes the tree of --hac in Newick format: it needs --hac'
    assert _refused(['--pair', 'p', '--method', 'average'], capsys).endswith('it needs --hac')
    # only the cut-off of its own score; --flat needs it
    assert _refused(['--hac', '--min-global', '0.5'], capsys) == '--hac domain orders the pairs by DCTdomain: its cut-off is --min-domain, not --min-global'
    assert _refused(['--hac', 'global', '--min-domain', '0.5'], capsys) == '--hac global orders the pairs by DCTglobal: its cut-off is --min-global, not --min-domain'
    assert _refused(['--hac', '--flat'], capsys) == '--flat prints the clusters at a cut-off: with --hac domain it needs --min-domain'
    assert _refused(['--hac', 'global', '--flat'], capsys) == '--flat prints the clusters at a cut-off: with --hac global it needs --min-global'
    assert 'invalid choice' in _refused(['--hac', '--method', 'single'], capsys)
    assert 'invalid choice' in _refused(['--hac', 'both'], capsys)
    # --linkage is not extended
    assert 'invalid choice' in _refused(['--cluster', '--min-domain', '0.5', '--linkage', 'complete'], capsys)


def test_hac_sim_checks_its_arguments_before_it_loads_anything():
    from dctdomain_amd import dct_sim
    for kw in ({'method': 'single'}, {'score': 'both'}, {'min_global': 0.5}, {'score': 'global', 'min_domain': 0.5}, {'flat': True},
               {'flat': True, 'score': 'global', 'min_domain': None}):
        with pytest.raises(ValueError):
            dct_sim.hac_sim('no-such-file.npz', None, **kw)


# ---- the native pieces

def test_header_exports_and_the_untouched_main_header():
    from dctdomain_amd import _lib
    import build_ext
    with open(os.path.join(ROOT, 'include', 'dctfp_linkage.h')) as fh:
        header = fh.read()
    assert '#include "dctfp.h"' in header and re.search(r'#define DCTFP_LINKAGE_VERSION 1\b', header)
    assert sorted(set(re.findall(r'^int (dctfp_\w+)\(', header, re.M))) == sorted(_lib.LINKAGE_EXPORTS)
    for name in ('dctfp_linkage_nearest', 'dctfp_linkage_merge'):
        doc = header.split(f'\nint {name}(')[0].rsplit('/*', 1)[1]
        assert 'DCTFP_ERR_LIMIT' in doc and 'DCTFP_ERR_INVALID' in doc and '46340' in doc and re.fullmatch(r'\s*', doc.split('*/', 1)[1])
        decl = header.split(f'\nint {name}(')[1].split(');')[0]
        assert decl.startswith('dctfp_ctx* ctx') and decl.rstrip().endswith('void* stream')
    with open(os.path.join(ROOT, 'include', 'dctfp.h')) as fh:
        main = fh.read()
    assert '#define DCTFP_VERSION 117 ' in main and 'dctfp_linkage' not in main
    for path in (_lib.LIB_PATH, _lib.EXPERIMENTS_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert all(hasattr(lib, name) for name in _lib.LINKAGE_EXPORTS)
        assert lib.dctfp_linkage_version() == 1 == _lib.DCTFP_LINKAGE_VERSION and lib.dctfp_version() == 117
    lib = _lib._configure(ctypes.CDLL(_lib.LIB_PATH))
    assert len(lib.dctfp_linkage_nearest.argtypes) == 11 and len(lib.dctfp_linkage_merge.argtypes) == 10
    assert lib.dctfp_linkage_nearest.restype is ctypes.c_int and lib.dctfp_linkage_merge.restype is ctypes.c_int
    assert not set(_lib.LINKAGE_EXPORTS) & set(_lib.EXPORTS)
    csrc = os.path.join(ROOT, 'dctdomain_amd', 'csrc')
    assert 'k_linkage.hip' in build_ext.UNITS and 'k_linkage.hip' not in build_ext.TWIN_UNITS
    assert os.path.join(ROOT, 'include', 'dctfp_linkage.h') in build_ext.HEADERS
    assert os.path.join(csrc, 'k_linkage.hip') in build_ext.kernel_sources()
    with open(os.path.join(csrc, 'k_linkage.hip')) as fh:
        unit = fh.read()
    assert 'atomic' not in unit.split('#define DCTFP_TEMPLATES_ONLY')[1].lower()          # plain loads and stores, no tickets
    assert '__syncthreads' in unit and '__shfl_xor' in unit


def test_a_library_without_the_exports_fails_clearly():
    from dctdomain_amd import _lib
    with pytest.raises(ImportError, match='dctfp_linkage_nearest'):
        _lib._configure(ctypes.CDLL(_lib.RECCUT_LIB_PATH))
