"""CPU-side checks of dct-sim --domain-map: the rule (domain_map_rule.py, the GPU tests' oracle) on the committed fixtures and on
hand-made cases, the host composer ``dct_sim.map_field`` against literal strings, the command line, and the two entry points in the
header and the libraries."""

import contextlib
import ctypes
import io
import os
import re

import numpy as np
import pytest

import domain_map_rule as rule
import golden_util as gu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(gu.GOLD, 'ref_fixtures')


def _fixture(name):
    with np.load(os.path.join(FIX, name)) as data:
        return [str(s) for s in data['sid']], np.asarray(data['idx'], dtype=np.int64), data['dct'], [str(s) for s in data['dom']]


def _row_with_l1(v, width=480):
    """A row at L1 ``v`` from the zero row."""
    row = np.zeros(width, dtype=np.int8)
    q, r = divmod(int(v), 127)
    row[:q] = 127
    row[q] = r
    return row


# ---- the rule

def test_bound_is_evaluated_not_derived():
    from dctdomain_amd import dct_sim
    assert (rule.bound(0.5), rule.bound(0.25), rule.bound(1), rule.bound(1e-9), rule.bound(0)) == (8500, 12750, 0, 16999, 16999)
    for x in (0.5, 0.25, 1, 1e-9, 0.3, 0.7, 0.999, 0.1, 1 / 3):
        assert dct_sim.map_bound(x) == rule.bound(x) == min(dct_sim.sim_bound(x), 16999)
    # X: the option's own value, else --min-domain, else 0.25; the bare flag parses to True
    assert dct_sim.map_bound() == dct_sim.map_bound(True) == dct_sim.map_bound(None, None) == 12750 and dct_sim.MAP_SIMILARITY == 0.25
    assert dct_sim.map_bound(True, 0.5) == dct_sim.map_bound(None, 0.5) == 8500 and dct_sim.map_bound(0.25, 0.5) == 12750
    assert dct_sim.map_bound(None, 0.0) == 16999 and dct_sim.map_bound(None, 1.5) == -1     # (similarity 0 never matches; nothing reaches 1.5)


@pytest.mark.parametrize('name,pairs,want', [
    ('G6PD-dct.npz', 351, {8500: (869, 869, 0), 12750: (1495, 1496, 0), 16999: (2801, 2945, 0)}),
    ('example-dct.npz', 28, {8500: (3, 3, 27), 12750: (6, 6, 26), 16999: (108, 193, 0)}),
])
def test_rule_counts_on_the_committed_fixtures(name, pairs, want):
    """The counts of the issue; the product's ``map_entries`` selects the same rows from the rule's arrays."""
    from dctdomain_amd import dct_sim
    sid, idx, dct, _ = _fixture(name)
    n = len(idx) - 1
    listed = [(i, j) for i in range(n) for j in range(i + 1, n)]
    assert len(listed) == pairs
    off, l1, arg = rule.flat(dct, idx, dct, idx, listed)
    got = {b: [0, 0, 0] for b in want}
    tied = 0
    for p, (i, j) in enumerate(listed):
        a, b = dct[idx[i]:idx[i + 1]].astype(np.int64), dct[idx[j]:idx[j + 1]].astype(np.int64)
        d = np.abs(a[:, None] - b[None]).sum(2)
        tied += int(((d == d.min(1, keepdims=True)).sum(1) > 1).sum() + ((d == d.min(0, keepdims=True)).sum(0) > 1).sum())
        mid = off[p] + len(a)
        assert l1[off[p]:mid].tolist() == d.min(1).tolist() and l1[mid:off[p + 1]].tolist() == d.min(0).tolist()
        for bound in want:
            first, second = rule.sides(a, b, bound)
            assert dct_sim.map_entries(l1[off[p]:mid], arg[off[p]:mid], bound) == first
            assert dct_sim.map_entries(l1[mid:off[p + 1]], arg[mid:off[p + 1]], bound) == second
            got[bound][0] += len(first)
            got[bound][1] += len(second)
            got[bound][2] += not first and not second
    assert {b: tuple(v) for b, v in got.items()} == want
    if name.startswith('G6PD'):
        assert tied == 0                                        # (ties: the hand-made cases below)


def test_rule_on_the_example_of_the_readme():
    sid, idx, dct, dom = _fixture('G6PD-dct.npz')
    i, j = sid.index('A0A2K6GTL0'), sid.index('A0A341BUD1')
    names = [WHOLE if r + 1 in idx[1:] else s for r, s in enumerate(dom)]
    text = rule.file_field(dct, idx, names, dct, idx, names, i, j, rule.bound(0.5), rule.all_text)
    assert text.split('/')[0] == '1-34=1-27:0.504;35-219=28-211:0.884;220-407=212-366:0.641;533-781=594-840:0.876;whole=whole:0.805'
    first, _ = rule.sides(dct[idx[i]:idx[i + 1]], dct[idx[j]:idx[j + 1]], rule.bound(0.5))
    assert [(r, c) for r, c, _ in first] == [(0, 0), (1, 1), (2, 2), (5, 6), (6, 7)]
    assert min(first, key=lambda e: e[2])[:2] == (1, 1)         # (--domains: "2 2")


WHOLE = 'whole'


def test_rule_ties_go_to_the_lowest_row_on_both_sides():
    rng = np.random.default_rng(11)
    x, y = rng.integers(-40, 41, size=(2, 480)).astype(np.int8)
    p, q = np.stack([x, y, x]), np.stack([y, x, x, y])
    assert rule.row_best(p, q) == ([0, 0, 0], [1, 0, 1], [0, 0, 0, 0], [1, 0, 0, 1])
    first, second = rule.sides(p, q, 0)
    assert first == [(0, 1, 0), (1, 0, 0), (2, 1, 0)] and second == [(0, 1, 0), (1, 0, 0), (2, 0, 0), (3, 1, 0)]


def test_rule_empty_and_one_row_proteins():
    none, one = np.zeros((0, 480), dtype=np.int8), np.zeros((1, 480), dtype=np.int8)
    assert rule.row_best(none, none) == ([], [], [], [])
    assert rule.row_best(one, none) == ([rule.NO_L1], [rule.NONE], [], [])
    assert rule.row_best(none, one) == ([], [], [rule.NO_L1], [rule.NONE])
    assert rule.sides(one, none, 16999) == ([], []) and rule.field(one, none, 16999, ['1'], []) == '-/-'
    assert rule.row_best(one, one) == ([0], [0], [0], [0]) and rule.field(one, one, 0, ['1'], ['1']) == '1=1:1.0/1=1:1.0'


@pytest.mark.parametrize('x,bound', [(0.5, 8500), (0.25, 12750), (1e-9, 16999), (1, 0)])
def test_rule_cut_off_edges(x, bound):
    """An L1 of exactly B matches, B + 1 does not; 16999 is the last L1 that can match, whatever X; --domain-map 1: only L1 = 0."""
    from dctdomain_amd import dct_sim
    assert rule.bound(x) == bound == dct_sim.map_bound(x)
    zero = np.zeros((1, 480), dtype=np.int8)
    at, over = _row_with_l1(bound)[None], _row_with_l1(bound + 1)[None]
    assert rule.sides(zero, at, bound) == ([(0, 0, bound)], [(0, 0, bound)])
    assert rule.sides(zero, over, bound) == ([], [])
    assert dct_sim.map_entries([bound, bound + 1, 17000, rule.NO_L1], [0, 1, 2, -1], bound) == [(0, 0, bound)]
    if bound == 16999:
        assert rule.sides(zero, _row_with_l1(17000)[None], rule.bound(0)) == ([], [])


# ---- the host composer

def test_map_field_literals():
    from dctdomain_amd import dct_sim
    f = dct_sim.map_field
    idx3, idx2 = ['1', '2', '3'], ['1', '2']
    assert f([(0, 1, 8500), (2, 0, 0)], [(1, 0, 8500)], idx3, idx2) == '1=2:0.5;3=1:1.0/2=1:0.5'
    assert f([], [], idx3, idx2) == '-/-' and f([], [], [], []) == '-/-'
    assert f([(1, 0, 4250)], [], idx3, idx2) == '2=1:0.75/-' and f([], [(0, 2, 4250)], idx3, idx2) == '-/1=3:0.75'
    dom_a, dom_b = ['1-30,61-100', '31-60', WHOLE], ['1-80', WHOLE]
    assert f([(0, 0, 1700), (2, 1, 3400)], [(0, 0, 1700), (1, 2, 3400)], dom_a, dom_b) == \
        '1-30,61-100=1-80:0.9;whole=whole:0.8/1-80=1-30,61-100:0.9;whole=whole:0.8'
    # the all-against-all's text of an L1: the five characters of the first half of score_table()
    table = dct_sim.score_table()
    five = lambda l1: bytes(table[0, l1]).decode()
    assert f([(0, 0, 8432)], [(0, 0, 8432)], ['1'], ['1'], five) == '1=1:0.504/1=1:0.504'
    for l1 in (0, 1, 8500, 12750, 16999):
        assert five(l1) == rule.all_text(l1) and str(dct_sim._sim1(l1)) == rule.pair_text(l1)


def test_map_field_is_the_rule_on_a_fixture():
    from dctdomain_amd import dct_sim
    sid, idx, dct, _ = _fixture('example-dct.npz')
    names = dct_sim.fingerprint_labels(sid, idx, dct_sim.read_dom_file(os.path.join(FIX, 'example.dom')))
    n = len(idx) - 1
    listed = [(i, j) for i in range(n) for j in range(n)]
    got = dct_sim._map_fields(*rule.flat(dct, idx, dct, idx, listed), 12750, listed, names, idx, names, idx)
    assert got == [rule.file_field(dct, idx, names, dct, idx, names, i, j, 12750) for i, j in listed]
    assert sum(g != '-/-' for g in got) == 8 + 2 * 2            # (every protein with itself, and two pairs, both ways)


def test_text_room_bounds_every_line_with_its_map():
    """What sizes the ranges of rows in FilteredPairs.chunks(): at least the longest line either protein can be part of."""
    from dctdomain_amd import dct_sim
    sid, idx, dct, _ = _fixture('example-dct.npz')
    names = dct_sim.fingerprint_labels(sid, idx, dct_sim.read_dom_file(os.path.join(FIX, 'example.dom')))
    job = dct_sim.FilteredPairs(sid, idx, dct, labels=names)
    with pytest.raises(ValueError, match='16999'):
        job.with_map(17000)
    with pytest.raises(ValueError, match='labels'):
        dct_sim.FilteredPairs(sid, idx, dct).with_map(8500)
    assert job.map_l1 is None and job.with_map(16999) is job and job.map_l1 == 16999
    room = job._map_room()
    for i in range(len(sid)):
        for j in range(len(sid)):
            first, second = rule.file_field(dct, idx, names, dct, idx, names, i, j, 16999, rule.all_text).split('/')
            assert len(first) <= room[i] and len(second) <= room[j]


# ---- the command line

def test_flagless_namespace_is_unchanged_and_the_option_implies_domains():
    from dctdomain_amd import dct_sim
    parse = dct_sim.build_parser().parse_args
    assert vars(parse(['--dct', 'x.npz'])) == {'dct': 'x.npz', 'output': None, 'pair': None, 'pairfound': None, 'db': None, 'top': 5,
                                               'threshold': 0.25, 'rank': None, 'min_domain': None, 'min_global': None, 'cluster': False}
    assert not hasattr(parse(['--dct', 'x.npz', '--domains']), 'domain_map')
    for argv, want in ((['--domain-map'], True), (['--domain-map', '0.5'], 0.5), (['--domain-map', '1'], 1.0),
                       (['--pair', 'p.txt', '--domain-map', '0.3'], 0.3), (['--db', 'y.npz', '--rank', 'domain', '--zscore', '--domain-map'], True),
                       (['--db', 'y.npz', '--rbh', '--min-domain', '0.5', '--domain-map', '--min-z', '2'], True),
                       (['--min-domain', '0.5', '--min-coverage', '0.8', '--cov-unit', 'domains', '--domain-map'], True),
                       (['--domain-map', '--dom', 'x.dom'], True)):
        args = parse(['--dct', 'x.npz'] + argv)
        assert args.domain_map == want and type(args.domain_map) is type(want) and args.domains is True


@pytest.mark.parametrize('argv,message', [
    (['--min-domain', '0.5', '--cluster', '--domain-map'], '--domain-map lists the matched domain pairs behind a result line: not with --cluster'),
    (['--tree', '--domain-map'], '--tree prints the single-linkage tree of --dct: not with --domain-map'),
    (['--assign', 'r.npz', '--min-domain', '0.5', '--domain-map', '0.5'],
     '--assign places the proteins of --dct on a fixed set of representatives: not with --domain-map'),
    (['--auc1', '--family-sep', '|', '--domain-map'], '--auc1 measures the AUC1 and the top-1 rates of --dct: not with --domain-map'),
    (['--hist', '--domain-map'], '--hist bins the scores of all pairs of --dct: not with --domain-map'),
    (['--domain-map', '0'], '--domain-map X is the similarity from which a domain is matched: above 0 and at most 1'),
    (['--domain-map', '1.01'], 'above 0 and at most 1'),
    (['--domain-map', '-0.5'], 'above 0 and at most 1'),
    (['--domain-map', 'nan'], 'above 0 and at most 1'),
    (['--pair', 'p.txt', '--domain-map', 'x'], 'invalid float value'),
])
def test_parser_rejects(argv, message, capsys):
    from dctdomain_amd import dct_sim
    with pytest.raises(SystemExit) as e:
        dct_sim.build_parser().parse_args(['--dct', 'x.npz'] + argv)
    assert e.value.code == 2
    assert message in capsys.readouterr().err


DOES = {'--rbh': '--rbh prints the reciprocal best hits of --dct and --db', '--tree': '--tree prints the single-linkage tree of --dct',
        '--assign': '--assign places the proteins of --dct on a fixed set of representatives',
        '--auc1': '--auc1 measures the AUC1 and the top-1 rates of --dct', '--hist': '--hist bins the scores of all pairs of --dct'}
MODE_ARGV = {'--rbh': ['--db', 'y.npz', '--rbh'], '--tree': ['--tree'], '--assign': ['--assign', 'r.npz', '--min-domain', '0.5'],
             '--auc1': ['--auc1', '--family-sep', '|'], '--hist': ['--hist']}
FLAG_ARGV = {'--pair': ['--pair', 'p'], '--db': ['--db', 'y'], '--cluster': ['--cluster'], '--assign': ['--assign', 'r'], '--tree': ['--tree'],
             '--rank': ['--rank', 'domain'], '--linkage': ['--linkage', 'single'], '--level': ['--level', 'protein'], '--no-whole': ['--no-whole'],
             '--reps-out': ['--reps-out', 'o'], '--domains': ['--domains'], '--dom': ['--dom', 'f'], '--db-dom': ['--db-dom', 'f'],
             '--domain-map': ['--domain-map'], '--min-coverage': ['--min-coverage', '0.5'], '--cov-unit': ['--cov-unit', 'domains'],
             '--rep': ['--rep', 'first'], '--min-neighbors': ['--min-neighbors', '3'], '--zscore': ['--zscore'], '--min-z': ['--min-z', '2'],
             '--auc1': ['--auc1'], '--hist': ['--hist']}
TREE_REFUSES = ('--pair', '--db', '--cluster', '--assign', '--rank', '--linkage', '--level', '--no-whole', '--reps-out', '--domains', '--dom',
                '--db-dom', '--domain-map', '--min-coverage', '--cov-unit', '--rep', '--min-neighbors', '--zscore', '--min-z', '--auc1', '--hist')
# what each of the four modes checked before --hist refuses beside --hist (a mode checked earlier names the pair itself: --tree beside
# --assign, --assign beside --auc1)
REFUSES_BESIDE_HIST = {
    '--rbh': ('--pair', '--cluster', '--assign', '--tree', '--rank', '--linkage', '--level', '--no-whole', '--reps-out', '--min-coverage',
              '--cov-unit', '--rep', '--min-neighbors', '--auc1'),
    '--tree': TREE_REFUSES[:-1],
    '--assign': tuple(f for f in TREE_REFUSES[:-1] if f not in ('--assign', '--reps-out')),
    '--auc1': tuple(f for f in TREE_REFUSES[:-1] if f not in ('--assign', '--auc1'))}


def _refusal(argv):
    from dctdomain_amd import dct_sim
    err = io.StringIO()
    with pytest.raises(SystemExit) as e, contextlib.redirect_stderr(err):
        dct_sim.build_parser().parse_args(['--dct', 'x.npz'] + argv)
    assert e.value.code == 2
    return err.getvalue().rstrip('\n').rsplit(': error: ', 1)[1]


def test_the_option_is_no_mode_and_stands_behind_db_dom():
    from dctdomain_amd import dct_sim
    parse = dct_sim.build_parser().parse_args
    # no mode: alone it is the all-against-all with one more column; and the five modes are checked with --hist last
    assert vars(parse(['--dct', 'x.npz', '--domain-map'])) == dict(vars(parse(['--dct', 'x.npz'])), domain_map=True, domains=True)
    for mode in ('--rbh', '--tree', '--assign', '--auc1'):
        assert _refusal(MODE_ARGV[mode] + ['--hist']) == f'{DOES[mode]}: not with --hist'
    for mode in ('--tree', '--assign', '--auc1', '--hist'):
        # given as the bare flag and with X, not without it
        assert _refusal(MODE_ARGV[mode] + ['--domain-map']) == _refusal(MODE_ARGV[mode] + ['--domain-map', '0.5']) == f'{DOES[mode]}: not with --domain-map'
        assert 'domain_map' not in vars(parse(['--dct', 'x.npz'] + MODE_ARGV[mode]))
        # named behind --db-dom; --min-neighbors, --zscore and --min-z in that order
        for first, second in (('--db-dom', '--domain-map'), ('--min-neighbors', '--zscore'), ('--zscore', '--min-z')):
            assert _refusal(MODE_ARGV[mode] + FLAG_ARGV[second] + FLAG_ARGV[first]) == f'{DOES[mode]}: not with {first}'
    assert parse(['--dct', 'x.npz'] + MODE_ARGV['--rbh'] + ['--domain-map']).domain_map is True     # (--rbh prints pair lines: it takes the option)
    # --hist is the last flag the four name: beside any other flag they refuse, that one is named
    for mode, others in REFUSES_BESIDE_HIST.items():
        for flag in others:
            assert _refusal(MODE_ARGV[mode] + ['--hist'] + FLAG_ARGV[flag]) == f'{DOES[mode]}: not with {flag}'
    # --hist refuses what --tree refuses, minus itself (beside --assign and --auc1 those two, checked before it, say so)
    for flag in TREE_REFUSES[:-1]:
        assert _refusal(['--tree'] + FLAG_ARGV[flag]) == f'{DOES["--tree"]}: not with {flag}'
        got = _refusal(['--hist'] + FLAG_ARGV[flag] + (['--family-sep', '|'] if flag == '--auc1' else []))
        assert got == (f'{DOES[flag]}: not with --hist' if flag in ('--assign', '--auc1') else f'{DOES["--hist"]}: not with {flag}')
    assert '--domain-map [X]' in dct_sim.build_parser().format_help()


def test_header_text(tmp_path):
    from dctdomain_amd import dct_sim
    assert dct_sim._header(dct_sim.HEADER, None, True, True) == '#prot1 prot2 sim-domain sim-global dom1 dom2 domain-map'
    assert dct_sim._header(dct_sim.HEADER, None, True, 0.5) == dct_sim.DOMAIN_HEADER + ' domain-map'
    assert dct_sim._header(dct_sim.HEADER, None, True) == dct_sim.DOMAIN_HEADER and dct_sim._header(dct_sim.HEADER) == dct_sim.HEADER
    assert dct_sim._header(dct_sim.CLUSTER_HEADER, None, False, None) == dct_sim.CLUSTER_HEADER
    # a report a mode function opens itself (the header is that of the mode of its name): the z columns stay last
    seen = []

    def all_sim(report, **kw):
        seen.append(kw)

    def db_search(report, **kw):
        seen.append(kw)

    def rbh_sim(report, **kw):
        seen.append(kw)

    for fn, kw, want in ((all_sim, {'domain_map': True}, ' dom1 dom2 domain-map'), (db_search, {'domain_map': 0.5, 'zscore': True, 'rank': 'domain'},
                                                                                     ' dom1 dom2 domain-map z-domain'),
                         (rbh_sim, {'domain_map': True, 'min_z': 1.0}, ' dom1 dom2 domain-map z-query z-db'), (all_sim, {'domains': True}, ' dom1 dom2'),
                         (all_sim, {}, '')):
        path = tmp_path / 'out.txt'
        dct_sim._reporting(fn)(str(path), **kw)
        assert path.read_text() == dct_sim.HEADER + want + '\n' and seen[-1] == kw
        assert dct_sim.mode_header(fn.__name__, kw) == dct_sim.HEADER + want


# ---- the entry points

@pytest.mark.parametrize('name,params,sibling', [
    ('dctfp_pair_row_best', 'dctfp_ctx* ctx, const int32_t* pairs, int64_t n_pairs, const int8_t* a, int64_t lda, const int64_t* idx_a, '
                            'int64_t npa, const int8_t* b, int64_t ldb, const int64_t* idx_b, int64_t npb, int32_t d, const int64_t* row_off, '
                            'int64_t out_len, int32_t* out_l1, int32_t* out_arg, void* stream', 'dctfp_pair_argmin'),
    ('dctfp_pair_map_lines', 'dctfp_ctx* ctx, int64_t n_lines, const int32_t* pi, const int32_t* pj, const int32_t* mn, '
                             'const int32_t* last, const int32_t* la, const int32_t* lb, const uint8_t* ids, const int64_t* id_off, '
                             'int64_t n_ids, const uint8_t* labels, const int64_t* label_off, int64_t n_labels, const char* table, '
                             'const int64_t* line_off, uint8_t* out, int64_t out_bytes, const int64_t* row_off, int64_t n_rows, '
                             'const int32_t* row_l1, const int32_t* row_arg, const int64_t* first_row, int32_t bound, int64_t* out_count, '
                             'void* stream', 'dctfp_pair_domain_lines'),
])
def test_library_exports_the_entry_points_and_header_documents_them(name, params, sibling):
    from dctdomain_amd import _lib
    with open(os.path.join(ROOT, 'include', 'dctfp.h')) as fh:
        header = fh.read()
    decl = re.search(r'int %s\(([^;]*)\);' % name, header)
    assert decl and ' '.join(decl.group(1).split()) == params
    doc = header[:decl.start()].rsplit('/*', 1)[1]
    assert '*/' in doc and 'DCTFP_ERR_LIMIT' in doc and sibling in doc
    assert re.fullmatch(r'\s*', doc.split('*/', 1)[1]), 'the comment must sit right above the declaration'
    sib = ' '.join(re.search(r'int %s\(([^;]*)\);' % sibling, header).group(1).split())
    if name == 'dctfp_pair_row_best':                           # (the sibling's arguments up to d, then its own)
        assert params.startswith(sib.split(', int32_t* out_min')[0] + ', ')
    else:                                                       # (the sibling's arguments, then its own)
        assert params.startswith(sib.replace(', void* stream', ', '))
    assert int(re.search(r'#define DCTFP_VERSION (\d+)', header).group(1)) == 117
    for path in (_lib.LIB_PATH, _lib.EXPERIMENTS_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert hasattr(lib, name)
        assert lib.dctfp_version() == 117
    assert name in _lib.EXPORTS
    with open(os.path.join(ROOT, 'dctdomain_amd', 'csrc', 'launch.h')) as fh:
        assert 'launch_' + name[len('dctfp_'):] + '(' in fh.read()
    with open(os.path.join(ROOT, 'INTEGRATION.md')) as fh:
        assert '`%s`' % name in fh.read()


def test_the_unit_is_built_once_for_both_libraries():
    import build_ext
    assert 'k_map.hip' in build_ext.UNITS and 'k_map.hip' not in build_ext.TWIN_UNITS
    assert os.path.exists(os.path.join(build_ext.CSRC, 'k_map.hip'))


def test_binding_declares_one_argument_type_per_parameter():
    import ctypes as C
    from dctdomain_amd import _lib
    lib = _lib._configure(C.CDLL(_lib.LIB_PATH))
    best, lines = lib.dctfp_pair_row_best.argtypes, lib.dctfp_pair_map_lines.argtypes
    assert len(best) == 17 and best[:12] == lib.dctfp_pair_argmin.argtypes[:12] and best[12:] == [C.c_void_p, C.c_int64] + [C.c_void_p] * 3
    assert len(lines) == 26 and lines[:18] == lib.dctfp_pair_domain_lines.argtypes[:18]
    assert lines[18:] == [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    assert lib.dctfp_pair_row_best.restype == C.c_int and lib.dctfp_pair_map_lines.restype == C.c_int


def test_null_and_bad_arguments_are_refused_without_a_device():
    """The argument checks stand in front of every HIP call: a NULL context is DCTFP_ERR_INVALID on any machine."""
    import ctypes as C
    from dctdomain_amd import _lib
    lib = _lib._configure(C.CDLL(_lib.LIB_PATH))
    assert lib.dctfp_pair_row_best(None, None, 0, None, 0, None, 0, None, 0, None, 0, 0, None, 0, None, None, None) == _lib.DCTFP_ERR_INVALID
    assert b'dctfp_pair_row_best: NULL argument' in lib.dctfp_last_error()
    assert lib.dctfp_pair_map_lines(None, 0, *([None] * 8), 0, None, None, 0, None, None, None, 0, None, 0, None, None, None, 0, None,
                                    None) == _lib.DCTFP_ERR_INVALID
    assert b'dctfp_pair_map_lines: NULL argument' in lib.dctfp_last_error()
