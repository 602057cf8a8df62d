"""CPU-side checks of dct-sim --tree: the numpy oracle (tree_rule.py, the GPU tests' reference) pinned on the committed reference
golden -- cut at any bound it gives cluster_rule's labels, its lines are lines of the reference's all-against-all --, the command
line, the cases that need no device, and the two entry points in the libraries and the header."""

import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import all_sim_filter_rule as rule
import cluster_rule as crule
import golden_util as gu
import tree_rule as trule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPZ = os.path.join(gu.GOLD, 'all_sim', 'all-dct.npz')
N = 139


@pytest.fixture(scope='module')
def golden():
    with np.load(NPZ) as data:
        sid, idx, dct = [str(s) for s in data['sid']], np.asarray(data['idx'], dtype=np.int64), data['dct']
    return sid, idx, dct, rule.triangle_l1(dct, idx)


# ---- the oracle on the reference's 139 proteins

@pytest.mark.parametrize('score', ['domain', 'global'])
def test_oracle_cut_at_any_bound_gives_the_clusters(golden, score):
    from dctdomain_amd import dct_sim
    sid, idx, dct, tri = golden
    i, j, key = trule.edges(dct, idx, score, triangle=tri)
    assert (i < j).all() and key.max() <= trule.DEFAULT_BOUND
    assert np.array_equal(np.lexsort((j, i, key)), np.arange(len(key)))      # (in (key, i, j) order)
    for x in (0.1, 0.5, 0.9, 1.0):
        b = dct_sim.sim_bound(x)
        want, _ = crule.labels(dct, idx, **{'min_' + score: x})
        assert np.array_equal(trule.cut(N, i, j, key, b), want), x
        # a tree built with that cut-off: the same edges up to it, n - components of them
        ci, cj, ck = trule.edges(dct, idx, score, b, triangle=tri)
        keep = key <= b
        assert np.array_equal(ci, i[keep]) and np.array_equal(cj, j[keep]) and np.array_equal(ck, key[keep])
        assert len(ci) == N - len(np.unique(want))
    # at the default bound: n - components of the graph of all pairs of similarity above 0
    all_i, all_j, mn, last = tri
    every = trule.keys(mn, last, score) <= trule.DEFAULT_BOUND
    assert len(i) == N - len(np.unique(crule.components(N, all_i[every], all_j[every])))


@pytest.mark.parametrize('score', ['domain', 'global'])
def test_oracle_lines_are_lines_of_the_all_against_all_in_the_stated_order(golden, score):
    sid, idx, dct, tri = golden
    lines = rule.read_lines(os.path.join(gu.GOLD, 'all_sim', 'expected.txt.gz'))
    assert lines[0] + b'\n' == trule.HEADER and len(lines) == 1 + N * (N - 1) // 2
    i, j, key = trule.edges(dct, idx, score, triangle=tri)
    place = i * N - i * (i + 1) // 2 + (j - i - 1)            # the pair's line in the upper triangle's output order
    got = trule.text(sid, dct, idx, i, j).split(b'\n')[:-1]
    assert got == [lines[1 + k] for k in place.tolist()]
    # most similar first: the printed score of the tree's own column never rises
    col = 2 if score == 'domain' else 3
    shown = [float(x.split()[col]) for x in got]
    assert all(a >= b for a, b in zip(shown, shown[1:])) and shown[0] == 1.0
    # the same forest from scipy's own routine, by total weight (its tie-breaks may differ; the weight cannot)
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import minimum_spanning_tree
    all_i, all_j, mn, last = tri
    k = trule.keys(mn, last, score)
    keep = k <= trule.DEFAULT_BOUND
    mst = minimum_spanning_tree(coo_matrix((k[keep] + 1.0, (all_i[keep], all_j[keep])), shape=(N, N)))      # (+ 1: a key of 0 is an edge)
    assert mst.nnz == len(key) and int(mst.sum()) == int(key.sum()) + len(key)


def test_kruskal_breaks_ties_by_index():
    n = 5
    i, j = np.triu_indices(n, 1)
    ti, tj, tk = trule.kruskal(n, i, j, np.full(len(i), 7), 7)
    assert ti.tolist() == [0, 0, 0, 0] and tj.tolist() == [1, 2, 3, 4] and tk.tolist() == [7] * 4
    assert len(trule.kruskal(n, i, j, np.full(len(i), 7), 6)[0]) == 0


# ---- the command line

def _parse(*argv):
    from dctdomain_amd import dct_sim
    return dct_sim.build_parser().parse_args(['--dct', 'x-dct.npz'] + list(argv))


def test_tree_alone_parses_to_domain_and_is_absent_otherwise():
    assert _parse('--tree').tree == 'domain' and _parse('--tree', 'domain').tree == 'domain' and _parse('--tree', 'global').tree == 'global'
    assert not hasattr(_parse(), 'tree') and not hasattr(_parse('--min-domain', '0.5'), 'tree')
    assert _parse('--tree', '--min-domain', '0.5').min_domain == 0.5
    assert _parse('--tree', 'global', '--min-global', '0.25', '--output', 'o').min_global == 0.25


@pytest.mark.parametrize('argv', [
    ['--tree', '--pair', 'p'], ['--tree', '--db', 'y.npz'], ['--tree', '--cluster', '--min-domain', '0.5'],
    ['--tree', '--assign', 'r.npz', '--min-domain', '0.5'], ['--tree', '--db', 'y.npz', '--rank', 'domain'],
    ['--tree', '--linkage', 'greedy'], ['--tree', '--level', 'domain'], ['--tree', '--no-whole'], ['--tree', '--reps-out', 'r.npz'],
    ['--tree', '--domains'], ['--tree', '--dom', 'x.dom'], ['--tree', '--db-dom', 'y.dom'],
    ['--tree', '--min-global', '0.5'], ['--tree', 'domain', '--min-global', '0.5'], ['--tree', 'global', '--min-domain', '0.5'],
    ['--tree', 'protein'],
], ids=lambda a: ' '.join(a))
def test_parser_errors(argv, capsys):
    with pytest.raises(SystemExit) as exit_:
        _parse(*argv)
    assert exit_.value.code == 2
    err = capsys.readouterr().err
    assert '--tree' in err


def test_tree_sim_refuses_the_other_cut_off_and_an_unknown_score(tmp_path):
    from dctdomain_amd import dct_sim
    for kw in ({'score': 'domain', 'min_global': 0.5}, {'score': 'global', 'min_domain': 0.5}, {'score': 'protein'}):
        with pytest.raises(ValueError):
            dct_sim.tree_sim(NPZ, str(tmp_path / 'out.txt'), **kw)
    assert list(inspect.signature(dct_sim.Tree.__init__).parameters) == ['self', 'sid', 'idx', 'fps', 'score', 'min_cut']


# ---- without a device

def test_trees_of_nothing_need_no_device():
    from dctdomain_amd import dct_sim
    rows = np.zeros((2, 480), dtype=np.int8)
    for sid, idx, fps, kw in (([], [0], rows[:0], {}), (['a'], [0, 1], rows[:1], {}), (['a', 'b'], [0, 1, 2], rows, {'min_cut': 1.5}),
                              (['a', 'b'], [0, 1, 2], rows, {'score': 'global', 'min_cut': 1.5})):
        tree = dct_sim.Tree(sid, np.array(idx), fps, **kw)
        assert all(a.dtype == np.int64 and len(a) == 0 for a in tree.edges()) and tree.rounds == 0
        got = []
        tree.write(got.append)
        assert got == []
        assert tree.labels(2.0).tolist() == list(range(len(sid)))
    assert dct_sim.Tree(['a', 'b'], np.array([0, 1, 2]), rows).bound == 16999 == trule.DEFAULT_BOUND
    assert dct_sim.Tree(['a', 'b'], np.array([0, 1, 2]), rows, min_cut=0.5).bound == dct_sim.sim_bound(0.5) == 8500
    tree = dct_sim.Tree(['a', 'b'], np.array([0, 1, 2]), rows, 'global', 0.5)
    assert (tree.route, tree.bound, tree.bound_domain) == ('global', 8500, 17000)
    with pytest.raises(ValueError):
        dct_sim.Tree(['a'], np.array([0, 1]), rows[:1], score='protein')
    with pytest.raises(ValueError):
        dct_sim.Tree(['a', 'b'], np.array([0, 1, 2]), rows, min_cut=1.5).labels(0.5)       # (a cut-off the tree does not reach)


# ---- the library

PARAMS = {
    'dctfp_tri_nearest': 'dctfp_ctx* ctx, const int32_t* tile, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row0, int64_t col0, '
                         'const uint8_t* row_empty, const uint8_t* col_empty, int32_t cap, int32_t bound, const int32_t* comp, uint64_t* best, '
                         'int64_t n_nodes, void* stream',
    'dctfp_tree_hook': 'dctfp_ctx* ctx, const int32_t* comp, uint64_t* best, int32_t* parent, int64_t n_nodes, int32_t* edge_i, int32_t* edge_j, '
                       'int32_t* edge_key, int32_t* counter, int64_t max_edges, void* stream',
}


@pytest.mark.parametrize('name', sorted(PARAMS))
def test_library_exports_the_entry_points_and_header_documents_them(name):
    from dctdomain_amd import _lib
    with open(os.path.join(ROOT, 'include', 'dctfp.h')) as fh:
        header = fh.read()
    decl = re.search(r'int %s\(([^;]*)\);' % name, header)
    assert decl and ' '.join(decl.group(1).split()) == PARAMS[name]
    doc = header[:decl.start()].rsplit('/*', 1)[1]
    flat = ' '.join(doc.replace(' * ', ' ').split())
    assert '*/' in doc and 'DCTFP_ERR_LIMIT' in doc and 'DCTFP_ERR_INVALID' in doc and 'dctfp_tri_filter_count' in doc and 'survival rule' in flat
    assert re.fullmatch(r'\s*', doc.split('*/', 1)[1]), 'the comment must sit right above the declaration'
    version = int(re.search(r'#define DCTFP_VERSION (\d+)', header).group(1))
    assert version >= 109                                       # (the parent commit's: 108)
    for path in (_lib.LIB_PATH, _lib.EXPERIMENTS_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert hasattr(lib, name) and lib.dctfp_version() == version
    assert name in _lib.EXPORTS
    fn = getattr(_lib._configure(ctypes.CDLL(_lib.LIB_PATH)), name)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(PARAMS[name].split(','))
    launch = open(os.path.join(ROOT, 'dctdomain_amd', 'csrc', 'launch.h')).read()
    assert 'launch_' + name[len('dctfp_'):] + '(' in launch
    assert name in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


def test_new_unit_is_part_of_the_build_and_touches_best_through_atomics_only_while_tiles_run():
    import build_ext
    assert 'k_tree.hip' in build_ext.UNITS and 'k_cluster.hip' in build_ext.UNITS
    text = open(os.path.join(ROOT, 'dctdomain_amd', 'csrc', 'k_tree.hip')).read()
    code = '\n'.join(line.split('//', 1)[0] for line in text.splitlines())
    assert '#include "union_find.hip.h"' in text and 'filter_quad(' in code and 'uf_union(parent' in code
    csrc = os.path.join(ROOT, 'dctdomain_amd', 'csrc')
    for unit in build_ext.UNITS:                              # (no translation unit is included into another)
        assert not re.search(r'#include\s+"[^"]*\.hip"', open(os.path.join(csrc, unit)).read()), unit
    nearest = code[code.index('void tri_nearest_kernel'):code.index('void tree_hook_kernel')]
    lower = code[code.index('void lower_best'):code.index('void tri_nearest_kernel')]
    assert not re.search(r'\bbest\s*\[', nearest + lower) and 'lower_best(best' in nearest     # (no plain load or store of best)
    uses = re.findall(r'[^\n]*\bbest \+ c\b[^\n]*', lower)
    assert len(uses) == 2 and all('__hip_atomic_' in u and '__ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT' in u for u in uses)
    assert '__hip_atomic_fetch_min(best + c' in lower
    assert not re.search(r'\bwhile\b|\bfor \(;;\)', nearest) and 'asm' not in code              # (no spin loop in the scan)


def test_the_node_limit_is_said_before_anything_else_is_looked_at():
    """2^24 nodes: 24 bits for each end of a packed edge.  The check needs no context, so it is made first and can be seen
    without a device; below the limit such a call ends at the NULL check."""
    from dctdomain_amd import _lib
    lib = _lib._configure(ctypes.CDLL(_lib.LIB_PATH))
    nearest = lambda n_nodes, cap=17000: lib.dctfp_tri_nearest(None, None, 1, 1, 1, 0, 0, None, None, cap, 0, None, None, n_nodes, None)   # noqa: E731
    hook = lambda n_nodes: lib.dctfp_tree_hook(None, None, None, None, n_nodes, None, None, None, None, 0, None)                            # noqa: E731
    assert nearest(2 ** 24 + 1) == _lib.DCTFP_ERR_LIMIT and b'2^24' in lib.dctfp_last_error()
    assert hook(2 ** 24 + 1) == _lib.DCTFP_ERR_LIMIT and b'2^24' in lib.dctfp_last_error()
    assert nearest(2 ** 24, cap=32768) == _lib.DCTFP_ERR_LIMIT
    assert nearest(2 ** 24) == _lib.DCTFP_ERR_INVALID and b'dctfp_tri_nearest: NULL argument' in lib.dctfp_last_error()
    assert hook(2 ** 24) == _lib.DCTFP_ERR_INVALID and b'dctfp_tree_hook: NULL argument' in lib.dctfp_last_error()


def test_the_wrappers_are_public_and_carry_the_stated_signatures():
    from dctdomain_amd import dct_sim, similarity
    assert list(inspect.signature(similarity.tri_nearest).parameters) == ['tile', 'row0', 'col0', 'bound', 'ts', 'row_empty', 'col_empty', 'cap']
    assert inspect.signature(similarity.tri_nearest).parameters['cap'].default == 17000
    assert list(inspect.signature(similarity.tree_hook).parameters) == ['ts']
    assert similarity.TREE_MAX_NODES == 2 ** 24 and dct_sim.SCORES == ('domain', 'global')
    assert '--tree' in dct_sim.__doc__ and 'dctfp_tri_nearest' in dct_sim.__doc__ and 'dctfp_tree_hook' in dct_sim.__doc__
    for name in ('README.md', 'DESIGN.md'):
        assert '--tree' in open(os.path.join(ROOT, name)).read()
