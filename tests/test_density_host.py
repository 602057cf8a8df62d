"""dct-sim --cluster --min-neighbors without a GPU: the numpy rule (density_rule.py) pinned by hand on the committed reference
fixture and checked against a textbook sequential DBSCAN, the command-line rules, and the new exports' place in the build."""

import contextlib
import io
import os
import re

import numpy as np
import pytest

import all_sim_filter_rule as rule
import cluster_rule
import density_rule as dr
import golden_util as gu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G6PD = os.path.join(gu.GOLD, 'ref_fixtures', 'G6PD-dct.npz')


@pytest.fixture(scope='module')
def g6pd():
    with np.load(G6PD) as data:
        sid, idx, dct = [str(s) for s in data['sid']], data['idx'], data['dct']
    return sid, idx, dct, rule.triangle_l1(dct, idx)


# ---- 1. the rule

def test_the_rule_by_hand():
    # 0-1-2-3 a clique; 4 hangs on 3 and on 6; 5-6-7-8 a clique; 9 hangs on 8 alone; 10 on nothing; 11 - 12 a pair
    edges = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3), (3, 4), (4, 6), (5, 6), (5, 7), (5, 8), (6, 7), (6, 8), (7, 8), (8, 9), (11, 12)]
    i, j = (np.array(v) for v in zip(*edges))
    single = cluster_rule.components(13, i, j)
    assert single.tolist() == [0] * 10 + [10, 11, 11]                        # the bridge 3 - 4 - 6 chains the two cliques
    label, kind, deg = dr.clusters(13, i, j, 3)
    assert deg.tolist() == [3, 3, 3, 4, 2, 3, 4, 3, 4, 1, 0, 1, 1]
    assert kind.tolist() == [2, 2, 2, 2, 1, 2, 2, 2, 2, 1, 0, 0, 0]          # 4 and 9 borders; 10, 11 and 12 noise (11 - 12: no core end)
    assert label.tolist() == [0, 0, 0, 0, 0, 5, 5, 5, 5, 5, 10, 11, 12]      # 4 goes to its LOWEST core neighbour, 3; no chain
    assert np.array_equal(dr.clusters(13, i, j, 1)[0], single)
    # a border below every core of its cluster names it: the label is the smallest MEMBER
    label, kind, _ = dr.clusters(5, np.array([0, 1, 1, 2]), np.array([2, 2, 3, 3]), 2)
    assert kind.tolist() == [1, 2, 2, 2, 0] and label.tolist() == [0, 0, 0, 0, 4]
    assert dr.clusters(13, i, j, 5)[1].tolist() == [0] * 13 and dr.clusters(13, i, j, 5)[0].tolist() == list(range(13))


PINNED = [({'min_global': 0.6}, 6, (15, 5, 7)), ({'min_global': 0.6}, 8, (4, 9, 14)), ({'min_global': 0.6}, 12, (0, 0, 27)),
          ({'min_global': 0.5}, 8, (12, 1, 14))]


def test_the_rule_on_the_reference_fixture(g6pd):
    sid, idx, dct, tri = g6pd
    assert len(sid) == 27
    single, _ = cluster_rule.labels(dct, idx, min_global=0.6)
    assert sorted(np.bincount(single)[np.unique(single)].tolist()) == [1, 6, 7, 13]
    for kw, m, want in PINNED:
        label, kind, _ = dr.of_file(dct, idx, m, triangle=tri, **kw)
        assert dr.counts(kind) == want, (kw, m)
        if want[0] == 0:
            assert label.tolist() == list(range(27))
    label, kind, deg = dr.of_file(dct, idx, 6, triangle=tri, min_global=0.6)
    sizes = np.bincount(label)[np.unique(label)]
    assert len(sizes) == 9 and sorted(sizes.tolist())[-2:] == [7, 13] and int((sizes == 1).sum()) == 7
    assert int(deg.max()) == 10 and (label <= np.arange(27)).all() and (label[label] == label).all()
    # --min-domain 0.5: every pair passes, every degree is 26 -- one cluster of 27 for any M up to 26 (so for any M <= 12)
    for m in (1, 6, 12, 26):
        label, kind, deg = dr.of_file(dct, idx, m, triangle=tri, min_domain=0.5)
        assert not label.any() and (kind == dr.CORE).all() and (deg == 26).all()
    assert dr.of_file(dct, idx, 27, triangle=tri, min_domain=0.5)[0].tolist() == list(range(27))


CUTS = [{'min_domain': 0.5}, {'min_global': 0.5}, {'min_global': 0.6}, {'min_domain': 0.7}, {'min_domain': 0.5, 'min_global': 0.6},
        {'min_domain': 0.0}, {'min_global': 1.5}]


@pytest.mark.parametrize('kw', CUTS, ids=lambda kw: '-'.join(f'{k[4:]}{v}' for k, v in kw.items()))
def test_one_neighbour_is_single_linkage(g6pd, kw):
    _, idx, dct, tri = g6pd
    label, kind, deg = dr.of_file(dct, idx, 1, triangle=tri, **kw)
    assert np.array_equal(label, cluster_rule.labels(dct, idx, **kw)[0])
    assert not (kind == dr.BORDER).any() and np.array_equal(kind == dr.NOISE, deg == 0)


def _textbook_dbscan(n, neighbours, m):
    """Ester et al.'s sequential DBSCAN in index order (the protein itself not counted): label per node, -1 = noise."""
    unseen, noise = -2, -1
    label = [unseen] * n
    c = 0
    for p in range(n):
        if label[p] != unseen:
            continue
        if len(neighbours[p]) < m:
            label[p] = noise
            continue
        label[p] = c
        seeds = list(neighbours[p])
        while seeds:
            q = seeds.pop()
            if label[q] == noise:
                label[q] = c                                                 # a border: the first cluster that reaches it keeps it
            if label[q] != unseen:
                continue
            label[q] = c
            if len(neighbours[q]) >= m:
                seeds.extend(neighbours[q])
        c += 1
    return np.array(label)


@pytest.mark.parametrize('m', [2, 4, 6, 8])
@pytest.mark.parametrize('kw', CUTS[:5], ids=lambda kw: '-'.join(f'{k[4:]}{v}' for k, v in kw.items()))
def test_against_a_textbook_dbscan(g6pd, kw, m):
    _, idx, dct, (i, j, mn, last) = g6pd
    n = len(idx) - 1
    keep = rule.kept(mn, last, **kw)
    neighbours = [[] for _ in range(n)]
    for a, b in zip(i[keep].tolist(), j[keep].tolist()):
        neighbours[a].append(b)
        neighbours[b].append(a)
    book = _textbook_dbscan(n, neighbours, m)
    label, kind, deg = dr.clusters(n, i[keep], j[keep], m)
    core = np.array([len(v) >= m for v in neighbours])
    assert np.array_equal(kind == dr.CORE, core) and np.array_equal(deg, [len(v) for v in neighbours])
    # the same partition of the cores
    pairs = {(int(a), int(b)) for a, b in zip(book[core], label[core])}
    assert len(pairs) == len({a for a, _ in pairs}) == len({b for _, b in pairs})
    # the same borders and the same noise; a border sits with its lowest core neighbour here, with some core neighbour there
    assert np.array_equal(kind == dr.NOISE, book == -1)
    for x in np.flatnonzero(kind == dr.BORDER):
        cores = [y for y in neighbours[x] if core[y]]
        assert cores and label[x] == label[min(cores)] and book[x] in {book[y] for y in cores}


# ---- 2. the command line

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


CLUSTER = ['--cluster', '--min-domain', '0.5']


@pytest.mark.parametrize('argv, message', [
    (['--min-domain', '0.5', '--min-neighbors', '3'], '--min-neighbors says how many neighbours'),
    (['--min-neighbors', '3'], '--min-neighbors says how many neighbours'),
    (CLUSTER + ['--min-neighbors', '0'], '--min-neighbors is a number of neighbours: at least 1'),
    (CLUSTER + ['--min-neighbors', '-2'], '--min-neighbors is a number of neighbours: at least 1'),
    (CLUSTER + ['--linkage', 'greedy', '--min-neighbors', '3'], '--min-neighbors thins the graph of single linkage: not with --linkage greedy'),
    (CLUSTER + ['--level', 'domain', '--min-neighbors', '3'], '--min-neighbors counts the neighbours of a protein: not with --level domain'),
])
def test_the_parser_refuses(argv, message):
    got = _parse(argv)
    assert isinstance(got, str) and got.startswith(message), got


@pytest.mark.parametrize('argv, mode', [(['--tree'], '--tree'), (['--db', 'y', '--rbh'], '--rbh'), (['--assign', 'r', '--min-domain', '0.5'], '--assign')])
def test_the_three_modes_refuse_it(argv, mode):
    got = _parse(argv + ['--min-neighbors', '3'])
    assert isinstance(got, str) and got.startswith(mode + ' ') and got.endswith(': not with --min-neighbors'), got


def test_the_parser_accepts():
    plain = _parse(CLUSTER)
    assert 'min_neighbors' not in plain
    assert _parse(CLUSTER + ['--min-neighbors', '3']) == dict(plain, min_neighbors=3)
    assert _parse(CLUSTER + ['--min-neighbors', '1', '--rep', 'medoid', '--reps-out', 'f', '--linkage', 'single', '--level', 'protein']) == \
        dict(plain, min_neighbors=1, rep='medoid', reps_out='f', linkage='single', level='protein')
    assert _parse(['--cluster', '--min-global', '0.6', '--min-domain', '0.5', '--min-coverage', '0.8', '--min-neighbors', '6']) == \
        dict(plain, min_global=0.6, min_coverage=0.8, min_neighbors=6)
    # --reps-out keeps its conditions: density clusters alone do not allow it
    got = _parse(CLUSTER + ['--min-neighbors', '3', '--reps-out', 'f'])
    assert isinstance(got, str) and got.startswith('--reps-out writes representatives')
    assert isinstance(_parse(CLUSTER + ['--min-neighbors', 'many']), str)


def test_cluster_sim_refuses_what_the_parser_refuses(tmp_path):
    from dctdomain_amd import dct_sim
    out = str(tmp_path / 'out.txt')
    assert dct_sim.LINKAGES == ('single', 'greedy') and dct_sim.REPS == ('first', 'medoid') and dct_sim.LEVELS == ('protein', 'domain')
    for kw in ({'min_neighbors': 0}, {'min_neighbors': 3, 'linkage': 'greedy'}, {'min_neighbors': 3, 'level': 'domain'},
               {'min_neighbors': 2.5}):
        with pytest.raises(ValueError):
            dct_sim.cluster_sim(G6PD, out, min_domain=0.5, **kw)
    with pytest.raises(ValueError):
        dct_sim.DensityClusters(['a'], [0, 0], np.zeros((0, 8), dtype=np.int8), min_domain=0.5, min_neighbors=0)


def test_what_needs_no_tile_needs_no_device(tmp_path, g6pd):
    """Fewer than two proteins or a bound below 0: every protein noise.  No bound excludes anything: the complete graph -- one
    cluster of cores if n - 1 >= M, else every protein its own."""
    from dctdomain_amd import dct_sim
    sid, idx, dct, _ = g6pd
    job = dct_sim.DensityClusters(sid, idx, dct, min_domain=1.5, min_neighbors=2)
    assert job.labels().tolist() == list(range(27)) and job.labels().dtype == np.int32
    assert job.kinds().tolist() == [0] * 27 and job.kinds().dtype == np.uint8 and not job.degrees().any() and job.degrees().dtype == np.int32
    assert job.medoids().tolist() == list(range(27))
    job = dct_sim.DensityClusters(sid, idx, dct, min_domain=0.0, min_neighbors=26)
    assert job.kinds().tolist() == [2] * 27 and job.degrees().tolist() == [26] * 27 and not job.labels().any()
    job = dct_sim.DensityClusters(sid, idx, dct, min_domain=0.0, min_neighbors=27)
    assert job.labels().tolist() == list(range(27)) and job.kinds().tolist() == [0] * 27 and job.degrees().tolist() == [26] * 27
    one = dct_sim.DensityClusters(sid[:1], idx[:2], dct, min_domain=0.5, min_neighbors=1)
    assert one.labels().tolist() == [0] and one.kinds().tolist() == [0] and one.degrees().tolist() == [0]
    none = dct_sim.DensityClusters([], idx[:1], dct, min_domain=0.5, min_neighbors=1)
    assert none.labels().tolist() == [] and none.kinds().tolist() == []
    out = str(tmp_path / 'out.txt')
    dct_sim.main(['--dct', G6PD, '--cluster', '--min-domain', '1.5', '--min-neighbors', '2', '--output', out])
    with open(out, 'rb') as fh:
        assert fh.read() == cluster_rule.HEADER + cluster_rule.text(sid, np.arange(27))


# ---- 3. the build

def _code(path):
    with open(path) as fh:
        return '\n'.join(line.split('//', 1)[0] for line in fh.read().splitlines())


def test_the_exports_are_declared_bound_and_built():
    import ctypes

    import build_ext
    from dctdomain_amd import _lib, similarity
    with open(os.path.join(ROOT, 'include', 'dctfp.h')) as fh:
        header = fh.read()
    assert int(re.search(r'#define DCTFP_VERSION (\d+)', header).group(1)) >= 113
    sizes = {'dctfp_tri_degree': 14, 'dctfp_tri_link_core': 16}      # ctx, the ten tile values, the arrays, n_nodes, stream
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
    assert ctypes.CDLL(_lib.LIB_PATH).dctfp_version() >= 113
    assert callable(similarity.tri_degree) and callable(similarity.tri_link_core)
    assert 'k_density.hip' in build_ext.UNITS


def test_the_unit_touches_its_arrays_through_agent_scope_atomics_alone():
    unit = _code(os.path.join(ROOT, 'dctdomain_amd', 'csrc', 'k_density.hip'))
    assert '__hip_atomic_fetch_add(' in unit and '__hip_atomic_fetch_min(' in unit and '__HIP_MEMORY_SCOPE_AGENT' in unit
    assert '#include "union_find.hip.h"' in unit and '#include "band_walk.hip.h"' in unit and 'uf_union(parent, ' in unit and 'asm' not in unit
    assert unit.count('__ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT') == 2          # add_degree and lower_nearest; the forest has its own
    degree = unit[unit.index('struct DegreePass'):unit.index('struct LinkCorePass')]
    link = unit[unit.index('struct LinkCorePass'):unit.index('__global__')]
    kernels = unit[unit.index('__global__'):unit.index('namespace dctfp_host')]
    # two passes of the one band walk over a triangle with a bound
    assert 'void tri_degree_kernel(const TriTile t, ' in kernels and 'band_walk(t, n_bands, n_steps, DegreePass{deg});' in kernels
    assert 'void tri_link_core_kernel(const TriTile t, ' in kernels and 'band_walk(t, n_bands, n_steps, LinkCorePass{core, parent, nearest});' in kernels
    for body in (degree, link):
        assert 'kBounded = true' in body
    # no plain load or store of deg, nearest or parent -- only ever offset and handed to the helpers, in the two flushes -- and no loop at all
    assert not re.search(r'\b(deg|nearest|parent)\s*\[', unit)
    assert len(re.findall(r'add_degree\(deg \+ ', degree)) == 2 and len(re.findall(r'lower_nearest\(nearest \+ ', link)) == 2
    for body, helper in ((degree, r'add_degree\(deg \+ '), (link, r'lower_nearest\(nearest \+ ')):
        assert re.search(r'void row_out\([^)]*\) const \{ ' + helper, body) and re.search(r'void col_out\([^)]*\) const \{ ' + helper, body)
    assert not re.search(r'\bwhile\b|\bfor\b', degree + link + kernels)
    # core: read in _is_core alone, which the pass's side() calls -- the walk takes a side value once per column and job and once per
    # row and band (test_cluster_host.py checks the walk) -- and wants() sees the two flags before the entry is loaded
    assert '_is_core(const uint8_t* __restrict__ core, int64_t x)' in unit
    assert len(re.findall(r'_is_core\(', link)) == 1 and 'Side side(int64_t x) const { return _is_core(core, x); }' in link
    assert 'bool wants(Side row_core, Side col_core) { return row_core || col_core; }' in link
    assert len(re.findall(r'\bcore\s*\[', unit)) == 1 and not re.search(r'\bcore\s*\[', degree + link + kernels)
