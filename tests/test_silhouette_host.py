"""python -m dctdomain_amd.cluster_quality without a GPU: the rule (tests/silhouette_rule.py) against scikit-learn, the G6PD example
of the README, `Silhouette`'s host arithmetic and text from given integer sums, the --clusters reader, the command's parser, and the
header, the binding, the build list and the source of the kernel."""

import ctypes
import io
import os
import re

import numpy as np
import pytest

import cluster_rule
import make_golden_silhouette as golden
import silhouette_rule as rule
from dctdomain_amd import _lib, cluster_quality, dct_sim
from dctdomain_amd.cluster_quality import Silhouette

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, 'tests', 'golden', 'ref_fixtures')
NAN = float('nan')


def _fixture(name):
    with np.load(os.path.join(FIX, name)) as data:
        return data['sid'], np.asarray(data['idx'], dtype=np.int64), data['dct']


def _random_case(rng):
    """(key matrix, labels) of n <= 40 proteins: keys from few values so that ties are common, singletons, and proteins without
    fingerprints (their rows and columns at the cap)."""
    n = int(rng.integers(2, 41))
    kind = int(rng.integers(0, 3))
    pool = [np.array([0, 1, 16999, 17000]), np.arange(0, 4), np.arange(16990, 17001)][kind]
    key = rng.choice(pool, size=(n, n))
    key = np.triu(key, 1)
    key = key + key.T
    empty = rng.random(n) < 0.1
    key[empty, :] = rule.CAP
    key[:, empty] = rule.CAP
    np.fill_diagonal(key, 0)
    n_clusters = int(rng.integers(2, max(3, n // 2 + 1)))
    labels = rng.integers(0, n_clusters, size=n)
    labels[:2] = [0, 1]                                             # (two clusters at least)
    lone = rng.random(n) < 0.15                                     # singletons: labels of their own
    labels = [int(1000 + i) if lone[i] else int(labels[i]) for i in range(n)]
    return key.astype(np.int64), labels


def _sklearn_cases():
    for name in ('G6PD-dct.npz', 'example-dct.npz'):
        sid, idx, dct = _fixture(name)
        n = len(sid)
        label = cluster_rule.labels(dct, idx, min_global=0.6)[0] if name.startswith('G6PD') else np.arange(n) % 3
        for score in ('domain', 'global'):
            yield rule.key_matrix(dct, idx, score), [int(x) for x in label]
    rng = np.random.default_rng(20261021)
    for _ in range(200):
        yield _random_case(rng)


def test_the_rule_is_scikit_learns_silhouette_on_the_precomputed_keys():
    metrics = pytest.importorskip('sklearn.metrics')
    worst, cases, tied = 0.0, 0, 0
    for key, labels in _sklearn_cases():
        if not 2 <= len(set(labels)) <= len(labels) - 1:            # (scikit-learn refuses the rest)
            continue
        four = rule.sums(key, labels)
        want = metrics.silhouette_samples(key.astype(np.float64), np.array([hash(x) for x in labels]), metric='precomputed')
        got = rule.values(four, labels)
        worst = max(worst, float(np.abs(got - want).max()))
        cases += 1
        tied += int((got == 0).any())
    assert cases >= 150 and tied >= 10
    assert worst <= 1e-12, worst


def test_g6pd_at_min_global_06_is_the_readmes_example():
    sid, idx, dct, labels = golden.g6pd()
    assert sorted(np.unique(labels, return_counts=True)[1].tolist()) == [1, 6, 7, 13]
    for score, last in (('global', b'mean_silhouette=0.5373 negative=0\n'), ('domain', b'mean_silhouette=0.2500 negative=8\n')):
        four = rule.sums(rule.key_matrix(dct, idx, score), labels)
        text = rule.PROTEIN_HEADER + rule.text(sid, labels, four)
        with open(os.path.join(golden.OUT, f'G6PD_{score}.txt'), 'rb') as fh:
            assert fh.read() == text
        assert text.endswith(b'# proteins=27 clusters=4 singletons=1 ' + last)
        values = rule.values(four, labels)
        assert values[labels.index('L9L140')] == 0 and labels.count('L9L140') == 1          # the singleton
        # the product's host side on the same integers: the same bytes, both forms
        job = Silhouette(sid, idx, dct, labels, score=score).with_sums(*four)
        for per in cluster_quality.PER:
            out = []
            job.write(out.append, per=per)
            assert b''.join(out) == rule.text(sid, labels, four, per)
        assert np.array_equal(job.values(), values)
        with open(os.path.join(ROOT, 'README.md')) as fh:
            assert last.decode().strip() in fh.read()


def _job(labels, own, near_sum, near_size, near_first):
    sid = [f'p{i}' for i in range(len(labels))]
    return Silhouette(sid, None, None, labels).with_sums(own, near_sum, near_size, near_first)


def test_values_summary_and_text_from_hand_made_sums():
    # clusters a = {0, 1, 2}, b = {3, 4}, c = {5}; p0: Sa 200 over 2, Sb 900 over 2 -> (900 - 200) / 900
    labels = ['a', 'a', 'a', 'b', 'b', 'c']
    job = _job(labels, [200, 0, 17000 * 2, 100, 100, 0], [900, 0, 17000, 300, 150, 17000 * 3], [2, 2, 1, 3, 3, 3], [3, 3, 5, 0, 0, 0])
    v = job.values()
    assert v[0] == (900 * 2 - 200 * 2) / (900 * 2)
    assert v[1] == 0.0                                              # both sums 0: the maximum is 0
    assert v[2] == (17000 * 2 - 34000 * 1) / max(34000 * 1, 17000 * 2) == 0.0
    assert v[3] == (300 * 1 - 100 * 3) / 300 == 0.0
    assert v[4] == (150 * 1 - 100 * 3) / (100 * 3) == -0.5
    assert v[5] == 0.0                                              # a singleton, whatever its neighbour
    assert job.neighbours().tolist() == [3, 3, 5, 0, 0, 0]
    s = job.summary()
    assert (s['proteins'], s['clusters'], s['singletons'], s['negative']) == (6, 3, 1, 1)
    assert s['mean'] == pytest.approx((v[0] - 0.5) / 6, abs=1e-15)
    assert [d[:2] for d in s['clusters_detail']] == [(0, 3), (3, 2), (5, 1)]
    assert s['clusters_detail'][1][2:] == (-0.25, -0.5, 1) and s['clusters_detail'][2][2:] == (0.0, 0.0, 0)
    assert list(job.lines()) == ['p0 a 3 0.9941 0.9735 b 0.7778', 'p1 a 3 1.0000 1.0000 b 0.0000', 'p2 a 3 0.0000 0.0000 c 0.0000',
                                 'p3 b 2 0.9941 0.9941 a 0.0000', 'p4 b 2 0.9941 0.9971 a -0.5000', 'p5 c 1 - 0.0000 a 0.0000',
                                 '# proteins=6 clusters=3 singletons=1 mean_silhouette=0.0463 negative=1']
    assert list(job.lines('cluster')) == ['a 3 0.2593 0.0000 0', 'b 2 -0.2500 -0.5000 1', 'c 1 0.0000 0.0000 0',
                                          '# proteins=6 clusters=3 singletons=1 mean_silhouette=0.0463 negative=1']
    out = []
    job.write(out.append, chunk_lines=2)                           # whole lines, in order, however they are chunked
    assert b''.join(out).decode().splitlines() == list(job.lines()) and all(part.endswith(b'\n') for part in out)
    with pytest.raises(ValueError):
        list(job.lines('family'))
    with pytest.raises(ValueError):
        job.with_sums([0], [0], [0], [0])
    with pytest.raises(ValueError):
        Silhouette(['x', 'y'], None, None, ['a'])
    with pytest.raises(ValueError):
        Silhouette(['x'], None, None, ['a'], score='local')


def test_fewer_than_two_clusters_is_undefined_everywhere():
    job = _job(['a', 'a', 'a'], [10, 20, 30], [0, 0, 0], [0, 0, 0], [-1, -1, -1])
    assert np.isnan(job.values()).all() and not job.defined()
    s = job.summary()
    assert s['mean'] is None and s['negative'] == 0 and s['clusters'] == 1 and s['clusters_detail'] == [(0, 3, None, None, 0)]
    assert list(job.lines()) == ['p0 a 3 0.9997 - - -', 'p1 a 3 0.9994 - - -', 'p2 a 3 0.9991 - - -',
                                 '# proteins=3 clusters=1 singletons=0 mean_silhouette=- negative=0']
    assert list(job.lines('cluster')) == ['a 3 - - 0', '# proteins=3 clusters=1 singletons=0 mean_silhouette=- negative=0']
    one = _job(['z'], [0], [0], [0], [-1])
    assert list(one.lines()) == ['p0 z 1 - - - -', '# proteins=1 clusters=1 singletons=1 mean_silhouette=- negative=0']
    none = Silhouette([], np.zeros(1, dtype=np.int64), np.zeros((0, 4), dtype=np.int8), [])
    assert [a.shape for a in none.sums()] == [(0,)] * 4 and list(none.lines()) == ['# proteins=0 clusters=0 singletons=0 mean_silhouette=- negative=0']


def test_a_tie_in_the_neighbour_goes_to_the_first_member_that_comes_first():
    # row 0 of cluster {0, 1}: clusters {2, 3} with 6 / 2, {4, 5, 6} with 9 / 3 and the singleton 7 with 3 / 1 tie at 3
    key = np.zeros((8, 8), dtype=np.int64)
    key[0] = [0, 5, 2, 4, 3, 3, 3, 3]
    for labels, want in ((['a', 'a', 'b', 'b', 'c', 'c', 'c', 'd'], (6, 2, 2)), (['a', 'a', 'c', 'c', 'b', 'b', 'b', 'd'], (6, 2, 2))):
        got = rule.tile_sums(key[:1], 0, 0, *rule.kernel_arrays(labels))[0]
        assert got == (5,) + want
    # ... and with the singleton first in the file it is the neighbour
    key[0] = [0, 3, 5, 2, 4, 3, 3, 3]
    got = rule.tile_sums(key[:1], 0, 0, *rule.kernel_arrays(['a', 'd', 'a', 'b', 'b', 'c', 'c', 'c']))[0]
    assert got == (5, 3, 1, 1)
    # dense ids are by first member whatever the labels are, and singletons carry -1
    cid, size, first = rule.kernel_arrays(['x', 9, 'x', 'y', 9, 'z'])
    assert cid.tolist() == [0, 1, 0, -1, 1, -1] and size.tolist() == [2, 2] and first.tolist() == [0, 1]
    job = Silhouette(list('abcdef'), None, None, ['x', 9, 'x', 'y', 9, 'z'])
    assert [a.tolist() for a in job.device_clusters()] == [[0, 1, 0, -1, 1, -1], [2, 2], [0, 1]]
    assert all(a.dtype == np.int32 for a in job.device_clusters())
    assert job.cluster.tolist() == [0, 1, 0, 2, 1, 3] and job.first.tolist() == [0, 1, 3, 5] and job.size.tolist() == [2, 2, 1, 1]


def test_the_clusters_reader(tmp_path):
    sid = np.array(['p1', 'p2', 'p3', 'p4'])
    path = tmp_path / 'c.txt'

    def read(text):
        path.write_text(text)
        return cluster_quality.read_clusters(str(path), sid)
    assert read('#representative member\n\np1 p1\np1 p3\n  \nrep9 p2\np1\tp4\nrep9 unknown\np1 p3\n') == ['p1', 'rep9', 'p1', 'p1']
    with pytest.raises(ValueError, match=r'line 2: four fields, a line of dct-sim --cluster --level domain'):
        read('#representative member dom1 dom2\np1 p2 1-50 3-40\n')
    with pytest.raises(ValueError, match=r'line 1: a line is "representative member", two fields'):
        read('p1 p2 p3\n')
    with pytest.raises(ValueError, match=r'line 3: p2 is given two representatives, p1 and p4'):
        read('p1 p1\np1 p2\np4 p2\n')
    with pytest.raises(ValueError, match=r'has no line for p3'):
        read('p1 p1\np1 p2\np4 p4\n')
    # the text of dct-sim --cluster read back: the labels it came from, by representative or by medoid
    label = np.array([0, 0, 2, 0])
    for rep, want in ((None, ['p1', 'p1', 'p3', 'p1']), (np.array([1, 1, 2, 1]), ['p2', 'p2', 'p3', 'p2'])):
        path.write_bytes((dct_sim.CLUSTER_HEADER + '\n').encode() + b''.join(bytes(part) for part in dct_sim.cluster_lines(sid, label, rep=rep)))
        got = cluster_quality.read_clusters(str(path), sid)
        assert got == want and rule.dense(got)[0].tolist() == rule.dense(label.tolist())[0].tolist()


def test_the_parser_takes_exactly_one_source_of_labels(capsys):
    parser = cluster_quality.build_parser()
    args = parser.parse_args(['--dct', 'x.npz', '--clusters', 'c.txt'])
    assert (args.dct, args.clusters, args.families, args.family_sep, args.score, args.per, args.out) == ('x.npz', 'c.txt', None, None, 'domain', 'protein', None)
    args = parser.parse_args(['--dct', 'x.npz', '--family-sep', '|', '--score', 'global', '--per', 'cluster', '--out', 'o.txt'])
    assert (args.family_sep, args.score, args.per, args.out) == ('|', 'global', 'cluster', 'o.txt')
    assert parser.parse_args(['--dct', 'x.npz', '--families', 'f.txt']).families == 'f.txt'
    for bad in (['--dct', 'x.npz'], ['--dct', 'x.npz', '--clusters', 'c', '--families', 'f'], ['--dct', 'x.npz', '--families', 'f', '--family-sep', '|'],
                ['--clusters', 'c'], ['--dct', 'x.npz', '--clusters', 'c', '--score', 'local'], ['--dct', 'x.npz', '--clusters', 'c', '--per', 'family']):
        with pytest.raises(SystemExit) as err:
            parser.parse_args(bad)
        assert err.value.code == 2
    capsys.readouterr()
    with pytest.raises(ValueError, match='one place'):
        cluster_quality.cluster_quality('x.npz', None, clusters='c', families='f')
    with pytest.raises(ValueError, match='one place'):
        cluster_quality.cluster_quality('x.npz', None)
    # dct-sim's own command line is untouched: no option of its parser speaks of the silhouette
    assert 'silhouette' not in dct_sim.build_parser().format_help()


def test_the_text_goes_out_through_report(tmp_path):
    out = tmp_path / 'o.txt'
    report = dct_sim.Report(str(out), cluster_quality.PROTEIN_HEADER)
    _job(['a', 'a', 'b'], [5, 5, 0], [10, 20, 30], [1, 1, 2], [2, 2, 0]).write(report.raw)
    report.close()
    assert out.read_text().splitlines() == ['#protein cluster size own other neighbour silhouette', 'p0 a 2 0.9997 0.9994 b 0.5000',
                                            'p1 a 2 0.9997 0.9988 b 0.7500', 'p2 b 1 - 0.9991 a 0.0000',
                                            '# proteins=3 clusters=2 singletons=1 mean_silhouette=0.4167 negative=0']
    assert (cluster_quality.PROTEIN_HEADER + '\n').encode() == rule.PROTEIN_HEADER and (cluster_quality.CLUSTER_HEADER + '\n').encode() == rule.CLUSTER_HEADER
    sink = io.StringIO()                                            # (a stream without a binary layer takes text)
    report = dct_sim.Report.__new__(dct_sim.Report)
    report.path, report.out = None, sink
    _job(['a'], [0], [0], [0], [-1]).write(report.raw, per='cluster')
    assert sink.getvalue() == 'a 1 - - 0\n# proteins=1 clusters=1 singletons=1 mean_silhouette=- negative=0\n'


def test_header_binding_and_build_list():
    import build_ext
    path = os.path.join(ROOT, 'include', 'dctfp_silhouette.h')
    with open(path) as fh:
        header = fh.read()
    assert sorted(set(re.findall(r'^int (dctfp_\w+)\(', header, re.M))) == sorted(_lib.SILHOUETTE_EXPORTS) == ['dctfp_silhouette_rows', 'dctfp_silhouette_version']
    assert not set(_lib.SILHOUETTE_EXPORTS) & (set(_lib.EXPORTS) | set(_lib.LINKAGE_EXPORTS))
    for other in ('dctfp.h', 'dctfp_linkage.h'):                     # the two other headers gain nothing
        with open(os.path.join(ROOT, 'include', other)) as fh:
            assert 'silhouette' not in fh.read()
    assert (_lib.DCTFP_SILHOUETTE_VERSION, _lib.DCTFP_SILHOUETTE_MAX_CAP, _lib.DCTFP_SILHOUETTE_MAX_PASS_CLUSTERS) == (1, 1 << 22, 4096)
    decl = re.sub(r'\s+', ' ', re.search(r'\nint dctfp_silhouette_rows\(([^;]*)\);', header).group(1))
    assert decl.count(',') == 21 - 1
    assert decl.endswith('const int32_t* cid, const int32_t* size, const int32_t* first, int64_t n_clusters, int32_t pass_clusters, uint64_t* own_sum, '
                         'uint64_t* near_sum, int32_t* near_size, int32_t* near_first, int64_t n_nodes, void* stream')
    for lib_path in (_lib.LIB_PATH, _lib.EXPERIMENTS_LIB_PATH):
        lib = _lib._configure(ctypes.CDLL(lib_path))
        assert all(hasattr(lib, name) for name in _lib.SILHOUETTE_EXPORTS)
        assert lib.dctfp_silhouette_version() == _lib.DCTFP_SILHOUETTE_VERSION
        fn = lib.dctfp_silhouette_rows
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == 21 and fn.argtypes[:10] == _lib._TRI_TILE[:10]
        assert fn.argtypes[10:] == [ctypes.c_void_p] * 3 + [ctypes.c_int64, ctypes.c_int32] + [ctypes.c_void_p] * 4 + [ctypes.c_int64, ctypes.c_void_p]
    assert 'k_silhouette.hip' in build_ext.UNITS and 'k_silhouette.hip' not in build_ext.TWIN_UNITS
    csrc = os.path.join(ROOT, 'dctdomain_amd', 'csrc')
    assert path in build_ext.HEADERS and path not in build_ext.kernel_sources() and os.path.join(csrc, 'k_silhouette.hip') in build_ext.kernel_sources()
    assert build_ext.HEADERS[-1] == os.path.join(csrc, 'union_find.hip.h')
    with open(os.path.join(csrc, 'launch.h')) as fh:
        assert 'void launch_silhouette_rows(const TriTile& t, ' in fh.read()
    with open(os.path.join(ROOT, 'INTEGRATION.md')) as fh:
        assert 'dctfp_silhouette.h' in fh.read()
    # the refusals that need no device, in the library's own codes, the message naming the export
    lib = _lib.load()
    null = [None, None, 1, 1, 1, 0, 0, None, None, 17000, None, None, None, 0, 1, None, None, None, None, 1, None]
    assert lib.dctfp_silhouette_rows(*null) == _lib.DCTFP_ERR_INVALID and b'dctfp_silhouette_rows: NULL argument' in lib.dctfp_last_error()
    for at, value in ((9, (1 << 22) + 1), (14, 4097), (19, 1 << 31)):
        args = list(null)
        args[at] = value
        assert lib.dctfp_silhouette_rows(*args) == _lib.DCTFP_ERR_LIMIT and b'dctfp_silhouette_rows: ' in lib.dctfp_last_error()


def test_an_older_library_is_told_to_rebuild():
    class Old:
        _name = 'libold.so'

        def __getattr__(self, name):
            if name in _lib.SILHOUETTE_EXPORTS:
                raise AttributeError(name)
            return type('F', (), {})()
    with pytest.raises(ImportError, match=r'libold.so lacks dctfp_silhouette_version, dctfp_silhouette_rows \(include/dctfp_silhouette.h\).*rebuild it'):
        _lib._configure(Old())


def _code(path):
    with open(path) as fh:
        return '\n'.join(line.split('//', 1)[0] for line in fh.read().splitlines())


def test_the_unit_keeps_its_sums_in_lds_and_owns_its_row():
    csrc = os.path.join(ROOT, 'dctdomain_amd', 'csrc')
    unit = _code(os.path.join(csrc, 'k_silhouette.hip'))
    # it stands on its own: the tile's description and the launchers' header, neither walk, no inline assembly
    assert re.findall(r'#include "([^"]+)"', unit) == ['launch.h', 'tri_tile.hip.h'] and 'asm' not in unit
    assert not re.search(r'struct \w*Tile\b', unit)
    kernel = unit[unit.index('__global__'):unit.index('namespace dctfp_host')]
    assert '__launch_bounds__(kSilThreads) void silhouette_rows_kernel(const TriTile t, ' in kernel and 'constexpr int kSilThreads = 256;' in unit
    # the sums: 64-bit words in LDS, added to at workgroup scope; no agent-scope atomic anywhere, no global atomic at all
    assert 'extern __shared__ unsigned long long s_sum[];' in kernel
    assert '__HIP_MEMORY_SCOPE_AGENT' not in unit and '__HIP_MEMORY_SCOPE_SYSTEM' not in unit and 'atomicAdd' not in unit
    assert unit.count('__hip_atomic_') == 3 == unit.count('__ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP')
    assert len(re.findall(r'__hip_atomic_fetch_add\(s_sum \+ \w+, \(unsigned long long\)\w+, ', unit)) == 3
    # the four results: named in the head, then written once each, by thread 0, with plain stores
    for array in ('own_sum', 'near_sum', 'near_size', 'near_first'):
        assert len(re.findall(r'\b%s\b' % array, kernel)) == 2 and len(re.findall(r'\b%s\[i\] = ' % array, kernel)) == 1
    assert kernel.index('if (tid == 0) {') < kernel.index('own_sum[i] = ')
    # the exact comparison: both halves of both products; and no workgroup waits for another
    assert unit.count('__umul64hi(') == 2 and not re.search(r'\bwhile\b|for \(;;\)', unit)
    assert 'constexpr int kSilMaxPass = 4096;' in unit and 'constexpr int kSilMaxCap = 1 << 22;' in unit
    # the export checks its tile in its own body
    sim = _code(os.path.join(csrc, 'dctfp_sim.hip'))
    body = sim[sim.index('\nint dctfp_silhouette_rows('):sim.index('DCTFP_GUARD("dctfp_silhouette_rows")')]
    assert 'check_tri_tile(' not in body and 'check_band_tile(' not in body and 'range_within(row0, n_rows, n_nodes)' in body
