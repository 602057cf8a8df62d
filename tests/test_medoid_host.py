"""dct-sim --cluster --rep medoid without a GPU: the numpy rule (medoid_rule.py) worked by hand and pinned on the committed reference
fixture, the text composer against the rule's text, the command-line rules, and the new export's place in the build."""

import contextlib
import io
import os
import re

import numpy as np
import pytest

import all_sim_filter_rule as rule
import cluster_rule
import golden_util as gu
import medoid_rule as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G6PD = os.path.join(gu.GOLD, 'ref_fixtures', 'G6PD-dct.npz')


# ---- 1. the rule

def test_the_rule_by_hand():
    # two clusters {0, 2, 3, 5} and {1, 4}; 5 is at 1 of everything in its cluster, 0 and 2 tie behind it
    key = np.full((6, 6), 9000, dtype=np.int64)
    np.fill_diagonal(key, 0)
    for a, b, v in ((0, 2, 10), (0, 3, 30), (2, 3, 30), (0, 5, 1), (2, 5, 1), (3, 5, 1), (1, 4, 7)):
        key[a, b] = key[b, a] = v
    labels = np.array([0, 1, 0, 0, 1, 0])
    assert mr.sums(key, labels).tolist() == [41, 7, 41, 61, 7, 3]
    assert mr.medoids(key, labels).tolist() == [5, 1, 5, 5, 1, 5]          # (two members: equal sums, the first)
    key[[0, 2, 3], 5] = key[5, [0, 2, 3]] = 17000                            # 5 has no fingerprint: 0 and 2 tie at 17040, to the lower
    assert mr.sums(key, labels).tolist() == [17040, 7, 17040, 17060, 7, 51000]
    assert mr.medoids(key, labels).tolist() == [0, 1, 0, 0, 1, 0]
    assert mr.medoids(key, np.arange(6)).tolist() == list(range(6))          # singletons
    assert mr.text(list('abcdef'), labels, [5, 1, 5, 5, 1, 5]) == b'f a\nf c\nf d\nf f\nb b\nb e\n'


def test_key_matrix_takes_the_route_and_caps():
    dct = np.zeros((4, 8), dtype=np.int8)
    dct[0], dct[1], dct[2], dct[3] = 0, 1, 127, -128                        # proteins: [0, 1], [2], none, [3]
    idx = np.array([0, 2, 3, 3, 4])
    dom, glob = mr.key_matrix(dct, idx, 'domain'), mr.key_matrix(dct, idx, 'global')
    assert dom[0, 1] == 8 * 126 and glob[0, 1] == 8 * 126 and dom[0, 3] == 8 * 128 and glob[0, 3] == 8 * 129
    assert (dom[2, [0, 1, 3]] == 17000).all() and (glob[[0, 1, 3], 2] == 17000).all()      # no fingerprint: 17000 to everyone
    assert dom[1, 3] == 8 * 255 and np.array_equal(dom, dom.T) and not dom.diagonal().any()
    assert mr.route_of(None) == 'domain' and mr.route_of(0.5) == 'global'


@pytest.fixture(scope='module')
def g6pd():
    with np.load(G6PD) as data:
        sid, idx, dct = [str(s) for s in data['sid']], data['idx'], data['dct']
    return sid, idx, dct, rule.triangle_l1(dct, idx)


def test_the_rule_on_the_reference_fixture(g6pd):
    sid, idx, dct, tri = g6pd
    n = len(sid)
    assert n == 27
    # --min-domain 0.5: one cluster, named after protein 0 today; protein 11 is closest to all the others, and alone in that
    labels, _ = cluster_rule.labels(dct, idx, min_domain=0.5)
    key = mr.key_matrix(dct, idx, 'domain', tri)
    assert not labels.any()
    s = mr.sums(key, labels)
    assert int(np.argmin(s)) == 11 and int((s == s.min()).sum()) == 1 and s[11] < s[0]
    assert mr.medoids(key, labels).tolist() == [11] * n
    # --min-global 0.5 (DCTglobal's keys): three clusters of 13, 7 and 6, the last decided by a genuine tie
    labels, _ = cluster_rule.labels(dct, idx, min_global=0.5)
    key = mr.key_matrix(dct, idx, 'global', tri)
    sizes = {int(c): int((labels == c).sum()) for c in np.unique(labels)}
    assert {c: k for c, k in sizes.items() if k > 1} == {0: 13, 8: 7, 21: 6}
    rep = mr.medoids(key, labels)
    want = {0: 7, 8: 14, 21: 24}
    assert rep.tolist() == [want.get(int(c), int(c)) for c in labels]
    s = mr.sums(key, labels)
    tied = np.flatnonzero((labels == 21) & (s == s[24]))
    assert len(tied) == 2 and tied[0] == 24
    # both cut-offs: the 'global' route's keys as well
    both, _ = cluster_rule.labels(dct, idx, min_domain=0.5, min_global=0.5)
    assert np.array_equal(both, labels) and np.array_equal(mr.medoids(key, both), rep)


# ---- 2. the text

IDS = {'ascii': lambda n: np.array([f'p{k * 37 % 101}' + 'x' * (k % 4) for k in range(n)]),
       'non-ascii': lambda n: np.array([f'protéine-{k}' if k % 3 else f'蛋白{k}' for k in range(n)]),
       'list': lambda n: [f'id{k}' for k in range(n)]}


@pytest.mark.parametrize('ids', sorted(IDS))
def test_the_composer_writes_the_rule_s_text(ids):
    from dctdomain_amd import dct_sim
    n = 40
    sid = IDS[ids](n)
    rng = np.random.default_rng(3)
    labels = cluster_rule.components(n, rng.integers(0, n, 25), rng.integers(0, n, 25))
    key = rng.integers(0, 17001, size=(n, n))
    rep = mr.medoids(key + key.T, labels)
    assert (rep != labels).any() and len(set(labels.tolist())) > 3
    for chunk_bytes in (1 << 24, 64):
        got = b''.join(bytes(c) for c in dct_sim.medoid_cluster_lines(sid, labels, rep, chunk_bytes))
        assert got == mr.text([str(s) for s in sid], labels, rep)
        assert got == b''.join(bytes(c) for c in dct_sim.cluster_lines(sid, labels, chunk_bytes, rep=rep))
    # the lines and their order are cluster_lines' own: only the first field differs
    plain = b''.join(bytes(c) for c in dct_sim.cluster_lines(sid, labels)).split(b'\n')
    assert plain == cluster_rule.text([str(s) for s in sid], labels).split(b'\n')
    assert [x.split(b' ')[1:] for x in got.split(b'\n')] == [x.split(b' ')[1:] for x in plain]
    assert b''.join(bytes(c) for c in dct_sim.medoid_cluster_lines(sid, labels, labels)) == b'\n'.join(plain)


def test_the_composer_refuses_representatives_that_do_not_fit():
    from dctdomain_amd import dct_sim
    with pytest.raises(ValueError):
        list(dct_sim.medoid_cluster_lines(['a', 'b'], [0, 0], [0]))
    with pytest.raises(IndexError):
        list(dct_sim.medoid_cluster_lines(['a', 'b'], [0, 0], [0, 2]))
    assert list(dct_sim.medoid_cluster_lines([], [], [])) == []


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


CLUSTER = ['--cluster', '--min-domain', '0.5']


@pytest.mark.parametrize('argv, message', [
    (['--rep', 'medoid'], '--rep says which member names a cluster: it needs --cluster'),
    (['--rep', 'first', '--min-domain', '0.5'], '--rep says which member names a cluster: it needs --cluster'),
    (CLUSTER + ['--level', 'domain', '--rep', 'medoid'], '--rep names clusters of proteins: not with --level domain'),
    (CLUSTER + ['--level', 'domain', '--rep', 'first'], '--rep names clusters of proteins: not with --level domain'),
    (CLUSTER + ['--linkage', 'greedy', '--rep', 'medoid'], '--rep medoid names single-linkage clusters: not with --linkage greedy'),
    (['--tree', '--rep', 'medoid'], '--tree prints the single-linkage tree of --dct: not with --rep'),
    (['--db', 'y', '--rbh', '--rep', 'first'], '--rbh prints the reciprocal best hits of --dct and --db: not with --rep'),
    (['--assign', 'r', '--min-domain', '0.5', '--rep', 'medoid'],
     '--assign places the proteins of --dct on a fixed set of representatives: not with --rep'),
    (CLUSTER + ['--rep', 'first', '--reps-out', 'f'],
     '--reps-out writes representatives: it needs --assign, or --cluster --linkage greedy at protein level'),
    (CLUSTER + ['--reps-out', 'f'], '--reps-out writes representatives: it needs --assign, or --cluster --linkage greedy at protein level'),
    (['--cluster', '--rep', 'medoid'], '--cluster needs a cut-off: --min-domain, --min-global or both'),
    (CLUSTER + ['--rep', 'median'], "argument --rep: invalid choice: 'median' (choose from 'first', 'medoid')"),
])
def test_the_parser_refuses(argv, message):
    got = _parse(argv)
    assert isinstance(got, str) and got.startswith(message), got


def test_the_greedy_refusal_says_why():
    got = _parse(CLUSTER + ['--linkage', 'greedy', '--rep', 'medoid'])
    assert 'every member is within the cut-offs of its representative' in got and 'medoid would break that' in got


def test_the_parser_accepts():
    plain = _parse(CLUSTER)
    assert 'rep' not in plain
    assert _parse(CLUSTER + ['--rep', 'first']) == plain                    # (the default: the same namespace)
    assert _parse(CLUSTER + ['--linkage', 'greedy', '--rep', 'first']) == _parse(CLUSTER + ['--linkage', 'greedy'])
    assert _parse(CLUSTER + ['--rep', 'medoid']) == dict(plain, rep='medoid')
    assert _parse(CLUSTER + ['--linkage', 'single', '--level', 'protein', '--rep', 'medoid', '--reps-out', 'f']) == \
        dict(plain, rep='medoid', linkage='single', level='protein', reps_out='f')
    assert _parse(['--cluster', '--min-global', '0.5', '--min-domain', '0.5', '--min-coverage', '0.8', '--rep', 'medoid']) == \
        dict(plain, min_global=0.5, min_coverage=0.8, rep='medoid')


def test_cluster_sim_refuses_what_the_parser_refuses(tmp_path):
    from dctdomain_amd import dct_sim
    out = str(tmp_path / 'out.txt')
    for kw in ({'rep': 'median'}, {'rep': 'medoid', 'linkage': 'greedy'}, {'rep': 'medoid', 'level': 'domain'},
               {'rep': 'first', 'reps_out': str(tmp_path / 'r.npz')}):
        with pytest.raises(ValueError):
            dct_sim.cluster_sim(G6PD, out, min_domain=0.5, **kw)


def test_a_file_of_singletons_needs_no_device(tmp_path, g6pd, capsys):
    """A cut-off above 1: every protein its own cluster and its own medoid -- no tile, no sums, no GPU."""
    from dctdomain_amd import dct_sim
    sid, idx, dct, _ = g6pd
    job = dct_sim.Clusters(sid, idx, dct, min_domain=1.5)
    assert job.medoids().tolist() == list(range(len(sid))) and job.medoids().dtype == np.int32
    out, reps = str(tmp_path / 'out.txt'), str(tmp_path / 'reps-dct.npz')
    dct_sim.main(['--dct', G6PD, '--cluster', '--min-domain', '1.5', '--rep', 'medoid', '--output', out, '--reps-out', reps])
    with open(out, 'rb') as fh:
        assert fh.read() == cluster_rule.HEADER + mr.text(sid, np.arange(len(sid)), np.arange(len(sid)))
    rsid, ridx, rfps = dct_sim._load_npz(reps)
    assert [str(s) for s in rsid] == sid and np.array_equal(ridx, idx) and np.array_equal(rfps, dct)


# ---- 4. the build

def test_the_export_is_declared_bound_and_built():
    import build_ext
    from dctdomain_amd import _lib, similarity
    with open(os.path.join(ROOT, 'include', 'dctfp.h')) as fh:
        header = fh.read()
    decl = re.search(r'\nint dctfp_label_sums\(([^;]*)\);', header)
    assert decl and decl.group(1).count(',') == 14               # ctx, the ten tile values, labels, sums, n_nodes, stream
    doc = header[:decl.start()].rsplit('/*', 1)[1]
    assert re.fullmatch(r'.*\*/\s*', doc, flags=re.S) and 'bound' in doc and 'DCTFP_ERR_INVALID' in doc
    assert int(re.search(r'#define DCTFP_VERSION (\d+)', header).group(1)) >= 112
    assert 'dctfp_label_sums' in _lib.EXPORTS and callable(similarity.label_sums)
    assert 'k_medoid.hip' in build_ext.UNITS
    csrc = os.path.join(ROOT, 'dctdomain_amd', 'csrc')
    with open(os.path.join(csrc, 'k_medoid.hip')) as fh:
        unit = fh.read()
    assert 'label_sums_kernel(const TriTile t, ' in unit and '__hip_atomic_fetch_add(' in unit and '__HIP_MEMORY_SCOPE_AGENT' in unit
    assert '#include "tri_walk.hip.h"' not in unit and '#include "band_walk.hip.h"' in unit
    code = '\n'.join(line.split('//', 1)[0] for line in unit.splitlines())
    assert 'asm' not in code and code.count('__ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT') == 1     # add_sum
    # a pass of the one band walk, with no bound; sums is only ever offset and handed to add_sum, in the pass's two flushes, and
    # labels is read in _label alone, which the pass's side() calls
    assert 'band_walk(t, n_bands, n_steps, LabelSumsPass{labels, sums});' in code and 'kBounded = false' in code
    assert not re.search(r'\bsums\s*\[', code) and len(re.findall(r'add_sum\(sums \+ ', code)) == 2
    assert re.search(r'void row_out\([^)]*\) const \{ add_sum\(sums \+ ', code) and re.search(r'void col_out\([^)]*\) const \{ add_sum\(sums \+ ', code)
    assert re.findall(r'[^\n]*\blabels\s*\[[^\n]*', code) == ['__device__ inline int32_t _label(const int32_t* __restrict__ labels, int64_t x) { return labels[x]; }']
    assert len(re.findall(r'_label\(', code)) == 2 and 'Side side(int64_t x) const { return _label(labels, x); }' in code
    assert not re.search(r'\bwhile\b|for \(;;\)', code)
    with open(os.path.join(csrc, 'launch.h')) as fh:
        assert 'void launch_label_sums(' in fh.read()
    with open(os.path.join(csrc, 'dctfp_sim.hip')) as fh:
        host = fh.read()
    body = host[host.index('\nint dctfp_label_sums('):host.index('DCTFP_GUARD("dctfp_label_sums")')]
    assert 'check_tri_tile(' not in body and 'label_sums_max_cap()' in body
    assert body.count('check_band_tile("dctfp_label_sums", t, n_nodes)') == 1 and 'cap, cap};' in body     # (no cut-off: the tile's bound is its cap)
    with open(os.path.join(ROOT, 'INTEGRATION.md')) as fh:
        assert 'dctfp_label_sums' in fh.read()
    import ctypes
    for path in (_lib.LIB_PATH, _lib.EXPERIMENTS_LIB_PATH):
        assert hasattr(ctypes.CDLL(path), 'dctfp_label_sums')
    fn = _lib._configure(ctypes.CDLL(_lib.LIB_PATH)).dctfp_label_sums
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 15
