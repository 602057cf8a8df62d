"""CPU-side checks of dct-sim --assign: the oracle (assign_rule.py, the GPU tests' reference) on an example worked by hand and
on the committed reference golden (the split property, with greedy_rule alone), the command line, the --reps-out writer, and
the entry point in the libraries and the header."""

import ctypes
import os
import re

import numpy as np
import pytest

import all_sim_filter_rule as rule
import assign_rule as arule
import golden_util as gu
import greedy_rule as grule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPZ = os.path.join(gu.GOLD, 'all_sim', 'all-dct.npz')
CUTS = [{'min_domain': x} for x in (0.1, 0.5, 0.9, 1.0)] + [{'min_global': y} for y in (0.1, 0.5, 0.9, 1.0)] + \
       [{'min_domain': 0.25, 'min_global': 0.1}, {'min_domain': 0.9, 'min_global': 0.5}, {'min_domain': 0.5, 'min_global': 0.9}]


# ---- the rule worked by hand

def test_five_proteins_by_hand():
    """R = {0, 1}, N = {2, 3, 4, 5, 6}.  The edge 0-1 lies inside R and does not exist: both stay representatives.  2 has edges
    from 0 and 1: the lower wins.  3 has none from a representative: a new one.  4 has edges from 2 (a member: it covers nobody)
    and 3: label 3.  5 has an edge from 1 and from 3: label 1.  6 has an edge from 4 only, a member: a new representative."""
    i, j = [0, 0, 1, 2, 3, 1, 3, 4], [1, 2, 2, 4, 4, 5, 5, 6]
    got = arule.assign(2, 5, i, j)
    assert got.dtype == np.int32 and got.tolist() == [0, 3, 3, 1, 6]
    arule.check(2, 5, i, j, got)
    assert arule.assign(2, 5, j, i).tolist() == got.tolist()              # (an edge either way round)
    # with R forced this differs from greedy on the concatenation: there 1 would be 0's member and cover nobody
    assert grule.greedy(7, i, j).tolist() == [0, 0, 0, 3, 3, 3, 6]
    assert arule.text(['r0', 'r1'], ['a', 'b', 'c', 'd', 'e'], got) == b'r0 a\nr1 d\nb b\nb c\ne e\n'


def test_check_refuses_wrong_labels():
    i, j = [0, 0, 1, 2, 3, 1, 3, 4], [1, 2, 2, 4, 4, 5, 5, 6]
    for wrong in ([1, 3, 3, 1, 6], [0, 3, 4, 1, 6], [0, 3, 3, 3, 6], [0, 3, 3, 1, 4], [0, 3, 3, 5, 6], [2, 3, 3, 1, 6]):
        with pytest.raises(AssertionError):
            arule.check(2, 5, i, j, np.array(wrong))


def test_no_representatives_is_greedy_and_no_new_proteins_is_empty():
    i, j = [0, 1, 2, 3], [1, 2, 3, 4]
    assert arule.assign(0, 5, i, j).tolist() == grule.greedy(5, i, j).tolist() == [0, 0, 2, 2, 4]
    assert arule.assign(5, 0, i, j).tolist() == []
    assert arule.assign(0, 0, [], []).tolist() == []


# ---- the split property on the reference's 139 proteins, with greedy_rule alone

@pytest.fixture(scope='module')
def golden():
    with np.load(NPZ) as data:
        sid, idx, dct = [str(s) for s in data['sid']], np.asarray(data['idx'], dtype=np.int64), data['dct']
    return sid, idx, dct, rule.triangle_l1(dct, idx)


def split_oracle(tri, n, k, kw):
    """(representatives among the first k proteins, labels of the rest in the split's numbering -- both from greedy_rule)."""
    i, j, mn, last = tri
    keep = rule.kept(mn, last, **kw)
    whole = grule.greedy(n, i[keep], j[keep])
    reps = np.flatnonzero(whole[:k] == np.arange(k))
    # node x of the file is node (its rank among reps) when a representative below k, m + x - k from k on
    renumber = np.full(n, -1, dtype=np.int64)
    renumber[reps] = np.arange(len(reps))
    renumber[k:] = len(reps) + np.arange(n - k)
    want = renumber[whole[k:]]
    assert (want >= 0).all()                                  # (a label is a representative: it is in R or in N)
    return reps, want, (i[keep], j[keep], renumber)


@pytest.mark.parametrize('kw', CUTS, ids=lambda kw: ','.join(f'{k[4:]}={v}' for k, v in kw.items()))
@pytest.mark.parametrize('k', [0, 1, 46, 138, 139])
def test_split_property_on_the_reference_golden(golden, kw, k):
    sid, idx, dct, tri = golden
    n = 139
    reps, want, (ei, ej, renumber) = split_oracle(tri, n, k, kw)
    # the assignment's graph: the file's edges among R u N, renumbered -- members of the first part are not nodes
    ok = (renumber[ei] >= 0) & (renumber[ej] >= 0)
    got = arule.assign(len(reps), n - k, renumber[ei[ok]], renumber[ej[ok]])
    assert np.array_equal(got, want)
    arule.check(len(reps), n - k, renumber[ei[ok]], renumber[ej[ok]], got)


def test_edges_of_the_two_files_are_the_edges_of_the_concatenation(golden):
    sid, idx, dct, tri = golden
    k = 46
    rep_idx, new_idx = idx[:k + 1], idx[k:] - idx[k]
    for kw in ({'min_domain': 0.5}, {'min_global': 0.5}, {'min_domain': 0.25, 'min_global': 0.1}):
        i, j = arule.edges(dct[:idx[k]], rep_idx, dct[idx[k]:], new_idx, **kw)
        ti, tj, mn, last = tri
        keep = rule.kept(mn, last, **kw) & (tj >= k)
        assert np.array_equal(i, ti[keep]) and np.array_equal(j, tj[keep]) and len(i)


# ---- the command line

def _parse(argv):
    from dctdomain_amd import dct_sim
    return dct_sim.build_parser().parse_args(['--dct', 'x.npz'] + argv)


@pytest.mark.parametrize('argv,want', [
    (['--assign', 'r.npz', '--min-domain', '0.5'], dict(assign='r.npz', min_domain=0.5, min_global=None)),
    (['--assign', 'r.npz', '--min-global', '0.25', '--output', 'o'], dict(assign='r.npz', min_global=0.25, output='o')),
    (['--assign', 'r.npz', '--min-domain', '0.5', '--min-global', '0.3', '--reps-out', 'all.npz'],
     dict(assign='r.npz', min_domain=0.5, min_global=0.3, reps_out='all.npz')),
    (['--cluster', '--linkage', 'greedy', '--min-domain', '0.5', '--reps-out', 'r0.npz'], dict(cluster=True, linkage='greedy', reps_out='r0.npz')),
    (['--cluster', '--linkage', 'greedy', '--level', 'protein', '--min-global', '0.5', '--reps-out', 'r0.npz'],
     dict(cluster=True, level='protein', reps_out='r0.npz')),
])
def test_parser_accepts(argv, want):
    args = vars(_parse(argv))
    assert {k: args[k] for k in want} == want
    assert args['cluster'] is bool(want.get('cluster', False))


@pytest.mark.parametrize('argv,said', [
    (['--assign', 'r.npz'], '--assign needs a cut-off'),
    (['--assign'], 'expected one argument'),
    (['--assign', 'r.npz', '--min-domain', '0.5', '--pair', 'p.txt'], 'not with --pair'),
    (['--assign', 'r.npz', '--min-domain', '0.5', '--db', 'd.npz'], 'not with --db'),
    (['--assign', 'r.npz', '--min-domain', '0.5', '--cluster'], 'not with --cluster'),
    (['--assign', 'r.npz', '--min-domain', '0.5', '--rank', 'domain'], 'not with --rank'),
    (['--assign', 'r.npz', '--min-domain', '0.5', '--domains'], 'not with --domains'),
    (['--assign', 'r.npz', '--min-domain', '0.5', '--dom', 'x.dom'], 'not with --dom'),
    (['--assign', 'r.npz', '--min-domain', '0.5', '--db-dom', 'y.dom'], 'not with --db-dom'),
    (['--assign', 'r.npz', '--min-domain', '0.5', '--linkage', 'greedy'], 'not with --linkage'),
    (['--assign', 'r.npz', '--min-domain', '0.5', '--level', 'protein'], 'not with --level'),
    (['--assign', 'r.npz', '--min-domain', '0.5', '--no-whole'], 'not with --no-whole'),
    (['--reps-out', 'r.npz'], '--reps-out writes representatives'),
    (['--reps-out', 'r.npz', '--min-domain', '0.5'], '--reps-out writes representatives'),
    (['--reps-out', 'r.npz', '--cluster', '--min-domain', '0.5'], '--reps-out writes representatives'),
    (['--reps-out', 'r.npz', '--cluster', '--linkage', 'single', '--min-domain', '0.5'], '--reps-out writes representatives'),
    (['--reps-out', 'r.npz', '--cluster', '--level', 'domain', '--min-domain', '0.5'], '--reps-out writes representatives'),
    (['--reps-out', 'r.npz', '--db', 'd.npz'], '--reps-out writes representatives'),
    (['--reps-out'], 'expected one argument'),
    (['--min-domain', '0.5', '--pair', 'p.txt'], '--min-domain applies to all-against-all only'),
    (['--min-global', '0.5', '--db', 'd.npz'], '--min-global applies to all-against-all only'),
    (['--cluster', '--level', 'domain', '--linkage', 'greedy', '--min-domain', '0.5'], 'not with --linkage greedy'),
    (['--cluster', '--level', 'domain', '--linkage', 'greedy', '--min-domain', '0.5', '--reps-out', 'r.npz'], 'greedy'),
])
def test_parser_rejects(argv, said, capsys):
    with pytest.raises(SystemExit) as e:
        _parse(argv)
    assert e.value.code == 2
    assert said in capsys.readouterr().err


def test_old_command_lines_parse_to_what_they_parsed_to():
    assert vars(_parse(['--cluster', '--min-global', '0.25', '--output', 'o'])) == dict(
        dct='x.npz', output='o', pair=None, pairfound=None, db=None, top=5, threshold=0.25, rank=None, min_domain=None, min_global=0.25,
        cluster=True)
    assert vars(_parse(['--min-domain', '0.5'])) == dict(
        dct='x.npz', output=None, pair=None, pairfound=None, db=None, top=5, threshold=0.25, rank=None, min_domain=0.5, min_global=None,
        cluster=False)
    for argv in ([], ['--cluster', '--min-domain', '0.5', '--linkage', 'greedy'], ['--db', 'd.npz', '--rank', 'domain'], ['--pair', 'p']):
        assert not {'assign', 'reps_out'} & set(vars(_parse(argv)))


def test_mode_functions_keep_their_signatures_and_assign_sim_has_the_stated_one():
    import inspect
    from dctdomain_amd import dct_sim
    assert list(inspect.signature(dct_sim.Assignment.__init__).parameters) == ['self', 'rep_sid', 'rep_idx', 'rep_fps', 'sid', 'idx', 'fps',
                                                                               'min_domain', 'min_global']
    assert dct_sim.assign_sim.__name__ == 'assign_sim' and 'representative member' in dct_sim.assign_sim.__doc__
    with pytest.raises(ValueError):
        dct_sim.assign_sim(NPZ, NPZ, None)                    # no cut-off: refused before anything is loaded
    with pytest.raises(ValueError):
        dct_sim.cluster_sim(NPZ, None, min_domain=0.5, reps_out='x.npz')           # (single linkage has no representatives to chain)
    with pytest.raises(ValueError):
        dct_sim.cluster_sim(NPZ, None, min_domain=0.5, level='domain', reps_out='x.npz')


# ---- no device: degenerate cut-offs, empty sides, the text

def test_a_cut_off_above_one_gives_every_new_protein_its_own_label_without_a_device(golden, tmp_path, capsys):
    from dctdomain_amd import dct_sim
    sid, idx, dct, _ = golden
    k = 46
    rep = (sid[:k], idx[:k + 1], dct[:idx[k]])
    new = (sid[k:], idx[k:] - idx[k], dct[idx[k]:])
    for kw in ({'min_domain': 1.0001}, {'min_global': 1.5}, {'min_domain': 0.5, 'min_global': 1.0001}):
        got = dct_sim.Assignment(*rep, *new, **kw).labels()
        assert got.dtype == np.int32 and np.array_equal(got, k + np.arange(139 - k))
        assert np.array_equal(got, arule.labels(rep[2], rep[1], new[2], new[1], **kw))
    # cut-offs that exclude nothing: FilteredPairs keeps every pair, node 0 has an edge to every new protein
    for kw in ({'min_domain': 0.0}, {'min_global': -1.0}, {'min_domain': float('nan'), 'min_global': 0.0}):
        assert not dct_sim.Assignment(*rep, *new, **kw).labels().any()
        assert not arule.labels(rep[2], rep[1], new[2], new[1], **kw).any()
        assert not dct_sim.Assignment([], [0], dct[:0], *new, **kw).labels().any()      # (no representatives: the first new protein)
        assert not arule.labels(dct[:0], [0], new[2], new[1], **kw).any()
    # no new proteins: no label, no line
    job = dct_sim.Assignment(*rep, [], [0], dct[:0], min_domain=0.5)
    assert job.labels().tolist() == [] and list(dct_sim.assign_lines(rep[0], [], [])) == []
    with pytest.raises(ValueError):
        dct_sim.Assignment(*rep, *new)
    # through the command line
    paths = [str(tmp_path / name) for name in ('r-dct.npz', 'n-dct.npz', 'out.txt', 'all-dct.npz')]
    np.savez(paths[0], sid=np.array(rep[0]), idx=rep[1], dct=rep[2])
    np.savez(paths[1], sid=np.array(new[0]), idx=new[1], dct=new[2], dom=np.array(['1-9'] * len(new[2])))
    dct_sim.main(['--dct', paths[1], '--assign', paths[0], '--min-domain', '1.5', '--output', paths[2], '--reps-out', paths[3]])
    assert open(paths[2], 'rb').read() == arule.HEADER + ''.join(f'{s} {s}\n' for s in new[0]).encode()
    got_sid, got_idx, got_dct = dct_sim._load_npz(paths[3])
    assert [str(s) for s in got_sid] == sid and np.array_equal(got_idx, idx) and np.array_equal(got_dct, dct)
    with np.load(paths[3]) as data:
        assert 'dom' not in data.files                         # (the representatives' file carries none)


def test_assign_lines_order_and_ids():
    from dctdomain_amd import dct_sim
    labels = [0, 3, 3, 1, 6]
    for rep_sid, sid in ((['r0', 'r1'], ['a', 'b', 'c', 'd', 'e']), (np.array(['r0', 'r1']), np.array(['a', 'b', 'c', 'd', 'e'])),
                         (['ré', 'r1'], ['蛋', 'b', 'c', 'd', 'e😀']), (np.array(['r0', 'r1']), ['a', 'b', 'c', 'd', 'e'])):
        got = b''.join(bytes(memoryview(t)) for t in dct_sim.assign_lines(rep_sid, sid, labels, chunk_bytes=7))
        assert got == arule.text(rep_sid, sid, np.array(labels))
    assert arule.text(['r0', 'r1'], ['a', 'b', 'c', 'd', 'e'], np.array(labels)) == b'r0 a\nr1 d\nb b\nb c\ne e\n'
    with pytest.raises(IndexError):
        list(dct_sim.assign_lines(['r'], ['a'], [2]))
    with pytest.raises(ValueError):
        list(dct_sim.assign_lines(['r'], ['a'], [0, 0]))


# ---- --reps-out

def test_reps_writer_round_trip_and_the_dom_rule(tmp_path):
    from dctdomain_amd import dct_sim
    rng = np.random.default_rng(5)
    sid_a, idx_a = np.array(['p0', 'p1', 'p2']), np.array([0, 2, 2, 5])
    sid_b, idx_b = np.array(['q0', 'longer-id-q1', 'q2', 'q3']), np.array([0, 1, 4, 4, 6])
    fps_a, fps_b = rng.integers(-128, 128, size=(5, 16), dtype=np.int8), rng.integers(-128, 128, size=(6, 16), dtype=np.int8)
    dom_a, dom_b = np.array([f'a{r}' for r in range(5)]), np.array([f'1-{r},7-9' for r in range(6)])
    path = str(tmp_path / 'reps.out')                          # (written to this very name: no suffix is added)
    dct_sim.write_reps(path, [(sid_a, idx_a, fps_a, dom_a, None), (sid_b, idx_b, fps_b, dom_b, np.array([1, 2]))])
    sid, idx, dct = dct_sim._load_npz(path)
    assert sid.tolist() == ['p0', 'p1', 'p2', 'longer-id-q1', 'q2'] and idx.tolist() == [0, 2, 2, 5, 8, 8] and idx.dtype == np.int64
    assert dct.dtype == np.int8 and np.array_equal(dct, np.concatenate([fps_a, fps_b[1:4]]))
    assert dct_sim._npz_dom(path, 8).tolist() == dom_a.tolist() + dom_b[1:4].tolist()
    # one part without names: none are written
    dct_sim.write_reps(path, [(sid_a, idx_a, fps_a, None, None), (sid_b, idx_b, fps_b, dom_b, np.array([0]))])
    with np.load(path) as data:
        assert sorted(data.files) == ['dct', 'idx', 'sid'] and data['idx'].tolist() == [0, 2, 2, 5, 6]
    assert dct_sim._npz_dom(path, 6) is None
    # nothing chosen from the second part, nothing at all
    dct_sim.write_reps(path, [(sid_a, idx_a, fps_a, dom_a, None), (sid_b, idx_b, fps_b, dom_b, np.zeros(0, dtype=np.int64))])
    assert dct_sim._load_npz(path)[1].tolist() == idx_a.tolist() and dct_sim._npz_dom(path, 5).tolist() == dom_a.tolist()
    dct_sim.write_reps(path, [(sid_a[:0], idx_a[:1], fps_a[:0], dom_a[:0], None)])
    sid, idx, dct = dct_sim._load_npz(path)
    assert len(sid) == 0 and idx.tolist() == [0] and dct.shape == (0, 16)
    with pytest.raises(ValueError):
        dct_sim._npz_dom(path, 3)                              # names that do not go with the rows


# ---- the library

PARAMS = ('dctfp_ctx* ctx, const int8_t* a, int64_t na, int64_t lda, const int32_t* value_a, int64_t a0, const int8_t* b, int64_t nb, '
          'int64_t ldb, const int32_t* slot_b, int64_t b0, int32_t d, int32_t cap, int32_t bound, int32_t* assign, int64_t n_assign, void* stream')


def test_library_exports_the_entry_point_and_header_documents_it():
    from dctdomain_amd import _lib
    with open(os.path.join(ROOT, 'include', 'dctfp.h')) as fh:
        header = fh.read()
    decl = re.search(r'int dctfp_rows_assign\(([^;]*)\);', header)
    assert decl and ' '.join(decl.group(1).split()) == PARAMS
    doc = header[:decl.start()].rsplit('/*', 1)[1]
    assert '*/' in doc and 'DCTFP_ERR_LIMIT' in doc and 'DCTFP_ERR_INVALID' in doc and 'dctfp_rows_link' in doc
    assert re.fullmatch(r'\s*', doc.split('*/', 1)[1]), 'the comment must sit right above the declaration'
    version = int(re.search(r'#define DCTFP_VERSION (\d+)', header).group(1))
    assert version >= 108                                       # (the parent commit's: 107)
    for path in (_lib.LIB_PATH, _lib.EXPERIMENTS_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert hasattr(lib, 'dctfp_rows_assign') and lib.dctfp_version() == version
    assert 'dctfp_rows_assign' in _lib.EXPORTS
    fn = _lib._configure(ctypes.CDLL(_lib.LIB_PATH)).dctfp_rows_assign
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 17 == len(PARAMS.split(','))
    launch = open(os.path.join(ROOT, 'dctdomain_amd', 'csrc', 'launch.h')).read()
    assert 'void launch_rows_assign(' in launch
    assert 'dctfp_rows_assign' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


def test_new_unit_is_part_of_the_build_and_uses_atomics_only_on_assign():
    import build_ext
    assert 'k_assign.hip' in build_ext.UNITS
    text = open(os.path.join(ROOT, 'dctdomain_amd', 'csrc', 'k_assign.hip')).read()
    code = '\n'.join(line.split('//', 1)[0] for line in text.splitlines())
    # every use of assign in the kernel's body is an agent-scope relaxed atomic
    uses = re.findall(r'[^\n]*\bassign \+ slot[^\n]*', code)
    assert len(uses) == 2 and all('__hip_atomic_' in u and '__ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT' in u for u in uses)
    assert '__hip_atomic_fetch_min(assign + slot' in code and 'assign[' not in code
    assert '__launch_bounds__(256, 4)' in code and '__builtin_amdgcn_sad_u8' in code


def test_null_and_bad_shapes_are_refused_without_a_device():
    """No context can be made without a device, so every call here ends at the NULL check -- whatever else is wrong with it --
    and none may touch its arguments; the shape checks behind a context are test_assign_gpu.py's."""
    from dctdomain_amd import _lib
    lib = _lib._configure(ctypes.CDLL(_lib.LIB_PATH))
    buf = (ctypes.c_int8 * 1024)()
    out = (ctypes.c_int32 * 4)()
    p, o = ctypes.addressof(buf), ctypes.addressof(out)
    for args in ((None, None, 1, 480, None, 0, None, 1, 480, None, 0, 480, 17000, 0, None, 1, None),       # all NULL
                 (None, p, 1, 480, None, 0, p, 1, 480, None, 0, 480, 17000, 0, o, 4, None),                # only the context
                 (None, p, -1, 480, None, 0, p, 1, 480, None, 0, 480, 17000, 0, o, 4, None),               # ... and a negative count
                 (None, p, 1, 479, None, 0, p, 1, 480, None, 0, 480, 17000, 0, o, 4, None),                # ... lda < d
                 (None, p, 1, 480, None, 0, p, 1, 480, None, 0, 0, 17000, 0, o, 4, None),                  # ... d = 0
                 (None, p, 1, 480, None, 0, p, 1, 480, None, 0, 480, 17000, -1, o, 4, None)):              # ... a bound below 0
        assert lib.dctfp_rows_assign(*args) == _lib.DCTFP_ERR_INVALID
        assert b'dctfp_rows_assign: NULL argument' in lib.dctfp_last_error()
    assert list(out) == [0, 0, 0, 0]


def test_the_wrapper_is_public_and_carries_the_stated_signature():
    import inspect
    from dctdomain_amd import similarity
    assert list(inspect.signature(similarity.rows_assign).parameters) == ['a', 'b', 'assign', 'bound', 'value_a', 'slot_b', 'a0', 'b0', 'cap']
    assert inspect.signature(similarity.rows_assign).parameters['cap'].default == 17000
