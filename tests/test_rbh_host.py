"""CPU-side checks of dct-sim --db --rbh: the numpy oracle (rbh_rule.py, the GPU tests' reference) pinned on the reference's own
db_search text of the committed golden, its tie rule, the command line, the cases that need no device, and the entry point in
the libraries and the header."""

import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import rbh_rule as rrule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = rrule.GOLD


# ---- the rule on the reference's text

def test_rule_agrees_with_the_reference_search_on_the_golden():
    (sid, idx, dct), (db_sid, db_idx, db_dct) = rrule.golden_files()
    first, _ = rrule.reference_rbh_lines()
    assert len(first) == len(sid) == 28                          # (every query has a printed hit: its best one comes first)
    k = rrule.keys(dct, idx, db_dct, db_idx, 'global')
    (best_b, key), (best_a, _) = rrule.best(k)
    assert [db_sid[b] for b in best_b.tolist()] == [first[q].split()[1] for q in sid]
    assert np.array_equal(key, k.min(axis=1))
    a, b, kk = rrule.pairs(k)
    assert len(a) >= 20 and np.array_equal(best_a[b], a) and np.array_equal(kk, k[a, b]) and (np.diff(a) > 0).all()
    # the rule's lines are those reference lines, verbatim
    assert rrule.text(sid, dct, idx, db_sid, db_dct, db_idx, 'global') == [first[sid[x]] for x in a.tolist()]


def test_ties_go_to_the_lower_index_on_both_sides():
    rng = np.random.default_rng(5)
    x, y = rng.integers(0, 128, (2, 480)).astype(np.int8)
    a, ia = np.stack([x, x, y]), [0, 1, 2, 3]                    # proteins 0 and 1 of A are identical
    b, ib = np.stack([y, x, x]), [0, 1, 2, 3]                    # proteins 1 and 2 of B are identical
    for score in ('domain', 'global'):
        k = rrule.keys(a, ia, b, ib, score)
        assert k[0, 1] == k[0, 2] == k[1, 1] == k[1, 2] == 0 == k[2, 0]
        (best_b, key), (best_a, _) = rrule.best(k)
        assert best_b.tolist() == [1, 1, 0] and best_a.tolist() == [2, 0, 0] and key.tolist() == [0, 0, 0]
        pa, pb, pk = rrule.pairs(k)
        assert (pa.tolist(), pb.tolist(), pk.tolist()) == ([0, 2], [1, 0], [0, 0])
    # a bound below every key, and a protein without fingerprints: no hit, whatever the bound
    assert all((v == -1).all() for side in rrule.best(k, -1) for v in side)
    k = rrule.keys(a, [0, 1, 1, 3], b, ib, 'domain')
    assert (k[1] == rrule.CAP).all() and rrule.best(k, rrule.CAP - 1)[0][0][1] == -1


# ---- the command line

def _parse(*argv):
    from dctdomain_amd import dct_sim
    return dct_sim.build_parser().parse_args(['--dct', 'x-dct.npz'] + list(argv))


def test_rbh_alone_parses_to_domain_and_is_absent_otherwise():
    assert _parse('--db', 'y.npz', '--rbh').rbh == 'domain' and _parse('--db', 'y.npz', '--rbh', 'domain').rbh == 'domain'
    assert _parse('--rbh', 'global', '--db', 'y.npz').rbh == 'global'
    assert not hasattr(_parse(), 'rbh') and not hasattr(_parse('--db', 'y.npz'), 'rbh') and not hasattr(_parse('--min-domain', '0.5'), 'rbh')
    assert _parse('--db', 'y.npz', '--rbh', '--min-domain', '0.5').min_domain == 0.5
    assert _parse('--db', 'y.npz', '--rbh', 'global', '--min-global', '0.25', '--output', 'o').min_global == 0.25
    ns = _parse('--db', 'y.npz', '--rbh', '--db-dom', 'y.dom')
    assert ns.domains is True and ns.db_dom == 'y.dom'
    assert _parse('--db', 'y.npz', '--rbh', '--domains', '--dom', 'x.dom').dom == 'x.dom'


@pytest.mark.parametrize('argv', [
    ['--rbh'], ['--rbh', 'global'], ['--rbh', '--db', 'y.npz', '--pair', 'p'], ['--rbh', '--db', 'y.npz', '--cluster', '--min-domain', '0.5'],
    ['--rbh', '--db', 'y.npz', '--assign', 'r.npz', '--min-domain', '0.5'], ['--rbh', '--db', 'y.npz', '--tree'],
    ['--rbh', '--db', 'y.npz', '--rank', 'domain'], ['--rbh', '--db', 'y.npz', '--rank', 'global'], ['--rbh', '--db', 'y.npz', '--linkage', 'greedy'],
    ['--rbh', '--db', 'y.npz', '--level', 'domain'], ['--rbh', '--db', 'y.npz', '--no-whole'], ['--rbh', '--db', 'y.npz', '--reps-out', 'r.npz'],
    ['--rbh', '--db', 'y.npz', '--min-global', '0.5'], ['--rbh', 'domain', '--db', 'y.npz', '--min-global', '0.5'],
    ['--rbh', 'global', '--db', 'y.npz', '--min-domain', '0.5'], ['--rbh', 'domain', '--db', 'y.npz', '--min-domain', '0.5', '--min-global', '0.5'],
    ['--db', 'y.npz', '--rbh', 'protein'],
], ids=lambda a: ' '.join(a))
def test_parser_errors(argv, capsys):
    with pytest.raises(SystemExit) as exit_:
        _parse(*argv)
    assert exit_.value.code == 2
    assert '--rbh' in capsys.readouterr().err


@pytest.mark.parametrize('opt', ['--min-domain', '--min-global'])
def test_a_cut_off_beside_db_without_rbh_is_still_the_old_error(opt, capsys):
    with pytest.raises(SystemExit):
        _parse('--db', 'y.npz', opt, '0.5')
    assert f'{opt} applies to all-against-all only, not to --pair or --db' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        _parse('--pair', 'p', opt, '0.5')
    assert f'{opt} applies to all-against-all only, not to --pair or --db' in capsys.readouterr().err


def test_rbh_sim_refuses_the_other_cut_off_and_an_unknown_score(tmp_path):
    from dctdomain_amd import dct_sim
    q, db = (os.path.join(GOLD, name + '-dct.npz') for name in ('query', 'db'))
    for kw in ({'score': 'domain', 'min_global': 0.5}, {'score': 'global', 'min_domain': 0.5}, {'score': 'protein'}):
        with pytest.raises(ValueError):
            dct_sim.rbh_sim(q, db, str(tmp_path / 'out.txt'), **kw)
    assert list(inspect.signature(dct_sim.ReciprocalBest.__init__).parameters) == ['self', 'sid_a', 'idx_a', 'fps_a', 'sid_b', 'idx_b', 'fps_b',
                                                                                 'score', 'min_cut']
    with pytest.raises(ValueError):
        dct_sim.ReciprocalBest(['a'], [0, 1], np.zeros((1, 480), np.int8), ['b'], [0, 1], np.zeros((1, 480), np.int8), score='protein')


# ---- without a device

def test_reciprocal_best_of_nothing_needs_no_device(tmp_path):
    from dctdomain_amd import dct_sim
    rows = np.zeros((2, 480), dtype=np.int8)
    two = (['a', 'b'], np.array([0, 1, 2]), rows)
    none = ([], np.array([0]), rows[:0])
    for side_a, side_b, kw in ((none, two, {}), (two, none, {}), (none, none, {'score': 'global'}), (two, two, {'min_cut': 1.5}),
                               (two, two, {'score': 'global', 'min_cut': 1.5})):
        job = dct_sim.ReciprocalBest(*side_a, *side_b, **kw)
        (best_b, key_a), (best_a, key_b) = job.best()
        assert len(best_b) == len(key_a) == len(side_a[0]) and len(best_a) == len(key_b) == len(side_b[0])
        assert all(v.dtype == np.int64 and (v == -1).all() for v in (best_b, key_a, best_a, key_b))
        assert all(v.dtype == np.int64 and len(v) == 0 for v in job.pairs())
        assert job.lines() == [] and job.lines(domains=True) == []
        report = dct_sim.Report(str(tmp_path / 'out.txt'))
        job.write(report)
        report.close()
        assert open(tmp_path / 'out.txt').read() == rrule.HEADER + '\n'
    assert dct_sim.ReciprocalBest(*two, *two).bound == 16999 == rrule.DEFAULT_BOUND
    assert dct_sim.ReciprocalBest(*two, *two, min_cut=0.5).bound == dct_sim.sim_bound(0.5) == 8500
    assert dct_sim.ReciprocalBest(*two, *two, 'global', 0.0).bound == 16999       # (a protein without fingerprints is never a hit)
    assert dct_sim.ReciprocalBest(*two, *two, min_cut=1.5).bound == -1
    for name in ('COL_ROWS', 'TILE_INTS', 'MAX_TILE_ROWS'):
        assert getattr(dct_sim.ReciprocalBest, name) == getattr(dct_sim.ProteinSearch, name)


# ---- the library

PARAMS = ('dctfp_ctx* ctx, const int32_t* tile, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row0, int64_t col0, '
          'const uint8_t* row_empty, const uint8_t* col_empty, int32_t cap, int32_t bound, uint64_t* best_row, int64_t n_a, '
          'uint64_t* best_col, int64_t n_b, void* stream')


def test_library_exports_the_entry_point_and_header_documents_it():
    from dctdomain_amd import _lib
    name = 'dctfp_rect_best'
    with open(os.path.join(ROOT, 'include', 'dctfp.h')) as fh:
        header = fh.read()
    decl = re.search(r'int %s\(([^;]*)\);' % name, header)
    assert decl and ' '.join(decl.group(1).split()) == PARAMS
    doc = header[:decl.start()].rsplit('/*', 1)[1]
    assert '*/' in doc and 'DCTFP_ERR_INVALID' in doc and 'key << 32' in doc and 'dctfp_tri_filter_count' in doc
    assert re.fullmatch(r'\s*', doc.split('*/', 1)[1]), 'the comment must sit right above the declaration'
    version = int(re.search(r'#define DCTFP_VERSION (\d+)', header).group(1))
    assert version >= 110                                       # (the parent commit's: 109)
    for path in (_lib.LIB_PATH, _lib.EXPERIMENTS_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert hasattr(lib, name) and lib.dctfp_version() == version
    assert name in _lib.EXPORTS
    assert sorted(_lib.EXPORTS) == sorted(set(re.findall(r'\b(dctfp_\w+)\(', re.sub(r'/\*.*?\*/', '', header, flags=re.S))))
    fn = getattr(_lib._configure(ctypes.CDLL(_lib.LIB_PATH)), name)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(PARAMS.split(','))
    launch = open(os.path.join(ROOT, 'dctdomain_amd', 'csrc', 'launch.h')).read()
    assert 'launch_rect_best(' in launch
    assert name in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


def test_null_arguments_are_refused_by_name_without_a_device():
    from dctdomain_amd import _lib
    lib = _lib._configure(ctypes.CDLL(_lib.LIB_PATH))
    assert lib.dctfp_rect_best(None, None, 1, 1, 1, 0, 0, None, None, 17000, 0, None, 1, None, 1, None) == _lib.DCTFP_ERR_INVALID
    assert b'dctfp_rect_best: NULL argument' in lib.dctfp_last_error()


def test_new_unit_is_part_of_the_build_and_touches_the_arrays_through_atomics_only():
    import build_ext
    assert 'k_best.hip' in build_ext.UNITS
    csrc = os.path.join(ROOT, 'dctdomain_amd', 'csrc')
    text = open(os.path.join(csrc, 'k_best.hip')).read()
    code = '\n'.join(line.split('//', 1)[0] for line in text.splitlines())
    walk = '\n'.join(line.split('//', 1)[0] for line in open(os.path.join(csrc, 'band_walk.hip.h')).read().splitlines())
    # the kernel is exempt from the one band walk by name (the reason is written at it and in profiles/band_walk/README.md): it keeps
    # its loop, over the TriTile, with the walk's constants, grid and key rule; its atomics are lower_hit's, defined in the walk's
    # header alone
    assert '#include "band_walk.hip.h"' in text and 'void lower_hit(' in walk and 'void lower_hit(' not in code
    assert 'EXEMPT from band_walk by name' in text and 'profiles/band_walk/README.md' in text and 'band_walk(' not in code
    assert 'rect_best_kernel' in open(os.path.join(ROOT, 'profiles', 'band_walk', 'README.md')).read()
    assert '__HIP_MEMORY_SCOPE_AGENT' in walk and 'asm' not in code and 'asm' not in walk and '__builtin_amdgcn_sad_u8' not in text + walk
    assert code.count('__ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT') == 0        # (no atomic of its own on the arrays: lower_hit's two)
    assert not re.search(r'#include\s+"(tri_walk|union_find|sad_tile)\.hip\.h"', text) and not re.search(r'#include\s+"[^"]*\.hip"', text)
    kernel = code[code.index('void rect_best_kernel'):code.index('namespace dctfp_host')]
    assert 'void rect_best_kernel(const TriTile t, ' in kernel and not re.search(r'\b(256|1024|64)\b', kernel.replace('& 63', ''))
    assert 'key_of(' in kernel and 'band_grid(t)' in code and 'n_cols +' not in code
    lower = walk[walk.index('void lower_hit'):walk.index('template <class Pass>')]
    # no plain load or store of the two arrays: they are only ever offset and handed to lower_hit
    assert not re.search(r'\bbest_(row|col)\s*\[', code) and not re.search(r'\*\s*\(?\s*best_(row|col)\b', kernel.split(')', 1)[1])
    assert kernel.count('lower_hit(best_row + ') == 1 and kernel.count('lower_hit(best_col + ') == 1
    uses = re.findall(r'[^\n]*\bslot\b[^\n]*', lower.split('{', 1)[1])
    assert len(uses) == 2 and all('__hip_atomic_' in u and '__ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT' in u for u in uses)
    assert '__hip_atomic_fetch_min(slot' in lower
    assert not re.search(r'\bwhile\b|\bfor \(;;\)', kernel + walk)     # (no spin loop)
    # s_row is cleared between two barriers and the flush stands behind a third
    sync = [m.start() for m in re.finditer(r'__syncthreads\(\);', kernel)]
    assert len(sync) == 3 and sync[0] < kernel.index('s_row[tid] = kNone32;') < sync[1] < kernel.index('for (int rl = 0;') < sync[2] < kernel.index('lower_hit(best_row + ')
    host = open(os.path.join(csrc, 'dctfp_sim.hip')).read()
    body = host[host.index('\nint dctfp_rect_best('):host.index('DCTFP_GUARD("dctfp_rect_best")')]
    # (the two range checks in the form that cannot overflow: range_within(first, count, n) is count <= n && first <= n - count)
    for check in ('ld < n_cols', '!range_within(row0, n_rows, n_a)', '!range_within(col0, n_cols, n_b)', '0x7fffffff', 'rect_best_max_cap()',
                  'launch_rect_best(TriTile{'):
        assert check in body, check
    assert 'row0 + n_rows' not in body and 'col0 + n_cols' not in body
    assert 'constexpr bool range_within(int64_t first, int64_t count, int64_t n) { return count <= n && first <= n - count; }' in host


def test_the_wrappers_are_public_and_carry_the_stated_signatures():
    from dctdomain_amd import dct_sim, similarity
    assert list(inspect.signature(similarity.rect_best).parameters) == ['tile', 'row0', 'col0', 'bound', 'state', 'row_empty', 'col_empty', 'cap']
    assert inspect.signature(similarity.rect_best).parameters['cap'].default == 17000
    assert list(inspect.signature(similarity.BestState.__init__).parameters) == ['self', 'n_a', 'n_b', 'device']
    assert similarity.BEST_NONE == -1
    assert dct_sim.rbh_sim.__name__ == 'rbh_sim' and 'ReciprocalBest' in dct_sim.rbh_sim.__doc__
    assert '--rbh' in dct_sim.__doc__ and 'dctfp_rect_best' in dct_sim.__doc__
    assert 'same file' in dct_sim.build_parser().format_help().replace('\n', ' ')
    for name in ('README.md', 'DESIGN.md'):
        assert '--rbh' in open(os.path.join(ROOT, name)).read()
    assert os.path.exists(os.path.join(ROOT, 'profiles', 'rbh', 'README.md'))
