"""CPU-side checks of dct-sim --cluster --linkage greedy: the oracle (greedy_rule.py, the GPU tests' reference) on graphs worked by
hand and on the committed reference golden, the command line, and the three entry points in the libraries and the header."""

import ctypes
import os
import re

import numpy as np
import pytest

import all_sim_filter_rule as rule
import cluster_rule as crule
import golden_util as gu
import greedy_rule as grule
from test_cluster_gpu import CUTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPZ = os.path.join(gu.GOLD, 'all_sim', 'all-dct.npz')


# ---- the oracle on graphs worked by hand

def test_a_path_of_five():
    got = grule.greedy(5, [0, 1, 2, 3], [1, 2, 3, 4])
    assert got.dtype == np.int32 and got.tolist() == [0, 0, 2, 2, 4]
    grule.check(5, [0, 1, 2, 3], [1, 2, 3, 4], got)
    assert crule.components(5, [0, 1, 2, 3], [1, 2, 3, 4]).tolist() == [0] * 5      # (single linkage: one chain, one cluster)


def test_a_star_centred_on_the_last_node():
    """0 represents itself and the centre; the centre is then a member, so no other leaf has an edge to a representative."""
    i, j = [0, 1, 2, 3], [4, 4, 4, 4]
    got = grule.greedy(5, i, j)
    assert got.tolist() == [0, 1, 2, 3, 0]
    grule.check(5, i, j, got)
    assert grule.greedy(5, j, i).tolist() == got.tolist()     # (an edge either way round)


def test_a_triangle_and_an_isolated_node():
    i, j = [0, 0, 1], [1, 2, 2]
    got = grule.greedy(4, i, j)
    assert got.tolist() == [0, 0, 0, 3]
    grule.check(4, i, j, got)


def test_two_representatives_compete_for_one_member_and_the_lower_wins():
    """0 and 1 share no edge, both have one to 2 -- and 3 has one to 1 only."""
    i, j = [1, 0, 1], [2, 2, 3]
    got = grule.greedy(4, i, j)
    assert got.tolist() == [0, 1, 0, 1]
    grule.check(4, i, j, got)


def test_a_later_representative_that_is_lower_than_the_first_one_seen():
    """2 is decided after 4 would be by any scheme that takes 'no earlier neighbour' first (0-1-2 is a path, 4 has no earlier
    neighbour but 3): 5 has edges to 2 and 4, both representatives -- the label is 2."""
    i, j = [0, 1, 2, 4], [1, 2, 5, 5]
    got = grule.greedy(6, i, j)
    assert got.tolist() == [0, 0, 2, 3, 4, 2]
    grule.check(6, i, j, got)


def test_check_refuses_wrong_labels():
    i, j = [0, 1, 2, 3], [1, 2, 3, 4]
    for wrong in ([0, 0, 0, 0, 0], [0, 0, 2, 2, 2], [0, 1, 2, 3, 4], [0, 0, 2, 3, 4], [0, 0, 1, 2, 4]):
        with pytest.raises(AssertionError):
            grule.check(5, i, j, np.array(wrong))


def test_self_pairs_and_no_edges():
    assert grule.greedy(3, [1, 2], [1, 2]).tolist() == [0, 1, 2]
    assert grule.greedy(0, [], []).tolist() == []


# ---- the oracle on the reference's 139 proteins

@pytest.fixture(scope='module')
def golden():
    with np.load(NPZ) as data:
        sid, idx, dct = [str(s) for s in data['sid']], np.asarray(data['idx'], dtype=np.int64), data['dct']
    return sid, idx, dct, rule.triangle_l1(dct, idx)


def _both(golden, kw):
    _, idx, _, (i, j, mn, last) = golden
    keep = rule.kept(mn, last, **kw)
    n = len(idx) - 1
    return n, i[keep], j[keep], grule.greedy(n, i[keep], j[keep]), crule.components(n, i[keep], j[keep])


@pytest.mark.parametrize('kw', CUTS, ids=lambda kw: ','.join(f'{k[4:]}={v}' for k, v in kw.items()))
def test_oracle_on_the_reference_golden(golden, kw):
    n, i, j, greedy, single = _both(golden, kw)
    grule.check(n, i, j, greedy)
    # greedy clusters refine single linkage's: a member and its representative share an edge
    assert np.array_equal(single[greedy], single)
    assert len(np.unique(greedy)) >= len(np.unique(single))
    assert np.array_equal(greedy, grule.labels(golden[2], golden[1], **kw)[0])


def test_greedy_differs_from_single_linkage_on_the_golden(golden):
    differing = [kw for kw in CUTS if not np.array_equal(*_both(golden, kw)[3:])]
    assert differing, 'no cut-off of the list tells the two linkages apart'
    n, i, j, greedy, single = _both(golden, {'min_domain': 0.5})
    assert {'min_domain': 0.5} in differing and len(np.unique(greedy)) > len(np.unique(single)) == 22


# ---- the command line

def test_parser_takes_linkage_with_cluster():
    from dctdomain_amd import dct_sim
    for value in ('single', 'greedy'):
        args = dct_sim.build_parser().parse_args(['--dct', 'x.npz', '--cluster', '--min-domain', '0.5', '--linkage', value])
        assert args.cluster is True and args.linkage == value
    assert dct_sim.LINKAGES == ('single', 'greedy')


@pytest.mark.parametrize('argv,said', [
    (['--linkage', 'greedy'], '--linkage says how --cluster forms its clusters'),
    (['--linkage', 'single', '--min-domain', '0.5'], '--linkage says how --cluster forms its clusters'),
    (['--linkage', 'greedy', '--db', 'd.npz'], '--linkage says how --cluster forms its clusters'),
    (['--cluster', '--linkage', 'greedy'], '--cluster needs a cut-off'),
    (['--cluster', '--min-domain', '0.5', '--linkage', 'complete'], 'invalid choice'),
    (['--cluster', '--min-domain', '0.5', '--linkage'], 'expected one argument'),
])
def test_parser_rejects(argv, said, capsys):
    from dctdomain_amd import dct_sim
    with pytest.raises(SystemExit) as e:
        dct_sim.build_parser().parse_args(['--dct', 'x.npz'] + argv)
    assert e.value.code == 2
    assert said in capsys.readouterr().err


def test_cluster_without_linkage_parses_to_what_it_parsed_to():
    from dctdomain_amd import dct_sim
    args = vars(dct_sim.build_parser().parse_args(['--dct', 'x.npz', '--cluster', '--min-global', '0.25', '--output', 'o']))
    assert args == dict(dct='x.npz', output='o', pair=None, pairfound=None, db=None, top=5, threshold=0.25, rank=None, min_domain=None,
                        min_global=0.25, cluster=True)
    assert 'linkage' not in vars(dct_sim.build_parser().parse_args(['--dct', 'x.npz']))


def test_cluster_sim_takes_the_linkage_and_refuses_an_unknown_one(tmp_path):
    from dctdomain_amd import dct_sim
    with pytest.raises(ValueError):
        dct_sim.cluster_sim(NPZ, str(tmp_path / 'out.txt'), min_domain=0.5, linkage='complete')
    with pytest.raises(ValueError):
        dct_sim.cluster_sim(NPZ, str(tmp_path / 'out.txt'), linkage='greedy')


@pytest.mark.parametrize('n', [0, 1])
def test_no_protein_and_one_protein_need_no_device(tmp_path, n):
    from dctdomain_amd import dct_sim
    sid = ['only'][:n]
    idx = np.arange(n + 1, dtype=np.int64)
    fps = np.zeros((n, 480), dtype=np.int8)
    r = dct_sim.Representatives(sid, idx, fps, min_domain=0.5)
    labels = r.labels()
    assert labels.dtype == np.int32 and labels.tolist() == list(range(n)) and r.rounds == 0
    path, out = str(tmp_path / 'x-dct.npz'), str(tmp_path / 'out.txt')
    np.savez(path, sid=np.array(sid, dtype='<U4'), idx=idx, dom=np.array(['1-9'] * n, dtype='<U3'), dct=fps)
    dct_sim.main(['--dct', path, '--output', out, '--cluster', '--linkage', 'greedy', '--min-global', '0.9'])
    assert open(out, 'rb').read() == grule.HEADER + b'only only\n' * n


def test_degenerate_cut_offs_need_no_tile(golden):
    from dctdomain_amd import dct_sim
    sid, idx, dct, _ = golden
    for kw in ({'min_domain': 1.0001}, {'min_global': 1.5}, {'min_domain': 0.5, 'min_global': 1.0001}):
        assert np.array_equal(dct_sim.Representatives(sid, idx, dct, **kw).labels(), np.arange(139))
        assert np.array_equal(grule.labels(dct, idx, **kw)[0], np.arange(139))
    for kw in ({'min_domain': 0.0}, {'min_global': -1.0}, {'min_domain': float('nan'), 'min_global': 0.0}):
        assert not dct_sim.Representatives(sid, idx, dct, **kw).labels().any()
        assert not grule.labels(dct, idx, **kw)[0].any()


def test_representatives_share_the_stripes_routes_and_bounds_of_the_filtered_pairs():
    from dctdomain_amd import dct_sim
    r = dct_sim.Representatives(['a', 'b'], [0, 1, 2], np.zeros((2, 480), np.int8), min_domain=0.5, min_global=0.25)
    assert (r.bound_domain, r.bound_global, r.route, r.rounds) == (8500, 12750, 'global', 0)
    for name in ('stripes', 'tiles', 'chunks'):
        assert getattr(dct_sim.Representatives, name) is getattr(dct_sim.FilteredPairs, name)


# ---- the library

DECLARED = [
    ('dctfp_greedy_decide', 'dctfp_ctx* ctx, int32_t* assign, int32_t* state, const int32_t* blocked, int64_t n_nodes, int64_t i0, int64_t i1, '
                            'int32_t round, int64_t* undecided, void* stream', 10),
    ('dctfp_greedy_tri_mark', 'dctfp_ctx* ctx, const int32_t* tile, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row0, int64_t col0, '
                              'const uint8_t* row_empty, const uint8_t* col_empty, int32_t cap, int32_t bound, int32_t* assign, '
                              'const int32_t* state, int32_t* blocked, int64_t n_nodes, int64_t range_end, int32_t next_round, void* stream', 18),
    ('dctfp_greedy_pairs_mark', 'dctfp_ctx* ctx, const int32_t* pi, const int32_t* pj, int64_t n_pairs, int32_t* assign, const int32_t* state, '
                                'int32_t* blocked, int64_t n_nodes, int64_t range_end, int32_t next_round, void* stream', 11),
]


@pytest.mark.parametrize('name,params,n_args', DECLARED)
def test_library_exports_the_entry_points_and_header_documents_them(name, params, n_args):
    from dctdomain_amd import _lib
    with open(os.path.join(ROOT, 'include', 'dctfp.h')) as fh:
        header = fh.read()
    decl = re.search(r'int %s\(([^;]*)\);' % name, header)
    assert decl and ' '.join(decl.group(1).split()) == params
    assert len(params.split(',')) == n_args
    doc = header[:decl.start()].rsplit('/*', 1)[1]
    assert '*/' in doc and 'DCTFP_ERR_LIMIT' in doc
    assert re.fullmatch(r'\s*', doc.split('*/', 1)[1]), 'the comment must sit right above the declaration'
    version = int(re.search(r'#define DCTFP_VERSION (\d+)', header).group(1))
    assert version >= 106
    for path in (_lib.LIB_PATH, _lib.EXPERIMENTS_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert hasattr(lib, name)
        assert lib.dctfp_version() == version
    assert name in _lib.EXPORTS
    fn = getattr(_lib._configure(ctypes.CDLL(_lib.LIB_PATH)), name)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == n_args
    with open(os.path.join(ROOT, 'dctdomain_amd', 'csrc', 'launch.h')) as fh:
        assert 'launch_' + name[len('dctfp_'):] + '(' in fh.read()


def test_a_null_context_is_refused_without_a_device():
    from dctdomain_amd import _lib
    lib = _lib._configure(ctypes.CDLL(_lib.LIB_PATH))
    assert lib.dctfp_greedy_decide(None, None, None, None, 5, 0, 5, 1, None, None) == _lib.DCTFP_ERR_INVALID
    assert lib.dctfp_greedy_tri_mark(None, None, 1, 1, 1, 0, 0, None, None, 17000, 0, None, None, None, 5, 1, 1, None) == _lib.DCTFP_ERR_INVALID
    assert lib.dctfp_greedy_pairs_mark(None, None, None, 0, None, None, None, 5, 5, 1, None) == _lib.DCTFP_ERR_INVALID
    assert b'NULL argument' in lib.dctfp_last_error()


def test_new_unit_is_part_of_the_build_and_shares_the_row_walk():
    import build_ext
    assert 'k_greedy.hip' in build_ext.UNITS
    text = open(os.path.join(ROOT, 'dctdomain_amd', 'csrc', 'k_greedy.hip')).read()
    assert '#include "tri_walk.hip.h"' in text and 'filter_quad(' in text and not re.search(r'\bQuad filter_quad\(', text)
