"""CPU-side checks of dct-sim --db --rank: the command line, and dctfp_protein_min in the library and its header."""

import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('rank', ['global', 'domain'])
def test_parser_accepts_rank_with_db(rank):
    from dctdomain_amd import dct_sim
    args = dct_sim.build_parser().parse_args(['--dct', 'q.npz', '--db', 'd.npz', '--rank', rank])
    assert args.rank == rank and args.db == 'd.npz'


def test_parser_default_rank_is_global_search():
    from dctdomain_amd import dct_sim
    args = dct_sim.build_parser().parse_args(['--dct', 'q.npz', '--db', 'd.npz'])
    assert (args.rank or 'global') == 'global'


@pytest.mark.parametrize('argv', [
    ['--dct', 'q.npz', '--db', 'd.npz', '--rank', 'best'],              # not a mode
    ['--dct', 'q.npz', '--db', 'd.npz', '--rank', 'Domain'],
    ['--dct', 'q.npz', '--pair', 'p.txt', '--rank', 'domain'],          # pair scoring ranks nothing
    ['--dct', 'q.npz', '--pair', 'p.txt', '--db', 'd.npz', '--rank', 'global'],
    ['--dct', 'q.npz', '--rank', 'domain'],                             # all-against-all ranks nothing
])
def test_parser_rejects(argv, capsys):
    from dctdomain_amd import dct_sim
    with pytest.raises(SystemExit) as e:
        dct_sim.build_parser().parse_args(argv)
    assert e.value.code == 2
    assert '--rank' in capsys.readouterr().err


def test_search_rejects_an_unknown_rank():
    import numpy as np
    from dctdomain_amd import dct_sim
    search = dct_sim.ProteinSearch(np.zeros((1, 480), np.int8), [0, 1])
    with pytest.raises(ValueError):
        search.search(np.zeros((1, 480), np.int8), [0, 1], 5, 0.25, rank='local')


def test_library_exports_protein_min_and_header_documents_it():
    from dctdomain_amd import _lib
    with open(os.path.join(ROOT, 'include', 'dctfp.h')) as fh:
        header = fh.read()
    decl = re.search(r'/\*((?:(?!\*/).)*)\*/\s*int dctfp_protein_min\(([^;]*)\);', header, re.S)
    assert decl, 'dctfp_protein_min is not declared with a comment in include/dctfp.h'
    doc, params = decl.group(1), ' '.join(decl.group(2).split())
    assert params == ('dctfp_ctx* ctx, const int8_t* a, int64_t lda, const int64_t* idx_a, int64_t npa, const int8_t* b, '
                      'int64_t ldb, const int64_t* idx_b, int64_t npb, int32_t d, int32_t* out, int64_t ldo, void* stream')
    for word in ('0x7fffffff', 'DCTFP_ERR_LIMIT', '512', 'dctfp_block_min'):
        assert word in doc
    version = int(re.search(r'#define DCTFP_VERSION (\d+)', header).group(1))
    assert version >= 102
    for path in (_lib.LIB_PATH, _lib.EXPERIMENTS_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert hasattr(lib, 'dctfp_protein_min')
        assert lib.dctfp_version() == version
    assert 'dctfp_protein_min' in _lib.EXPORTS
