"""CPU-side checks of dct-sim's all-against-all cut-offs: the command line, the three entry points in the libraries and the
header, and the numpy rule (all_sim_filter_rule.py, the GPU tests' oracle) pinned on the committed reference golden."""

import ctypes
import os
import re

import numpy as np
import pytest

import all_sim_filter_rule as rule
import golden_util as gu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(gu.GOLD, 'all_sim')


@pytest.mark.parametrize('argv,want', [
    (['--min-domain', '0.5'], (0.5, None)),
    (['--min-global', '0.25'], (None, 0.25)),
    (['--min-domain', '0.1', '--min-global', '1'], (0.1, 1.0)),
    (['--min-domain', '-1', '--threshold', '0.9', '--top', '3'], (-1.0, None)),
])
def test_parser_accepts_the_cut_offs_in_all_against_all_mode(argv, want):
    from dctdomain_amd import dct_sim
    args = dct_sim.build_parser().parse_args(['--dct', 'x.npz'] + argv)
    assert (args.min_domain, args.min_global) == want and not args.pair and not args.db


def test_parser_takes_nan_and_defaults_to_no_cut_off():
    from dctdomain_amd import dct_sim
    args = dct_sim.build_parser().parse_args(['--dct', 'x.npz', '--min-global', 'nan'])
    assert np.isnan(args.min_global) and args.min_domain is None
    args = dct_sim.build_parser().parse_args(['--dct', 'x.npz'])
    assert args.min_domain is None and args.min_global is None


@pytest.mark.parametrize('argv,named', [
    (['--pair', 'p.txt', '--min-domain', '0.5'], '--min-domain'),
    (['--pair', 'p.txt', '--min-global', '0.5'], '--min-global'),
    (['--db', 'd.npz', '--min-domain', '0.5'], '--min-domain'),
    (['--db', 'd.npz', '--rank', 'domain', '--min-global', '0.5'], '--min-global'),
    (['--pair', 'p.txt', '--db', 'd.npz', '--min-global', '0.5'], '--min-global'),
    (['--min-domain', 'half'], '--min-domain'),
    (['--min-global', ''], '--min-global'),
])
def test_parser_rejects(argv, named, capsys):
    from dctdomain_amd import dct_sim
    with pytest.raises(SystemExit) as e:
        dct_sim.build_parser().parse_args(['--dct', 'x.npz'] + argv)
    assert e.value.code == 2
    assert named in capsys.readouterr().err


def test_all_sim_takes_the_cut_offs_as_keywords():
    import inspect
    from dctdomain_amd import dct_sim
    assert {'sid', 'idx', 'fps', 'min_domain', 'min_global'} <= set(inspect.signature(dct_sim.FilteredPairs.__init__).parameters)
    f = dct_sim.FilteredPairs(['a', 'b'], [0, 1, 2], np.zeros((2, 480), np.int8), min_domain=0.5)
    assert (f.bound_domain, f.bound_global, f.route) == (8500, 17000, 'domain')
    f = dct_sim.FilteredPairs(['a', 'b'], [0, 1, 2], np.zeros((2, 480), np.int8), min_domain=0.5, min_global=0.25)
    assert (f.bound_domain, f.bound_global, f.route) == (8500, 12750, 'global')
    f = dct_sim.FilteredPairs(['a', 'b'], [0, 1, 2], np.zeros((2, 480), np.int8), min_domain=1.0001, min_global=float('nan'))
    assert (f.bound_domain, f.bound_global, f.route) == (-1, 17000, 'domain')


def test_stripes_cover_the_rows_within_the_tile():
    from dctdomain_amd import dct_sim
    rng = np.random.default_rng(0)
    idx = np.concatenate([[0], np.cumsum(rng.integers(0, 9, size=500))])

    class Small(dct_sim.FilteredPairs):
        TILE_INTS = 3000
        COL_ROWS = 40
    f = Small(['x'] * 500, idx, np.zeros((int(idx[-1]), 480), np.int8), min_domain=0.5)
    stripes = list(f.stripes())
    assert stripes[0][0] == 0 and stripes[-1][1] == 499 and all(a[1] == b[0] for a, b in zip(stripes, stripes[1:]))
    for i0, i1 in stripes:
        assert i1 > i0
        if i1 - i0 > 1:
            assert (i1 - i0) * (500 - 1 - i0) <= 3000 and idx[i1] - idx[i0] <= 40


@pytest.mark.parametrize('name,params', [
    ('dctfp_tri_filter_count', 'dctfp_ctx* ctx, const int32_t* tile, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row0, int64_t col0, '
                               'const uint8_t* row_empty, const uint8_t* col_empty, int32_t cap, int32_t bound, int32_t* out_count, void* stream'),
    ('dctfp_tri_filter_fill', 'dctfp_ctx* ctx, const int32_t* tile, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row0, int64_t col0, '
                              'const uint8_t* row_empty, const uint8_t* col_empty, int32_t cap, int32_t bound, const int64_t* offsets, '
                              'int64_t out_len, int32_t* out_i, int32_t* out_j, void* stream'),
    ('dctfp_pair_lines', 'dctfp_ctx* ctx, int64_t n_lines, const int32_t* pi, const int32_t* pj, const int32_t* mn, const int32_t* last, '
                         'const uint8_t* ids, const int64_t* id_off, int64_t n_ids, const char* table, const int64_t* line_off, uint8_t* out, '
                         'int64_t out_bytes, void* stream'),
])
def test_library_exports_the_entry_points_and_header_documents_them(name, params):
    from dctdomain_amd import _lib
    with open(os.path.join(ROOT, 'include', 'dctfp.h')) as fh:
        header = fh.read()
    decl = re.search(r'int %s\(([^;]*)\);' % name, header)
    assert decl and ' '.join(decl.group(1).split()) == params
    # the comment above the declaration (the two filter calls share one) says what the call extends and names its error code
    doc = header[:decl.start()].rsplit('/*', 1)[1]
    assert '*/' in doc and 'DCTFP_ERR_LIMIT' in doc and ('dctfp_select_count' in doc or 'dctfp_sim_lines' in doc)
    if name != 'dctfp_tri_filter_fill':
        assert re.fullmatch(r'\s*', doc.split('*/', 1)[1]), 'the comment must sit right above the declaration'
    version = int(re.search(r'#define DCTFP_VERSION (\d+)', header).group(1))
    assert version >= 103
    for path in (_lib.LIB_PATH, _lib.EXPERIMENTS_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert hasattr(lib, name)
        assert lib.dctfp_version() == version
    assert name in _lib.EXPORTS


def test_new_unit_is_part_of_the_build():
    import build_ext
    assert 'k_filter.hip' in build_ext.UNITS
    assert os.path.exists(os.path.join(ROOT, 'dctdomain_amd', 'csrc', 'k_filter.hip'))


# ---- the rule on the reference's own output: 139 proteins, 9 591 pairs, none of them empty

@pytest.fixture(scope='module')
def golden():
    with np.load(os.path.join(GOLD, 'all-dct.npz')) as data:
        idx, dct = np.asarray(data['idx'], dtype=np.int64), data['dct']
    assert len(idx) - 1 == 139 and (np.diff(idx) > 0).all()
    lines = rule.read_lines(os.path.join(GOLD, 'expected.txt.gz'))
    i, j, mn, last = rule.triangle_l1(dct, idx)
    assert len(lines) == 1 + len(i) == 1 + 9591
    return lines, mn, last


CUTS = (0.1, 0.25, 0.5, 0.9, 1.0)
KEPT_DOMAIN = (7237, 4087, 973, 52, 10)
KEPT_GLOBAL = (7131, 3329, 962, 45, 4)


def test_rule_counts_on_the_reference_golden(golden):
    _, mn, last = golden
    assert tuple(int(rule.kept(mn, last, min_domain=x).sum()) for x in CUTS) == KEPT_DOMAIN
    assert tuple(int(rule.kept(mn, last, min_global=y).sum()) for y in CUTS) == KEPT_GLOBAL
    assert (mn <= last).all()                                   # DCTdomain is never below DCTglobal
    for x in (0, -1, float('nan')):
        assert rule.kept(mn, last, min_domain=x, min_global=x).all()
    assert not rule.kept(mn, last, min_domain=1.0001).any() and not rule.kept(mn, last, min_global=1.0001).any()


def test_rule_agrees_with_the_printed_scores_and_with_sim_bound(golden):
    from dctdomain_amd import dct_sim
    lines, mn, last = golden
    # the golden's own text: a kept line never prints a score whose three decimals lie below the cut-off by more than rounding
    for x in CUTS:
        keep = rule.kept(mn, last, min_domain=x, min_global=x)
        text = rule.filtered_text(lines, keep).split(b'\n')[:-1]
        assert text[0] == dct_sim.HEADER.encode() and len(text) == 1 + int(keep.sum())
        for line in text[1:]:
            a, b = (float(v) for v in line.split()[2:4])
            assert a >= x - 0.0005 and b >= x - 0.0005
        # the integer form the device uses: min(L1, 17000) <= sim_bound
        bound = dct_sim.sim_bound(x)
        assert np.array_equal(keep, (np.minimum(mn, 17000) <= bound) & (np.minimum(last, 17000) <= bound))
