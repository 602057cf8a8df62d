"""dct-sim --db --zscore without a GPU: the rule of zscore_rule.py pinned on cases worked by hand, dct_sim's two helpers against it, the
parser's new messages, and what the export and its kernel unit promise, read off the sources."""

import contextlib
import io
import math
import os
import re

import numpy as np

import rbh_rule as rrule
import zscore_rule as zr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G6PD = os.path.join(rrule.gu.GOLD, 'ref_fixtures', 'G6PD-dct.npz')


# ---- 1. the rule

def test_the_rule_on_cases_worked_by_hand():
    # one protein to compare with: no spread to measure against
    assert zr.moments([5]) == (1, 5, 25) and zr.zscore(1, 5, 25, 5) is None and zr.text(None) == '-'
    # all at one distance: the radicand 3 * 147 - 21^2 is 0
    assert zr.moments([7, 7, 7]) == (3, 21, 147) and zr.zscore(3, 21, 147, 7) is None and zr.zscore(3, 21, 147, 0) is None
    # 1, 2, 6: n = 3, S1 = 9, S2 = 41, radicand 3 * 41 - 81 = 42; d = 1: 6 / sqrt(42), d = 6: -9 / sqrt(42), d = 3 (the mean): 0
    assert zr.moments([1, 2, 6]) == (3, 9, 41)
    assert zr.zscore(3, 9, 41, 1) == 6 / math.sqrt(42) and zr.text(zr.zscore(3, 9, 41, 1)) == '0.93'
    assert zr.zscore(3, 9, 41, 6) == -9 / math.sqrt(42) and zr.text(zr.zscore(3, 9, 41, 6)) == '-1.39'
    assert zr.zscore(3, 9, 41, 3) == 0.0 and zr.text(0.0) == '0.00'
    # a protein without fingerprints is no part of the background, and a hit on it has no z
    assert zr.moments([1, zr.NONE, 2, 6, zr.NONE]) == (3, 9, 41)
    assert zr.zscore(3, 9, 41, zr.NONE) is None and zr.zscore(3, 9, 41, None) is None
    # L1s above 17000 count raw: 20000 and 30000 are one sigma = 5000 either side of 25000 (capped, both would be 17000: no z)
    n, s1, s2 = zr.moments([20000, 30000])
    assert (n, s1, s2) == (2, 50000, 1_300_000_000)
    assert zr.zscore(n, s1, s2, 20000) == 1.0 and zr.zscore(n, s1, s2, 30000) == -1.0 and zr.zscore(*zr.moments([17000, 17000]), 17000) is None
    # S2 above 2^63, exact in Python integers: 10^9 proteins, half at 100000 and half at 122400 -- mean 111200, sigma 11200
    n = 10 ** 9
    s1, s2 = n // 2 * (100000 + 122400), n // 2 * (100000 ** 2 + 122400 ** 2)
    assert 1 << 63 < s2 < 1 << 64 and n * s2 - s1 * s1 == (n * 11200) ** 2
    assert zr.zscore(n, s1, s2, 100000) == 1.0 and zr.zscore(n, s1, s2, 122400) == -1.0 and zr.zscore(n, s1, s2, 111200) == 0.0
    assert zr.text(zr.zscore(n, s1, s2, 0)) == '9.93'                    # 111200 / 11200
    # a hair below the mean prints as -0.00: 0 and 2001, d = 1001 -- -1 / 2001
    assert zr.zscore(2, 2001, 2001 ** 2, 1001) == -1 / 2001 and zr.text(-1 / 2001) == '-0.00'


def test_tile_moments_counts_what_the_kernel_counts():
    t = np.array([[3, 5, -1], [4, 0x7fffffff, 6]], dtype=np.int32)
    row, col = zr.tile_moments(t, 1, 2, 4, 6, limit=6)
    assert row.tolist() == [[0, 2, 1, 0], [0, 8, 4, 0], [0, 34, 16, 0]]          # (6 = the limit is out, like -1 and 0x7fffffff)
    assert col.tolist() == [[0, 0, 2, 1, 0, 0], [0, 0, 7, 5, 0, 0], [0, 0, 25, 25, 0, 0]]
    row, col = zr.tile_moments(t, 0, 0, 2, 3, limit=7, row_empty=[0, 0], col_empty=[1, 0, 0])
    assert row.tolist() == [[1, 1], [5, 6], [25, 36]] and col.tolist() == [[0, 1, 1], [0, 5, 6], [0, 25, 36]]


# ---- 2. dct_sim's helpers

def test_zscore_of_and_zscore_text_are_the_rule():
    from dctdomain_amd import dct_sim
    with np.load(G6PD) as data:
        idx, dct = np.asarray(data['idx'], dtype=np.int64), data['dct']
    l1 = {score: rrule.protein_l1(dct, idx, dct, idx, score) for score in ('domain', 'global')}
    # the figures of the issue: 27 proteins of one family against themselves by DCTglobal
    rows, cols = zr.backgrounds(l1['global'])
    assert rows == cols and all(n == 27 for n, _, _ in rows)
    self_z = [zr.zscore(*rows[q], 0) for q in range(27)]
    # (low for hits on oneself, because the database IS the family: z is relative to the database searched)
    assert zr.text(min(self_z)) == '2.22' and zr.text(max(self_z)) == '4.66' and zr.text(float(np.median(self_z))) == '2.47'
    assert np.allclose(self_z, l1['global'].mean(axis=1) / l1['global'].std(axis=1), rtol=1e-12)
    rng = np.random.default_rng(3)
    seen = set()
    for trial in range(10_000):
        row = l1['domain' if trial % 2 else 'global'][int(rng.integers(0, 27))]
        kind = int(rng.integers(0, 10))
        if kind == 0:
            vec = row[:int(rng.integers(0, 2))]                                   # n = 0 or 1
        elif kind == 1:
            vec = np.full(int(rng.integers(2, 9)), row[int(rng.integers(0, 27))])  # all at one distance
        elif kind == 2:
            vec = row[rng.random(27) < 0.5] * int(rng.integers(1, 8))             # far above 17000, raw
        else:
            vec = row[rng.random(27) < 0.7]
        n, s1, s2 = zr.moments(vec)
        d = None if kind == 3 and trial % 3 == 0 else int(rng.integers(0, 20000)) if trial % 5 == 0 or n == 0 else int(vec[int(rng.integers(0, n))])
        want = zr.zscore(n, s1, s2, d)
        got = dct_sim.zscore_of(np.int64(n), np.int64(s1), s2, d)
        assert got == want and type(got) is type(want), (n, s1, s2, d)
        assert dct_sim.zscore_text(got) == zr.text(want)
        seen.add('-' if want is None else 'neg' if want < 0 else 'pos')
    assert seen == {'-', 'neg', 'pos'}
    assert dct_sim.zscore_text(dct_sim.zscore_of(2, 2001, 2001 ** 2, 1001)) == '-0.00'
    assert dct_sim.zscore_text(None) == '-' and dct_sim.zscore_text(float('nan')) == '-' and dct_sim.zscore_text(1.005) == f'{1.005:.2f}'
    n = 10 ** 9
    assert dct_sim.zscore_of(n, n // 2 * 222400, n // 2 * (100000 ** 2 + 122400 ** 2), 100000) == 1.0
    # the words as the device holds them: a sum of squares of 2^63 or more shows negative in int64 and is read back unsigned
    mom = np.array([[n, 2], [n // 2 * 222400, 9], [n // 2 * (100000 ** 2 + 122400 ** 2), 41]], dtype=np.uint64).view(np.int64)
    assert mom[2, 0] < 0
    assert dct_sim._moment_ints(mom) == [(n, n // 2 * 222400, n // 2 * (100000 ** 2 + 122400 ** 2)), (2, 9, 41)]
    assert dct_sim.zscores_of(mom, [0, 0, 1], [100000, 122400, 1]).tolist() == [1.0, -1.0, zr.zscore(2, 9, 41, 1)]


def test_zscores_of_is_zscore_of_to_the_bit():
    """The vector form the searches use: the same floats as the rule for every hit, NaN where the rule has None."""
    from dctdomain_amd import dct_sim
    rng = np.random.default_rng(17)
    backgrounds = [[], [5], [7, 7, 7], [1, 2, 6], [0, 2001], [20000, 30000], [17000, 17000]]
    backgrounds += [rng.integers(0, 122401, size=int(rng.integers(2, 400))).tolist() for _ in range(60)]
    backgrounds += [(rng.integers(15000, 16000, size=1000) * int(rng.integers(1, 100))).tolist() for _ in range(10)]
    words = [zr.moments(b) for b in backgrounds]
    big = 2 ** 31 - 1                                                    # (as many proteins as the library takes, all near L1 1000)
    words.append((big, big * 1000 + 12345, big * 10 ** 6 + 12345 * 3000))
    mom = np.array(words, dtype=np.uint64).T.view(np.int64)
    owner = rng.integers(0, len(words), size=20_000)
    d = rng.integers(0, 130_000, size=20_000)
    d[::7] = 0x7fffffff
    owner[-50:], d[-50:] = len(words) - 1, rng.integers(2 ** 23, 2 ** 24, size=50)   # numerators beyond 2^53: exact in int64, rounded once
    has = d != 0x7fffffff
    got = dct_sim.zscores_of(mom, owner, d, has)
    want = [zr.zscore(*words[o], v) for o, v in zip(owner.tolist(), d.tolist())]
    assert got.dtype == np.float64 and [None if v != v else v for v in got.tolist()] == want
    assert sum(v is None for v in want) > 3000 and sum(v is not None for v in want) > 10_000
    assert all(abs(words[-1][1] - big * int(v)) > 2 ** 53 for v in d[-50:]) and all(v is not None for v in want[-50:])
    # without the mask every pair is taken to have an L1; no hit at all: an empty array
    assert np.array_equal(dct_sim.zscores_of(mom, owner[has], d[has]), got[has], equal_nan=True)
    assert dct_sim.zscores_of(mom, [], []).shape == (0,)


# ---- 3. the parser

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


Z_DOES = '--zscore places every hit of a database search in the background of its query: '
MIN_Z_DOES = '--min-z cuts the hits of a database search by their z-score: '


def test_the_parser_takes_the_two_options_with_db_alone():
    plain = _parse(['--db', 'y'])
    assert 'zscore' not in plain and 'min_z' not in plain
    assert _parse(['--db', 'y', '--zscore']) == dict(plain, zscore=True)
    assert _parse(['--db', 'y', '--min-z', '1.5']) == dict(plain, min_z=1.5)
    assert _parse(['--db', 'y', '--min-z', '-2', '--zscore', '--rank', 'domain']) == dict(plain, min_z=-2.0, zscore=True, rank='domain')
    rbh = _parse(['--db', 'y', '--rbh', 'global'])
    assert 'zscore' not in rbh and _parse(['--db', 'y', '--rbh', 'global', '--zscore', '--min-z', '0']) == dict(rbh, zscore=True, min_z=0.0)
    assert _parse(['--db', 'y', '--domains', '--zscore'])['domains'] is True
    for flag, does in ((['--zscore'], Z_DOES), (['--min-z', '2'], MIN_Z_DOES)):
        assert _parse(flag) == does + 'it needs --db'
        assert _parse(flag + ['--min-domain', '0.5']) == does + 'it needs --db'
        assert _parse(flag + ['--pair', 'p']) == does + 'not with --pair'
        assert _parse(flag + ['--pair', 'p', '--db', 'y']) == does + 'not with --pair'
        assert _parse(flag + ['--cluster', '--min-domain', '0.5']) == does + 'not with --cluster'
        name = flag[0]
        assert _parse(flag + ['--tree']) == f'--tree prints the single-linkage tree of --dct: not with {name}'
        assert _parse(flag + ['--assign', 'r', '--min-domain', '0.5']) == f'--assign places the proteins of --dct on a fixed set of representatives: not with {name}'
        assert _parse(flag + ['--auc1', '--family-sep', '|']) == f'--auc1 measures the AUC1 and the top-1 rates of --dct: not with {name}'
        assert _parse(flag + ['--hist']) == f'--hist bins the scores of all pairs of --dct: not with {name}'
        assert _parse(flag + ['--rbh']) == '--rbh compares the proteins of --dct with those of another file: it needs --db'
    assert _parse(['--zscore', '--min-z', '1', '--tree']) == '--tree prints the single-linkage tree of --dct: not with --zscore'
    assert 'invalid float value' in _parse(['--db', 'y', '--min-z', 'high'])


def test_the_help_says_what_z_is_relative_to():
    from dctdomain_amd import dct_sim
    text = re.sub(r'\s+', ' ', dct_sim.build_parser().format_help())
    assert 'z is relative to the database searched' in text and 'counts in its own background like any other protein' in text
    assert '--zscore' in text and '--min-z Z' in text
    # --zscore is given when it is there, --min-z whatever its Z (0 too)
    assert _parse(['--tree', '--zscore']).endswith(': not with --zscore') and _parse(['--tree', '--min-z', '0']).endswith(': not with --min-z')
    # the four modes name --min-neighbors, --zscore and --min-z in that order
    for mode in (['--tree'], ['--assign', 'r', '--min-domain', '0.5'], ['--auc1', '--family-sep', '|'], ['--hist']):
        assert _parse(mode + ['--min-z', '2', '--zscore', '--min-neighbors', '3']).endswith(': not with --min-neighbors')
        assert _parse(mode + ['--min-z', '2', '--zscore']).endswith(': not with --zscore')
        assert _parse(mode + ['--min-z', '2']).endswith(': not with --min-z')
    assert _parse(['--db', 'y', '--rbh', '--zscore'])['zscore'] is True
    assert dct_sim._z_header(False) == '' and dct_sim._z_header(True) == ' z-global' and dct_sim._z_header(True, rank='domain') == ' z-domain'
    assert dct_sim._z_header(True, True, 'domain') == ' z-query z-db'


# ---- 4. the build

def test_the_export_is_declared_bound_and_built():
    import ctypes

    import build_ext
    from dctdomain_amd import _lib, similarity
    with open(os.path.join(ROOT, 'include', 'dctfp.h')) as fh:
        header = fh.read()
    assert int(re.search(r'#define DCTFP_VERSION (\d+)', header).group(1)) >= 116
    name = 'dctfp_rect_moments'
    decl = re.search(r'\nint %s\(([^;]*)\);' % name, header)
    assert decl and decl.group(1).count(',') == 16 - 1               # ctx, the ten tile values, row_mom, n_a, col_mom, n_b, stream
    assert 'uint64_t* row_mom, int64_t n_a, uint64_t* col_mom, int64_t n_b, void* stream' in re.sub(r'\s+', ' ', decl.group(1))
    assert name in _lib.EXPORTS
    for path in (_lib.LIB_PATH, _lib.EXPERIMENTS_LIB_PATH):
        assert hasattr(ctypes.CDLL(path), name)
    fn = getattr(_lib._configure(ctypes.CDLL(_lib.LIB_PATH)), name)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 16 and fn.argtypes[:11] == _lib._TRI_TILE
    with open(os.path.join(ROOT, 'dctdomain_amd', 'csrc', 'launch.h')) as fh:
        assert 'void launch_rect_moments(const TriTile& t, ' in fh.read()
    with open(os.path.join(ROOT, 'INTEGRATION.md')) as fh:
        assert name in fh.read()
    assert ctypes.CDLL(_lib.LIB_PATH).dctfp_version() >= 116
    assert callable(similarity.rect_moments) and callable(similarity.MomentState)
    assert 'k_moments.hip' in build_ext.UNITS and 'k_moments.hip' not in build_ext.TWIN_UNITS
    # the refusals that need no device: a NULL context, and the message carries the export's name
    lib = _lib.load()
    assert lib.dctfp_rect_moments(None, None, 1, 1, 1, 0, 0, None, None, 17000, 17000, None, 1, None, 1, None) == _lib.DCTFP_ERR_INVALID
    assert b'dctfp_rect_moments: NULL argument' in lib.dctfp_last_error()


def _code(path):
    with open(path) as fh:
        return '\n'.join(line.split('//', 1)[0] for line in fh.read().splitlines())


def test_the_unit_touches_the_arrays_through_agent_scope_atomics_alone():
    csrc = os.path.join(ROOT, 'dctdomain_amd', 'csrc')
    unit = _code(os.path.join(csrc, 'k_moments.hip'))
    # it stands on its own: the tile's description and the launchers' header, neither walk
    assert re.findall(r'#include "([^"]+)"', unit) == ['launch.h', 'tri_tile.hip.h'] and 'asm' not in unit
    with open(os.path.join(csrc, 'k_moments.hip')) as fh:
        assert 'NOT a pass of band_walk' in fh.read()
    # none of the walk's names, and neither of the two lines pinned to the files that have them
    for word in ('key_of', 'lower_hit', 'hit_word', 'band_grid', 'kBand', 's_row[tid >> 2][tid & 3]', 'check_band_tile'):
        assert word not in unit, word
    assert 'rows = (int)min((int64_t)kBandRows, t.n_rows - r_lo)' not in unit
    kernel = unit[unit.index('__global__'):unit.index('namespace dctfp_host')]
    assert 'void rect_moments_kernel(const TriTile t, unsigned long long* row_mom, int64_t n_a,' in kernel
    # the output arrays: named behind the head, then only as the base of an address handed to mom_add -- three words a side
    for array in ('row_mom', 'col_mom'):
        uses = re.findall(r'\b%s\b' % array, kernel)
        assert len(uses) == 4 and len(re.findall(r'mom_add\(%s \+ ' % array, kernel)) == 3
        assert not re.search(r'%s\s*\[|(?<!long)\*\s*\(?\s*%s' % (array, array), kernel)
        assert array not in unit[:unit.index('__global__')] and array not in unit[unit.index('namespace dctfp_host'):]
    assert unit.count('__ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT') == 1 and unit.count('__HIP_MEMORY_SCOPE_AGENT') == 1
    assert unit.count('__hip_atomic_') == 1
    helper = unit[unit.index('void mom_add('):unit.index('template <bool kRowSide')]
    assert '__hip_atomic_fetch_add(slot, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);' in helper
    # no workgroup waits for another, and an idle part is not sent
    assert not re.search(r'\bwhile\b|for \(;;\)', unit)
    assert 'if (n != 0) {' in kernel and 'if (col_n[e] == 0) continue;' in kernel
    # the flags: once per column and job, once per row and job -- both in front of the row loop, none inside it
    loop = kernel.index('for (int rl = 0;')
    assert len(re.findall(r'\bcol_empty\[', kernel)) == 1 and len(re.findall(r'\brow_empty\[', kernel)) == 1
    assert kernel.index('col_empty[') < kernel.index('row_empty[') < loop
    # why the 32-bit sums cannot overflow is asserted where it is written, and the export holds the caller to it
    assert 'static_assert((int64_t)64 * kMomPer * (kMomMaxCap - 1) < ((int64_t)1 << 32)' in unit
    assert 'static_assert((int64_t)kMomRows * (kMomMaxCap - 1) < ((int64_t)1 << 32)' in unit
    with open(os.path.join(csrc, 'dctfp_sim.hip')) as fh:
        text = fh.read()
    body = text[text.index('\nint dctfp_rect_moments('):text.index('DCTFP_GUARD("dctfp_rect_moments")')]
    assert 'check_band_tile(' not in body and 'check_tri_tile(' not in body and 'ld < n_cols' in body and 'rect_moments_max_cap()' in body
    assert 'unsigned __int128' in body and body.count('fail(DCTFP_ERR_INVALID, "dctfp_rect_moments: ') == 8
