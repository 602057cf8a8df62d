"""The two one-launch kernels by name: what the options "last_walk" / "last_gen" (include/dctfp.h) say, the tables of every
walk_ab_kernel build (csrc/k_walk.hip) and every walk_gen_kernel build (csrc/k_gen.hip) the two launch ladders can launch --
written by hand from the ladders, not derived from the library --, the rules that pick one (choose_route, walk_shape and
gen_slot_bytes / gen_wg_per_cu of csrc/dctfp.hip and csrc/launch.h, copied by hand as well), and the inputs that run each of
them once against the float64 oracle.  Importing needs no GPU.

The inputs are stage_ladder.py's: `Workload`, the seed search of `_finish` / `_oracle` (no degenerate channel but the planted
ones, every 127 Z other than an exact 0 or 127 at least TIE_MARGIN from an integer), `round_to_storage`, `to_device`.  Every
call of the GPU test is forced to the one-launch kernels ("path" = 2), so the size of a call only has to satisfy the fuse rule
of choose_route: a FUSED build is asked for by proteins given as parts + whole protein in a call of 64 jobs (layers x domains)
or more; the same workload under "fuse" = 0 (walk kernel) / "gen_fuse" = 0 (general kernel) asks for the plain build.

What these workloads do not do on their own: a call of 82 .. 106 jobs is fewer jobs than the chip holds workgroups, so run_length
(csrc/dctfp.hip) gives every plain call one job per workgroup -- flush groups of one job, no loop over jobs, a second Y' slot
that is allocated and never written.  tests/test_walk_ladder_gpu.py runs them again under "ab_run_jobs" for that."""

from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

from oracle import dct_oracle as orc
from recipes import make_input
from stage_ladder import ESIZE, STORAGES, TIE_MARGIN, Workload, _finish, _oracle, round_to_storage, to_device  # noqa: F401

# ---- the two option words ---------------------------------------------------------------------------------------------
WalkBuild = namedtuple('WalkBuild', 'storage s nt fused win')
GenBuild = namedtuple('GenBuild', 'storage n vec ntc fused')
GenLaunch = namedtuple('GenLaunch', 'build waves slots')


def decode_walk(word: int):
    """"last_walk" -> WalkBuild, None for 0 (another route).  Byte 0 storage + 1, byte 1 S, byte 2 NT, byte 3: 1 FUSED, 2 WIN."""
    if word == 0:
        return None
    b = [(word >> (8 * i)) & 0xff for i in range(8)]
    assert 1 <= b[0] <= 4 and b[3] < 4 and not any(b[4:]), hex(word)
    return WalkBuild(STORAGES[b[0] - 1], b[1], b[2], bool(b[3] & 1), bool(b[3] & 2))


def decode_gen(word: int):
    """"last_gen" -> GenLaunch, None for 0.  Byte 0 storage + 1, byte 1 N, byte 2 VEC, byte 3 NTC, byte 4: 1 FUSED, byte 5 the
    waves launched, byte 6 the Y' slots."""
    if word == 0:
        return None
    b = [(word >> (8 * i)) & 0xff for i in range(8)]
    assert 1 <= b[0] <= 4 and b[4] < 2 and b[7] == 0, hex(word)
    return GenLaunch(GenBuild(STORAGES[b[0] - 1], b[1], b[2], b[3], bool(b[4] & 1)), b[5], b[6])


# ---- the tables ---------------------------------------------------------------------------------------------------------
WALK_STORAGES = ('f32', 'f16', 'bf16')       # walk_shape: `if (ly.dtype == DCTFP_F64) return false;`
WALK_S = (3, 5, 10)
GEN_LAYOUTS = (('f32', 4), ('f32', 1), ('f64', 2), ('f64', 1))       # launch_gen: (storage, VEC); VEC 1 = rows not 16-byte aligned
GEN_N = (2, 3, 4, 5, 6, 7, 8)
GEN_FUSED_MAX_N, GEN_FUSED_MAX_WAVES = 5, 10     # launch.h: kGenFusedMaxN, kGenFusedMaxWaves
GEN_LDS_BUDGET = 150 * 1024                      # launch.h: kGenLdsBudget


def _walk_table():
    """WalkBuild -> None (reachable) or the reason it is not.  Row by row as launch_walk / launch_walk_impl are written:
      launch_walk, half precision: S = 3 / 5 / 10 at NT 5, float16 and bfloat16;
      launch_walk, `p.m > 80`: S = 3 / 5 / 10 at NT 6, float32 only;
      launch_walk, the rest: S = 3 / 5 / 10 at NT 5, float32;
      launch_walk_impl: each plain and FUSED; `sizeof(T) == 4 && NT == 5` and p.two_source: the two WIN builds beside them."""
    table = {}

    def add(storage, nt, win):
        for s in WALK_S:
            for fused in (False, True):
                b = WalkBuild(storage, s, nt, fused, win)
                assert b not in table, b
                table[b] = None

    for storage in ('f16', 'bf16'):
        add(storage, 5, False)
    add('f32', 6, False)
    add('f32', 5, False)
    add('f32', 5, True)
    return table


def _gen_table():
    """GenBuild -> None or the reason.  As launch_gen / launch_gen_n / launch_gen_impl are written: float32 at VEC 4 / 1, float64
    at VEC 2 / 1; the fused switch N = 2 .. 5, the plain switch N = 2 .. 8; each at NTC 4 (m <= 64) and NTC 8."""
    table = {}
    for storage, vec in GEN_LAYOUTS:
        for fused, ns in ((True, (2, 3, 4, 5)), (False, GEN_N)):
            for n in ns:
                for ntc in (4, 8):
                    b = GenBuild(storage, n, vec, ntc, fused)
                    assert b not in table, b
                    table[b] = None
    return table


WALK_BUILDS = _walk_table()
GEN_BUILDS = _gen_table()


def walk_builds_of(storage, s, win=False, reachable=True):
    return {b for b, why in WALK_BUILDS.items() if (b.storage, b.s, b.win) == (storage, s, win) and (why is None) == reachable}


def gen_builds_of(layout, n, reachable=True):
    return {b for b, why in GEN_BUILDS.items() if (b.storage, b.vec, b.n) == (*layout, n) and (why is None) == reachable}


# ---- the rules, copied by hand ------------------------------------------------------------------------------------------
def is_walk_shape(storage, aligned, n, m, D):
    """walk_shape and the alignment walk_refusal asks for: what walk_ab_kernel takes under "path" = 2 (domains of at most 8 192
    rows).  rows_aligned16 needs D % (16 / element size) == 0 beside the pointers and the leading dimension."""
    if storage == 'f64' or not aligned:
        return False
    m_max = 96 if storage == 'f32' else 80
    return n == 3 and 64 < m <= m_max and 512 <= D <= 2560 and D % 4 == 0 and D % (16 // ESIZE[storage]) == 0


def expected_walk(storage, D, m, fused, windows=False):
    """The walk_ab_kernel build of a call at kept sizes [3, m] on 16-byte aligned rows of width D; `fused`: the call asks for fused
    walks (parts + whole protein, >= 64 jobs, "fuse" = 1); `windows`: some piece is the mean of two windows' rows."""
    assert is_walk_shape(storage, True, 3, m, D), (storage, D, m)
    assert not windows or (storage == 'f32' and m <= 80)              # two_source_refusal
    s = 3 if D <= 768 else (5 if D <= 1280 else 10)                   # choose_route: r.walk_s
    nt = 6 if m > 80 else 5                                           # launch_walk: `if (p.m > 80)`
    b = WalkBuild(storage, s, nt, bool(fused), bool(windows))
    assert b in WALK_BUILDS, b
    return b


def gen_slot_bytes(n, m, waves, vec):
    """launch.h: Y'[N][CH] float64, and the partial Z blocks [S][N][cp] behind it where a wave's columns are too few to hold them."""
    ch, cp = waves * 64 * vec, (m + 15) // 16 * 16
    return (n * ch + (0 if cp <= 64 * vec else waves * n * cp)) * 8


def gen_wg_per_cu(n, m, waves, vec, slots):
    """dctfp.hip: workgroups per CU by waves (20 per CU) and by LDS."""
    return min(max(1, 20 // waves), GEN_LDS_BUDGET // (slots * gen_slot_bytes(n, m, waves, vec) + 64))


def gen_fits(n, m, waves, vec):
    return waves <= 16 and gen_slot_bytes(n, m, waves, vec) + 64 <= GEN_LDS_BUDGET


def expected_gen(storage, aligned, n, m, D, fused) -> GenLaunch:
    """The walk_gen_kernel build, its waves and its Y' slots for a call at kept sizes [n, m] on rows of width D (`aligned`: every
    row 16-byte aligned and D a multiple of the lane's channels); `fused` as for expected_walk, with "gen_fuse" = 1."""
    assert storage in ('f32', 'f64') and 2 <= n <= 8 and 2 <= m <= 128
    assert not is_walk_shape(storage, aligned, n, m, D), (storage, n, m, D)
    vec = (16 // ESIZE[storage]) if aligned else 1                    # choose_route: r.gen_vec
    assert not aligned or D % vec == 0
    waves = (D + 64 * vec - 1) // (64 * vec)
    assert gen_fits(n, m, waves, vec), (n, m, waves, vec)             # r.gen_slots >= 1
    slots = 2 if gen_wg_per_cu(n, m, waves, vec, 2) >= gen_wg_per_cu(n, m, waves, vec, 1) else 1
    fused_build = bool(fused) and n <= GEN_FUSED_MAX_N and waves <= GEN_FUSED_MAX_WAVES      # r.gen_fuse
    ntc = 4 if m <= 64 else 8                                         # launch_gen_impl
    b = GenBuild(storage, n, vec, ntc, fused_build)
    assert b in GEN_BUILDS, b
    return GenLaunch(b, waves, slots)


# ---- proteins and domain lists --------------------------------------------------------------------------------------------
BIG_LENS = (31, 40, 64, 95, 127, 128, 129, 140, 200, 257, 300)
NAN_LEN, CONST_LEN = 95, 129             # the proteins that carry the planted NaN / constant channel (both: parts + whole protein)


def ladder_lens(n):
    """n, n + 1, 7, 8, 9, 16, 17 (eight rows in flight: one short of, exactly and one past one and two rounds) as far as a
    protein of that many rows can be kept as n, then stage_a_lens's longer ones up to 300."""
    return sorted({L for L in (n, n + 1, 7, 8, 9, 16, 17) if L >= n}) + list(BIG_LENS)


def ladder_domains(n):
    """stage_a_domains' rule on ladder_lens: whole protein only below 3 n + 3 rows; else two or three parts that tile it, then the
    whole protein; the protein of 140 rows has its first and last third as one discontinuous part, written last piece first."""
    doms = []
    for i, L in enumerate(ladder_lens(n)):
        c1, c2 = L // 3, 2 * L // 3 + 1
        if L < 3 * n + 3:
            doms.append([f'1-{L}'])
        elif L == 140:
            doms.append([f'{c2 + 1}-{L},1-{c1}', f'{c1 + 1}-{c2}', f'1-{L}'])
        elif i % 2:
            doms.append([f'1-{c1}', f'{c1 + 1}-{c2}', f'{c2 + 1}-{L}', f'1-{L}'])
        else:
            c = L // 2 + 1
            doms.append([f'1-{c}', f'{c + 1}-{L}', f'1-{L}'])
    return doms


def _ladder_workload(name, storage, n, m, D, ld, col_off, base_seed):
    """ladder_lens / ladder_domains at kept sizes [n, m] twice.  Planted in layer 0, next to the fold line D / 2 - 1 of the walk
    kernel's channel pairs: a NaN (the protein of 95 rows, row 50, channel D / 2) and a constant channel D / 2 - 1 (the protein
    of 129 rows); layer 1 is left alone, its blocks must not notice."""
    lens, doms = ladder_lens(n), ladder_domains(n)
    p_nan, p_const = lens.index(NAN_LEN), lens.index(CONST_LEN)
    assert len(doms[p_nan]) > 1 and len(doms[p_const]) > 1 and D // 2 < D
    assert 2 * sum(len(d) for d in doms) >= 64 and any(len(d) > 1 for d in doms)          # the fuse rule: >= 64 jobs, with groups
    planted = {(0, p_const): (D // 2 - 1,)}

    def fill(layers):
        layers[0][p_nan][50, D // 2] = np.nan
        layers[0][p_const][:, D // 2 - 1] = 0.5

    w = _finish(name, storage, n, m, D, ld, col_off, lens, doms, base_seed, fill, planted)
    first = np.cumsum([0] + [len(d) for d in doms])
    zero = [(int(first[p_const]) + k, 0) for k in range(len(doms[p_const]))]
    for k, dom in enumerate(doms[p_nan]):                 # the domains that hold row 50 (1-based 51)
        if any(b < 51 <= e for b, e in orc.split_domain(dom, NAN_LEN)[0]):
            zero.append((int(first[p_nan]) + k, 0))
    w.zero_blocks = sorted(zero)
    w.degenerate = len(doms[p_const])
    assert len(w.zero_blocks) == w.degenerate + 2         # (the NaN: a part and the whole protein)
    return w


# ---- walk_ab_kernel -------------------------------------------------------------------------------------------------------
#: widths per wave count: both ends of it, one with D % 8 == 4 (two lanes hold the same four channels of a pair group) and one whose
#: half is no multiple of 16 (zero-padded pair groups).  rows_aligned16 wants D % 8 == 0 of half-precision rows, so 516, 772, 1284
#: and 2052 are float32's alone
WALK_WIDTHS = {
    'f32': {3: (512, 516, 768), 5: (772, 1000, 1280), 10: (1284, 2052, 2560)},
    'half': {3: (512, 520, 768), 5: (776, 1000, 1280), 10: (1288, 2056, 2560)},
}
WALK_M = {5: (65, 80), 6: (81, 96)}          # both ends of the kept columns of an NT


def walk_widths(storage, s):
    return WALK_WIDTHS['f32' if storage == 'f32' else 'half'][s]


def walk_cases(storage, s):
    """(D, m) of every workload of a (storage type, wave count): every width at both ends of NT 5 and -- float32 -- of NT 6."""
    ms = WALK_M[5] + (WALK_M[6] if storage == 'f32' else ())
    return [(D, m) for D in walk_widths(storage, s) for m in ms]


@functools.lru_cache(maxsize=2)
def walk_workload(storage, D, m):
    """16-byte aligned rows (leading dimension D + 16 bytes at the widths that are no multiple of 64 channels)."""
    ld = D if D % 64 == 0 else D + 16 // ESIZE[storage]
    return _ladder_workload(f'walk_{storage}_D{D}_m{m}', storage, 3, m, D, ld, 0,
                            5_000_000 + 100_000 * WALK_STORAGES.index(storage) + 10 * D + m)


# -- the two-source builds (dctfp_quantize_windows)
OVERLAP = 200
#: rows of the two windows of every sequence: 201 .. 260, the fewest the reference's overlap of 200 allows and a few more
WINDOW_ROWS = ((201, 260), (260, 201), (203, 203), (204, 231), (217, 208), (260, 260), (222, 205), (209, 247), (233, 203), (205, 250),
               (244, 212), (203, 260), (251, 207))
WINDOW_CASES = {3: ((516, 80), (768, 65)), 5: ((772, 65), (1280, 80)), 10: ((1284, 80), (2560, 65))}    # (D, m) per wave count
WIN_NAN_SEQ, WIN_CONST_SEQ = 4, 7


def window_domains(r0, r1, i):
    """Domain list of a sequence of two windows (stitched rows L = r0 + r1 - 200; the windows share the rows r0 - 199 .. r0, 1-based):
    cuts ON both borders of the shared rows where that leaves three rows to each part, cuts INSIDE the shared rows, or the first and
    last part as one discontinuous domain (written last piece first) with one cut inside and one on the border."""
    L = r0 + r1 - OVERLAP
    own0 = r0 - OVERLAP
    if i % 3 == 0 and own0 >= 3 and L - r0 >= 3:
        return [f'1-{own0}', f'{own0 + 1}-{r0}', f'{r0 + 1}-{L}', f'1-{L}']
    if i % 3 == 2 and L - r0 >= 3:
        return [f'{r0 + 1}-{L},1-{own0 + 99}', f'{own0 + 100}-{r0}', f'1-{L}']
    return [f'1-{own0 + 49}', f'{own0 + 50}-{own0 + 151}', f'{own0 + 152}-{L}', f'1-{L}']


@functools.lru_cache(maxsize=2)
def window_workload(D, m):
    """13 sequences of two float32 windows each, kept sizes [3, m] twice.  w.windows[li]: the windows of a layer, sequence after
    sequence; w.layers: the stitched sequences (the reference's `run[-olp:] = (run[-olp:] + new[:olp]) / 2`, stitch_oracle) the
    expected rows are computed from.  Planted in layer 0: a NaN in an own row of a first window, and a channel that is the same
    constant in both windows of a sequence."""
    import torch
    from oracle import stitch_oracle as so
    lens = [r0 + r1 - OVERLAP for r0, r1 in WINDOW_ROWS]
    doms = [window_domains(r0, r1, i) for i, (r0, r1) in enumerate(WINDOW_ROWS)]
    assert 2 * sum(len(d) for d in doms) >= 64
    planted = {(0, WIN_CONST_SEQ): (D // 2 - 1,)}
    base_seed = 6_000_000 + 10 * D + m
    name = f'windows_D{D}_m{m}'
    for seed in range(base_seed, base_seed + 16):
        windows = [[make_input('gauss', r, D, seed * 1000 + 4 * s + 2 * k + li) for s, rows in enumerate(WINDOW_ROWS)
                    for k, r in enumerate(rows)] for li in range(2)]
        windows[0][2 * WIN_NAN_SEQ][1, D // 2] = np.nan            # row 2 of the sequence: one of the first window's own
        for k in range(2):
            windows[0][2 * WIN_CONST_SEQ + k][:, D // 2 - 1] = 0.5
        layers = [[so.stitch_embeddings([torch.from_numpy(x) for x in win[2 * s:2 * s + 2]], OVERLAP).numpy()
                   for s in range(len(lens))] for win in windows]
        assert all(x.shape == (L, D) for layer in layers for x, L in zip(layer, lens))
        expected, margin, unplanted = _oracle(layers, lens, doms, 3, m, planted)
        if margin >= TIE_MARGIN and not unplanted:
            break
    else:
        raise AssertionError(f'{name}: no seed in {base_seed} .. {base_seed + 15} meets the input conditions')
    w = Workload(name=name, storage='f32', n=3, m=m, D=D, ld=D, col_off=0, lens=lens, doms=doms, layers=layers, expected=expected,
                 seed=seed, base_seed=base_seed, margin=margin, planted=planted, windows=windows)
    first = np.cumsum([0] + [len(d) for d in doms])
    zero = [(int(first[WIN_CONST_SEQ]) + k, 0) for k in range(len(doms[WIN_CONST_SEQ]))]
    for k, dom in enumerate(doms[WIN_NAN_SEQ]):
        if any(b < 2 <= e for b, e in orc.split_domain(dom, lens[WIN_NAN_SEQ])[0]):
            zero.append((int(first[WIN_NAN_SEQ]) + k, 0))
    w.zero_blocks = sorted(zero)
    w.degenerate = len(doms[WIN_CONST_SEQ])
    assert len(w.zero_blocks) == w.degenerate + 2
    return w


def windows_to_device(w, dd):
    """(layer batches of one matrix per window, window rows, windows per sequence, piece table of the stitched sequences)."""
    import torch
    lbs = [dd.LayerBatch([torch.from_numpy(x).cuda() for x in win], w.n, w.m) for win in w.windows]
    rows = np.asarray([r for pair in WINDOW_ROWS for r in pair], dtype=np.int32)
    return lbs, rows, np.full(len(WINDOW_ROWS), 2, dtype=np.int64), dd.PieceTable(w.lens, w.doms)


# ---- walk_gen_kernel ------------------------------------------------------------------------------------------------------
GenCase = namedtuple('GenCase', 'm D ld col_off')


def _gen_width(layout, waves):
    """(D, ld, first column) of a width of `waves` waves that ends inside the last wave.  16-byte aligned rows (VEC > 1) end three
    lanes short of it -- a lane's channels cannot be cut there: rows_aligned16 wants D % VEC == 0 --; unaligned rows (VEC 1) end
    three channels short of it and start one element into rows whose leading dimension alone would allow 16 bytes per lane."""
    storage, vec = layout
    if vec > 1:
        D = waves * 64 * vec - 3 * vec
        return D, D, 0
    return waves * 64 - 3, waves * 64, 1


def gen_ms(layout, n, m_low, m_top, waves):
    """The kept columns m_low .. m_top a width of `waves` waves takes through walk_gen_kernel at kept rows n: the slot fits the LDS,
    walk_ab_kernel does not take the shape, and m < D (m = D resamples nothing: the kept columns are the channels themselves, and at
    N = 2, where every Y' is 0 or 1, every 127 Z is a rounded 0 or 127)."""
    storage, vec = layout
    D = _gen_width(layout, waves)[0]
    return [m for m in range(m_low, min(m_top, D - 1) + 1)
            if gen_fits(n, m, waves, vec) and not is_walk_shape(storage, vec > 1, n, m, D)]


def gen_widest(layout, n, ms, cap):
    """The most waves <= cap that take some m of `ms`."""
    for waves in range(cap, 0, -1):
        if gen_ms(layout, n, min(ms), max(ms), waves):
            return waves
    raise AssertionError((layout, n, ms, cap))


def gen_cases(layout, n):
    """The workloads of a (memory layout, N): per NTC (m = 2 .. 64; 65 .. 128) the fewest and the most kept columns a width takes
    (gen_ms), at one wave (two where one wave has fewer than 65 channels), at the widest the plain build allows (16 waves,
    fewer where the LDS says so) and, for N <= 5, at the widest the FUSED build allows (10 waves) where that is another width.
    The widest is chosen per end of the kept columns: float32 rows at N = 3 and m = 65 .. 96 are walk_ab_kernel's from 512 to 2560
    channels, so the widest FUSED width of m = 65 is two waves, and that of the upper end -- m = 97 .. 128 -- the full ten."""
    cases = []
    for m_low, m_top in ((2, 64), (65, 128)):
        widths = [min(waves for waves in (1, 2) if _gen_width(layout, waves)[0] > m_low)]
        for cap in (16, GEN_FUSED_MAX_WAVES) if n <= GEN_FUSED_MAX_N else (16,):
            widths += [gen_widest(layout, n, (m_low,), cap), gen_widest(layout, n, range(m_low, m_top + 1), cap)]
        for waves in sorted(set(widths)):
            D, ld, off = _gen_width(layout, waves)
            ms = gen_ms(layout, n, m_low, m_top, waves)
            cases += [GenCase(m, D, ld, off) for m in sorted({ms[0], ms[-1]})]
    return cases


@functools.lru_cache(maxsize=2)
def gen_workload(layout, n, case):
    storage, vec = layout
    return _ladder_workload(f'gen_{storage}x{vec}_n{n}_m{case.m}_D{case.D}', storage, n, case.m, case.D, case.ld, case.col_off,
                            7_000_000 + 200_000 * GEN_LAYOUTS.index(layout) + 20_000 * n + 4 * case.D + case.m)
