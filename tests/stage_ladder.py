"""The two-kernel path by name: what the options "last_stage_a" / "last_stage_b" (include/dctfp.h) say, the table of every
stage-A build the launch ladder of csrc/k_stage_a.inc can launch -- written by hand from the ladder's rules, not derived from
the library -- and the inputs that run each of them once against the float64 oracle.  Importing needs no GPU.

Every workload carries its expected int8 rows, computed once by the oracle (`get_doms` + `quantize_layer_matrix`, the two
calls `quantize_matrix` is made of, so that the intermediates are at hand), under two conditions on the input that make an
off-by-one indefensible as a tie:
  * no channel of any domain is exactly constant except the planted ones -- nor degenerate in the wider sense the counter
    "degenerate_channels" has (include/dctfp.h): N resampled values that are equal in exact arithmetic, where the kernels
    write 0 and the float64 oracle scales its own round-off (3 rows kept as 2 with equal first and last value: the one
    coefficient is cos(pi / 2) times the middle value -- and two bfloat16 values of 8 mantissa bits meet in some channel at
    every seed); a range of the resampled values below 1e-9 of the range of the channel's rows counts as that;
  * every v = 127 Z other than an exact 0 or 127 is at least 1e-9 away from an integer -- a builder that meets a closer
    value takes the next seed (`Workload.seed`; it goes into every assertion message)."""

from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

from oracle import dct_oracle as orc
from recipes import make_input

# ---- the two option words ---------------------------------------------------------------------------------------------
STORAGES = ('f32', 'f64', 'f16', 'bf16')     # DCTFP_F32 .. DCTFP_BF16, in the header's order

StageA = namedtuple('StageA', 'storage n vec waves unroll fused packed split')
StageB = namedtuple('StageB', 'form nt packed combine combine_packed')
MFMA, SLAB, SLAB_FROM_SPLIT = 1, 2, 3


def decode_stage_a(word: int):
    """"last_stage_a" -> StageA, None for 0 (another route).  One byte per field; byte 5: 1 fused, 2 packed, 4 split."""
    if word == 0:
        return None
    b = [(word >> (8 * i)) & 0xff for i in range(8)]
    assert 1 <= b[0] <= 4 and b[6] == 0 and b[7] == 0 and b[5] < 8, hex(word)
    return StageA(STORAGES[b[0] - 1], b[1], b[2], b[3], b[4], bool(b[5] & 1), bool(b[5] & 2), bool(b[5] & 4))


def decode_stage_b(word: int):
    """"last_stage_b" -> StageB, None for 0.  Byte 0 form, byte 1 NT, byte 2: 1 PACKED, 2 combine ran, 4 ... packed."""
    if word == 0:
        return None
    form, nt, flags = word & 0xff, (word >> 8) & 0xff, (word >> 16) & 0xff
    assert form in (MFMA, SLAB, SLAB_FROM_SPLIT) and flags < 8 and word >> 24 == 0, hex(word)
    return StageB(form, nt, bool(flags & 1), bool(flags & 2), bool(flags & 4))


# ---- the table ----------------------------------------------------------------------------------------------------------
Build = namedtuple('Build', 'storage n vec waves unroll fused')

# choose_route: `if (r.fuse && n == 3 && r.vec == 8) r.vec = 4;` -- half-precision rows at N = 3 are read 4 channels per lane if
# and only if the walks are fused, so neither the unfused 4-channel builds nor the fused 8-channel builds can be asked for
UNREACHABLE_VEC4 = 'UNREACHABLE: the route lowers 8 channels per lane to 4 only for fused walks'
UNREACHABLE_VEC8 = 'UNREACHABLE: the route lowers 8 channels per lane to 4 for every fused walk at N = 3'

#: the memory layouts a caller can hand over: (storage, channels per lane of 16 bytes; 1 = rows that are not 16-byte aligned)
LAYOUTS = (('f32', 4), ('f32', 1), ('f64', 2), ('f64', 1), ('f16', 8), ('f16', 1), ('bf16', 8), ('bf16', 1))
A_WAVES = (2, 4, 8, 16)          # what the option "a_waves" can force
N_RANGE = (2, 3, 4, 5, 6, 7, 8)


def _build_table():
    """Build -> None (reachable) or the reason it is not.  Row by row as the ladder is written:
      launch_a_cfg (N = 2, 3): 2 / 4 / 8 waves, 4 rows in flight; 8 channels per lane stop at 4 waves; 4 channels per lane
        also have 16 waves, with 8 rows in flight unless fused;
      launch_a_n   (N = 4 .. 8): 4 waves, 4 rows in flight;
      every one plain and fused;
      float16 / bfloat16 at 4 channels per lane: launch_a_cfg at N = 3 only."""
    table = {}

    def add(storage, vec, ns, waves):
        for n in ns:
            for w in waves:
                for fused in (False, True):
                    unroll = 8 if (w == 16 and not fused) else 4
                    b = Build(storage, n, vec, w, unroll, fused)
                    assert b not in table, b
                    half = storage in ('f16', 'bf16')
                    table[b] = (UNREACHABLE_VEC4 if (half and vec == 4 and not fused) else
                                UNREACHABLE_VEC8 if (half and vec == 8 and n == 3 and fused) else None)

    add('f32', 4, (2, 3), (2, 4, 8, 16))
    add('f32', 4, (4, 5, 6, 7, 8), (4,))
    for storage, vec in (('f32', 1), ('f64', 2), ('f64', 1), ('f16', 1), ('bf16', 1)):
        add(storage, vec, (2, 3), (2, 4, 8))
        add(storage, vec, (4, 5, 6, 7, 8), (4,))
    for storage in ('f16', 'bf16'):
        add(storage, 8, (2, 3), (2, 4))
        add(storage, 8, (4, 5, 6, 7, 8), (4,))
        add(storage, 4, (3,), (2, 4, 8, 16))
    return table


BUILDS = _build_table()


def waves_for(request: int, vec: int, n: int) -> int:
    """The WAVES an "a_waves" request ends in: 16 -> 8 unless 4 channels per lane, above 4 -> 4 at 8 channels per lane,
    N >= 4 -> 4."""
    assert request in A_WAVES
    if n >= 4:
        return 4
    w = request
    if w == 16 and vec != 4:
        w = 8
    if vec == 8 and w > 4:
        w = 4
    return w


def expected_build(layout, n: int, a_waves: int, fused: bool) -> Build:
    """The table's entry for a request on a memory layout (half-precision rows of 8 channels per lane: fused walks at N = 3
    read 4)."""
    storage, vec = layout
    if vec == 8 and n == 3 and fused:
        vec = 4
    waves = waves_for(a_waves, vec, n)
    b = Build(storage, n, vec, waves, 8 if (waves == 16 and not fused) else 4, fused)
    assert b in BUILDS, b
    return b


def builds_of_layout(layout, reachable=True):
    """The table's builds a memory layout can end in (8 channels per lane: also the 4-channel ones of the storage type)."""
    storage, vec = layout
    return {b for b, why in BUILDS.items()
            if b.storage == storage and (b.vec == vec or (vec == 8 and b.vec == 4)) and (why is None) == reachable}


# ---- inputs ---------------------------------------------------------------------------------------------------------------
TIE_MARGIN = 1e-9
DEGENERATE_RANGE = 1e-9      # range of a channel's N resampled values, as a fraction of the range of its rows
ESIZE = {'f32': 4, 'f64': 8, 'f16': 2, 'bf16': 2}


class Workload:
    """Proteins, domain strings and layers of one call, with the oracle's answer.
    layers[li][s]: (L_s, D) matrix of protein s as the oracle reads it (float32, the storage type's values promoted;
    float64 for float64 storage); expected: (domains, layers * n * m) int64; zero_blocks: (row, layer) pairs whose block is
    planted to be all 0; degenerate: jobs of the call that stream a planted constant channel; margin: the smallest distance of
    a 127 Z from an integer (exact 0 and 127 apart); planted: {(layer, protein): constant channels}."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def n_domains(self):
        return sum(len(d) for d in self.doms)

    def __repr__(self):
        return (f'<{self.name} {self.storage} D={self.D} ld={self.ld} off={self.col_off} [{self.n}, {self.m}] '
                f'seed {self.seed}>')


def round_to_storage(x32: np.ndarray, storage: str) -> np.ndarray:
    """float32 values rounded to the storage type and promoted back (float64 storage: widened)."""
    if storage == 'f32':
        return x32
    if storage == 'f64':
        return x32.astype(np.float64)
    import torch
    dt = torch.float16 if storage == 'f16' else torch.bfloat16
    return torch.from_numpy(np.ascontiguousarray(x32)).to(dt).float().numpy()


def _oracle(layers, lens, doms, n, m, planted):
    """(expected rows, the smallest distance of a 127 Z other than an exact 0 or 127 from an integer, the constant or otherwise
    degenerate channels of a domain -- as (layer, protein, channel) -- that are not in `planted`: {(layer, protein): channels})."""
    n_dom = sum(len(d) for d in doms)
    margin, unplanted = np.inf, set()
    out = np.zeros((n_dom, len(layers) * n * m), dtype=np.int64)
    for li, layer in enumerate(layers):
        row = 0
        for s, L in enumerate(lens):
            for dom in doms[s]:
                mat, _ = orc.get_doms(layer[s], dom)
                assert mat.shape[0] >= n, (dom, L, n)
                const = set(np.flatnonzero((mat == mat[0:1]).all(axis=0)).tolist())
                q, inter = orc.quantize_layer_matrix(mat, n, m, want_intermediates=True)
                a = inter['A']
                with np.errstate(invalid='ignore'):
                    flat = (a.max(axis=0) - a.min(axis=0)) <= DEGENERATE_RANGE * np.abs(mat - mat[0:1]).max(axis=0)
                const |= set(np.flatnonzero(flat).tolist())
                unplanted |= {(li, s, c) for c in const - set(planted.get((li, s), ()))}
                v = 127.0 * inter['Z']
                v = v[np.isfinite(v) & (v != 0.0) & (v != 127.0)]
                if v.size:
                    margin = min(margin, float(np.abs(v - np.rint(v)).min()))
                out[row, li * n * m:(li + 1) * n * m] = q
                row += 1
    return out, margin, unplanted


def _distinct_rows(x):
    """A protein of two or three rows: no value twice in a channel (8 mantissa bits repeat one in some channel at every seed,
    and two equal rows of two, or an equal first and last row of three, are a degenerate channel).  The repeated value is
    negated, doubled or halved: exact in every storage type."""
    if x.shape[0] > 3:
        return
    for r in range(1, x.shape[0]):
        for c in np.flatnonzero((x[r:r + 1] == x[:r]).any(axis=0)):
            v = x[r, c] if x[r, c] != 0 else 1.0
            x[r, c] = next(u for u in (-v, 2 * v, 0.5 * v, -2 * v) if not (x[:r, c] == u).any())


def _finish(name, storage, n, m, D, ld, col_off, lens, doms, base_seed, fill, planted_of, n_layers=2):
    """Values by recipe 'gauss' from the first seed >= base_seed that meets the input conditions; `fill(layers)` plants and
    returns nothing; `planted_of`: see _oracle."""
    for seed in range(base_seed, base_seed + 16):
        layers = [[round_to_storage(make_input('gauss', L, D, seed * 1000 + 2 * s + li), storage).copy()
                   for s, L in enumerate(lens)] for li in range(n_layers)]
        for layer in layers:
            for x in layer:
                _distinct_rows(x)
        fill(layers)
        expected, margin, unplanted = _oracle(layers, lens, doms, n, m, planted_of)
        if margin >= TIE_MARGIN and not unplanted:
            break
    else:
        raise AssertionError(f'{name}: no seed in {base_seed} .. {base_seed + 15} meets the input conditions')
    return Workload(name=name, storage=storage, n=n, m=m, D=D, ld=ld, col_off=col_off, lens=list(lens), doms=doms,
                    layers=layers, expected=expected, seed=seed, base_seed=base_seed, margin=margin, planted=planted_of)


# -- stage A
def stage_a_lens(n):
    return [n, n + 1, 31, 40, 64, 95, 127, 128, 129, 140, 200, 257, 300]


def stage_a_domains(n):
    """Per protein: whole only below 3 n + 3 rows; else two or three parts that tile it, then the whole protein.  The
    protein of 140 rows has its first and last third as one discontinuous part, written last piece first."""
    doms = []
    for i, L in enumerate(stage_a_lens(n)):
        if L < 3 * n + 3:
            doms.append([f'1-{L}'])
        elif L == 140:
            c1, c2 = L // 3, 2 * L // 3 + 1
            doms.append([f'{c2 + 1}-{L},1-{c1}', f'{c1 + 1}-{c2}', f'1-{L}'])
        elif i % 2:
            c1, c2 = L // 3, 2 * L // 3 + 1
            doms.append([f'1-{c1}', f'{c1 + 1}-{c2}', f'{c2 + 1}-{L}', f'1-{L}'])
        else:
            c = L // 2 + 1
            doms.append([f'1-{c}', f'{c + 1}-{L}', f'1-{L}'])
    return doms


#: widths per memory layout, as (D, ld, first column of the view): one that ends a few channels into the second slab (with a
#: leading dimension padded by 16 bytes where the rows are 16-byte aligned) and one that is exactly one slab; 1 channel per
#: lane: D = 67, and for float32 an aligned width and leading dimension with every row off by one element -- with the odd
#: width and the leading dimension of D = 67 the three reasons of rows_aligned16
STAGE_A_WIDTHS = {('f32', 4): [(260, 264, 0), (256, 256, 0)], ('f64', 2): [(130, 132, 0), (128, 128, 0)],
                  ('f16', 8): [(520, 528, 0), (512, 512, 0)], ('bf16', 8): [(520, 528, 0), (512, 512, 0)],
                  ('f32', 1): [(67, 67, 0), (256, 260, 1)], ('f64', 1): [(67, 67, 0)], ('f16', 1): [(67, 67, 0)],
                  ('bf16', 1): [(67, 67, 0)]}

NAN_PROTEIN, CONST_A_PROTEIN, CONST_B_PROTEIN = 5, 8, 11   # 95 rows; 129 rows (two parts + whole); 257 rows (three + whole)


@functools.lru_cache(maxsize=2)      # (each is used by one loop of one test; 112 of them would hold 300 MB for the session)
def stage_a_workload(layout, n, wi):
    """Workload of one (memory layout, N, width index): 13 proteins, two layers of kept size [N, 20].  Planted in layer 0:
    a NaN (protein 5, row 50, channel 3), a constant channel 64 VEC - 1 (protein 8) and -- where the width has it -- a
    constant channel 64 VEC (protein 11); layer 1 is left alone, its blocks must not notice."""
    storage, vec = layout
    D, ld, off = STAGE_A_WIDTHS[layout][wi]
    lens, doms = stage_a_lens(n), stage_a_domains(n)
    assert 2 * sum(len(d) for d in doms) >= 64          # fused walks need 64 jobs
    assert len(doms[CONST_A_PROTEIN]) == 3 and len(doms[CONST_B_PROTEIN]) == 4 and len(doms[NAN_PROTEIN]) > 1
    ch_a, ch_b = 64 * vec - 1, 64 * vec
    planted = {(0, CONST_A_PROTEIN): (ch_a,)}
    if ch_b < D:
        planted[(0, CONST_B_PROTEIN)] = (ch_b,)

    def fill(layers):
        layers[0][NAN_PROTEIN][50, 3] = np.nan
        layers[0][CONST_A_PROTEIN][:, ch_a] = 0.5
        if ch_b < D:
            layers[0][CONST_B_PROTEIN][:, ch_b] = -1.25

    w = _finish(f'stage_a_{storage}x{vec}_n{n}_D{D}', storage, n, 20, D, ld, off, lens, doms,
                100_000 * (1 + LAYOUTS.index(layout)) + 1000 * n + 100 * wi, fill, planted)
    first = np.cumsum([0] + [len(d) for d in doms])
    zero = [(int(first[s]) + k, 0) for (_, s) in planted for k in range(len(doms[s]))]
    for k, dom in enumerate(doms[NAN_PROTEIN]):           # the domains that hold row 50 (1-based 51)
        if any(b < 51 <= e for b, e in orc.split_domain(dom, lens[NAN_PROTEIN])[0]):
            zero.append((int(first[NAN_PROTEIN]) + k, 0))
    w.zero_blocks = sorted(zero)
    w.degenerate = sum(len(doms[s]) for (_, s) in planted)
    assert len(w.zero_blocks) == w.degenerate + 2         # (the NaN: a part and the whole protein)
    return w


# -- stage B
STAGE_B_N = (2, 3, 5, 8)
STAGE_B_M = {1: (2, 16), 2: (17, 32), 3: (33, 48), 4: (49, 64), 5: (65, 80), 6: (81, 96), 7: (97, 112), 8: (113, 128)}


@functools.lru_cache(maxsize=None)
def stage_b_workload(n, m, D=131):
    """27 whole proteins of 12 .. 40 rows, one float32 layer of width 131 (Y' rows of 160: slabs of 64 / 64 / 3
    channels; D = 99: the slab kernel's 4-way unrolled tail, 35 channels) -- 27 n rows are no multiple of 16."""
    lens = [12 + (s * 11) % 29 for s in range(27)]
    assert min(lens) == 12 and max(lens) == 40 and (27 * n) % 16 != 0
    doms = [[f'1-{L}'] for L in lens]
    w = _finish(f'stage_b_n{n}_m{m}_D{D}', 'f32', n, m, D, D, 0, lens, doms, 2_000_000 + 1000 * n + m + 7 * D,
                lambda layers: None, {}, n_layers=1)
    w.zero_blocks, w.degenerate = [], 0
    return w


# -- the row split
@functools.lru_cache(maxsize=None)
def split_workload():
    """3 proteins of 150 / 300 / 420 rows, float32, D = 260, [3, 80] twice: per protein a discontinuous domain whose piece
    boundary (job row 50) falls inside a row chunk (chunks are multiples of 32 rows), a domain of 40 rows -- the chunk size
    follows the longest job, so its later chunks are empty -- and the whole protein."""
    lens = [150, 300, 420]
    doms = [[f'1-50,81-{L}', '61-100', f'1-{L}'] for L in lens]
    jobs = 2 * sum(len(d) for d in doms)
    rows = [sum(e - b for b, e in orc.split_domain(dom, L)[0]) for L, ds in zip(lens, doms) for dom in ds]
    assert jobs * 2 < 128 and sum(rows) // len(rows) >= 128 and 50 % 32 != 0      # 2 slabs of 256 channels at ldy = 288
    w = _finish('split', 'f32', 3, 80, 260, 260, 0, lens, doms, 3_000_000, lambda layers: None, {})
    w.zero_blocks, w.degenerate = [], 0
    return w


# -- stage_a_waves' branches ("a_waves" = 0)
#: name -> (memory layout, N, D, rows per protein, proteins, copies of the whole-protein domain, the build the comments promise)
AUTO_WAVES = {
    'short_rows_2': (('f32', 4), 2, 260, 100, 6, 1, Build('f32', 2, 4, 2, 4, False)),
    'mid_rows_4': (('f32', 1), 3, 67, 200, 4, 1, Build('f32', 3, 1, 4, 4, False)),
    'long_rows_8_vec1': (('f32', 1), 3, 67, 330, 3, 1, Build('f32', 3, 1, 8, 4, False)),
    'long_rows_8_full_chip': (('f32', 4), 2, 260, 330, 1, 64, Build('f32', 2, 4, 8, 4, False)),
    'small_call_16': (('f32', 4), 2, 260, 150, 3, 1, Build('f32', 2, 4, 16, 8, False)),
    'vec8_at_most_4': (('f16', 8), 2, 520, 330, 3, 1, Build('f16', 2, 8, 4, 4, False)),
}


@functools.lru_cache(maxsize=None)
def auto_waves_workload(name):
    layout, n, D, L, n_prot, copies, _ = AUTO_WAVES[name]
    lens = [L] * n_prot
    doms = [[f'1-{L}'] * copies for _ in lens]
    w = _finish(f'auto_{name}', layout[0], n, 20, D, D, 0, lens, doms, 4_000_000 + 100 * list(AUTO_WAVES).index(name),
                lambda layers: None, {})
    w.zero_blocks, w.degenerate = [], 0
    return w


# ---- onto the GPU -------------------------------------------------------------------------------------------------------
def to_device(w, dd):
    """(layer batches, piece table) of a workload: per layer one (rows, ld) buffer of the storage type, the proteins back
    to back in the columns [col_off, col_off + D)."""
    import torch
    dt = {'f32': torch.float32, 'f64': torch.float64, 'f16': torch.float16, 'bf16': torch.bfloat16}[w.storage]
    first = np.cumsum([0] + w.lens)
    lbs = []
    for layer in w.layers:
        buf = torch.full((int(first[-1]), w.ld), 7.0, dtype=dt)
        buf[:, w.col_off:w.col_off + w.D] = torch.from_numpy(np.concatenate(layer, axis=0)).to(dt)
        view = buf.cuda()[:, w.col_off:w.col_off + w.D]
        lbs.append(dd.LayerBatch(view, w.n, w.m, row_offsets=first[:-1]))
    return lbs, dd.PieceTable(w.lens, w.doms)
