"""tests/stage_ladder.py without a GPU: the arithmetic of the hand-written table of stage-A builds, the decoders of the two option
words, and the conditions on the inputs of tests/test_stage_ladder_gpu.py -- checked by the oracle alone, so that no
difference found on the GPU can be argued away as a tie or as a degenerate channel nobody planted."""

import numpy as np
import pytest

import stage_ladder as sl
from oracle import dct_oracle as orc


def test_table_arithmetic():
    """188 instantiations, 12 of them unreachable, none twice; the counts of the table's rows."""
    assert len(sl.BUILDS) == 188
    assert len(set(sl.BUILDS)) == 188          # (a dict: the builder asserts on a repeated key)
    unreachable = {b for b, why in sl.BUILDS.items() if why is not None}
    assert len(unreachable) == 12
    assert unreachable == {sl.Build(s, 3, 4, w, 8 if w == 16 else 4, False) for s in ('f16', 'bf16') for w in (2, 4, 8, 16)} | \
        {sl.Build(s, 3, 8, w, 4, True) for s in ('f16', 'bf16') for w in (2, 4)}
    assert all(why.startswith('UNREACHABLE') for why in sl.BUILDS.values() if why is not None)
    count = lambda storage, vec: sum(1 for b in sl.BUILDS if b.storage == storage and b.vec == vec)
    assert count('f32', 4) == 2 * 4 * 2 + 5 * 2
    for storage, vec in (('f32', 1), ('f64', 2), ('f64', 1), ('f16', 1), ('bf16', 1)):
        assert count(storage, vec) == 2 * 3 * 2 + 5 * 2
    for storage in ('f16', 'bf16'):
        assert count(storage, 8) == 2 * 2 * 2 + 5 * 2
        assert count(storage, 4) == 4 * 2
    # 8 rows in flight: the unfused 16-wave builds and nothing else; 16 waves at 4 channels per lane only
    assert all((b.unroll == 8) == (b.waves == 16 and not b.fused) for b in sl.BUILDS)
    assert all(b.vec == 4 and b.n in (2, 3) for b in sl.BUILDS if b.waves == 16)
    assert all(b.waves == 4 for b in sl.BUILDS if b.n >= 4)
    # the memory layouts share the table out among themselves: every build belongs to exactly one layout
    owners = {b: [lay for lay in sl.LAYOUTS if b in sl.builds_of_layout(lay) | sl.builds_of_layout(lay, reachable=False)]
              for b in sl.BUILDS}
    assert all(len(v) == 1 for v in owners.values())
    assert sum(len(sl.builds_of_layout(lay)) for lay in sl.LAYOUTS) == 176


def test_requests_end_in_reachable_builds():
    """Every ("a_waves", fuse) request on every layout ends in a reachable build of the table, and the requests of a layout
    cover its reachable builds: what the GPU test asserts at the end of a parameter can hold."""
    for layout in sl.LAYOUTS:
        got = {sl.expected_build(layout, n, aw, fused) for n in sl.N_RANGE for aw in sl.A_WAVES for fused in (False, True)}
        assert got == sl.builds_of_layout(layout), layout
        assert all(sl.BUILDS[b] is None for b in got)
    assert [sl.waves_for(r, 4, 3) for r in sl.A_WAVES] == [2, 4, 8, 16]
    assert [sl.waves_for(r, 1, 2) for r in sl.A_WAVES] == [2, 4, 8, 8]
    assert [sl.waves_for(r, 2, 3) for r in sl.A_WAVES] == [2, 4, 8, 8]
    assert [sl.waves_for(r, 8, 2) for r in sl.A_WAVES] == [2, 4, 4, 4]
    assert [sl.waves_for(r, v, n) for r in sl.A_WAVES for v in (1, 2, 4, 8) for n in (4, 8)] == [4] * 32
    assert sl.expected_build(('f32', 4), 3, 16, False) == sl.Build('f32', 3, 4, 16, 8, False)
    assert sl.expected_build(('f32', 4), 3, 16, True) == sl.Build('f32', 3, 4, 16, 4, True)
    assert sl.expected_build(('bf16', 8), 3, 16, True) == sl.Build('bf16', 3, 4, 16, 4, True)
    assert sl.expected_build(('bf16', 8), 3, 16, False) == sl.Build('bf16', 3, 8, 4, 4, False)
    assert sl.expected_build(('f16', 8), 5, 2, True) == sl.Build('f16', 5, 8, 4, 4, True)


def test_option_words_decode():
    """The layout include/dctfp.h documents: one byte per field."""
    assert sl.decode_stage_a(0) is None and sl.decode_stage_b(0) is None
    word = 1 | 3 << 8 | 4 << 16 | 16 << 24 | 8 << 32
    assert sl.decode_stage_a(word) == sl.StageA('f32', 3, 4, 16, 8, False, False, False)
    word = 4 | 8 << 8 | 8 << 16 | 4 << 24 | 4 << 32 | 1 << 40
    assert sl.decode_stage_a(word) == sl.StageA('bf16', 8, 8, 4, 4, True, False, False)
    word = 2 | 3 << 8 | 2 << 16 | 8 << 24 | 4 << 32 | 3 << 40
    assert sl.decode_stage_a(word) == sl.StageA('f64', 3, 2, 8, 4, True, True, False)
    word = 1 | 3 << 8 | 4 << 16 | 8 << 24 | 4 << 32 | 4 << 40
    assert sl.decode_stage_a(word) == sl.StageA('f32', 3, 4, 8, 4, False, False, True)
    assert sl.decode_stage_b(2) == sl.StageB(sl.SLAB, 0, False, False, False)
    assert sl.decode_stage_b(3) == sl.StageB(sl.SLAB_FROM_SPLIT, 0, False, False, False)
    assert sl.decode_stage_b(1 | 5 << 8 | 7 << 16) == sl.StageB(sl.MFMA, 5, True, True, True)
    assert sl.decode_stage_b(1 | 8 << 8 | 2 << 16) == sl.StageB(sl.MFMA, 8, False, True, False)
    with pytest.raises(AssertionError):
        sl.decode_stage_a(5)
    with pytest.raises(AssertionError):
        sl.decode_stage_b(4)


def _check_conditions(w):
    """What every workload promises, from its own fields."""
    assert w.margin >= sl.TIE_MARGIN, w
    assert w.expected.shape == (w.n_domains, len(w.layers) * w.n * w.m)
    assert w.expected.min() >= 0 and w.expected.max() <= 127
    for (row, li) in w.zero_blocks:
        assert not w.expected[row, li * w.n * w.m:(li + 1) * w.n * w.m].any(), (w, row, li)
    # every block that is not planted holds a 0 and a 127 in each of its n rows: nothing else is degenerate
    blocks = w.expected.reshape(w.n_domains, len(w.layers), w.n, w.m)
    for row in range(w.n_domains):
        for li in range(len(w.layers)):
            if (row, li) not in w.zero_blocks:
                assert (blocks[row, li].max(axis=1) == 127).all() and (blocks[row, li].min(axis=1) == 0).all(), (w, row, li)


@pytest.mark.parametrize('layout', sl.LAYOUTS, ids=[f'{s}x{v}' for s, v in sl.LAYOUTS])
def test_stage_a_inputs(layout):
    storage, vec = layout
    esz, margins = sl.ESIZE[storage], []
    widths = sl.STAGE_A_WIDTHS[layout]
    if vec > 1:   # a few channels into the second slab with 16 bytes of padding per row, and exactly one slab
        assert [(D, ld - D, off) for D, ld, off in widths] == [(64 * vec + 16 // esz, 16 // esz, 0), (64 * vec, 0, 0)]
    else:         # the reasons of rows_aligned16: the leading dimension and the width (D = 67), the pointer (the shifted view)
        assert widths[0] == (67, 67, 0) and (67 * esz) % 16 != 0 and 67 % (16 // esz) != 0
        for D, ld, off in widths[1:]:
            assert (ld * esz) % 16 == 0 and D % (16 // esz) == 0 and (off * esz) % 16 != 0 and off + D <= ld
    assert sum(len(sl.STAGE_A_WIDTHS[lay]) == 2 for lay in sl.LAYOUTS if lay[1] == 1) == 1
    for n in sl.N_RANGE:
        for wi, (D, ld, off) in enumerate(widths):
            w = sl.stage_a_workload(layout, n, wi)
            margins.append(w.margin)
            assert (w.D, w.ld, w.col_off, w.n, w.m, len(w.layers)) == (D, ld, off, n, 20, 2)
            assert w.lens == [n, n + 1, 31, 40, 64, 95, 127, 128, 129, 140, 200, 257, 300]
            assert 2 * w.n_domains >= 64
            n_disc = 0
            for L, ds in zip(w.lens, w.doms):
                assert ds[-1] == f'1-{L}'
                if L < 3 * n + 3:
                    assert ds == [f'1-{L}']
                    continue
                assert len(ds) in (3, 4)
                pieces = sorted(p for dom in ds[:-1] for p in orc.split_domain(dom, L)[0])
                assert pieces[0][0] == 0 and pieces[-1][1] == L
                assert all(a[1] == b[0] for a, b in zip(pieces, pieces[1:]))      # the parts tile the protein
                assert all(sum(e - b for b, e in orc.split_domain(dom, L)[0]) >= n for dom in ds)
                first = orc.split_domain(ds[0], L)[0]
                if len(first) == 2:
                    assert first[0][0] > first[1][1] and first[1][0] == 0 and first[0][1] == L   # 'c-d,a-b': last + first
                    n_disc += 1
            assert n_disc == 1
            x = w.layers[0]
            assert np.isnan(x[sl.NAN_PROTEIN]).sum() == 1 and all(np.isfinite(y).all() for y in w.layers[1])
            ch_a, ch_b = 64 * vec - 1, 64 * vec
            assert (x[sl.CONST_A_PROTEIN][:, ch_a] == 0.5).all() and w.planted[(0, sl.CONST_A_PROTEIN)] == (ch_a,)
            assert ((0, sl.CONST_B_PROTEIN) in w.planted) == (ch_b < D)
            if ch_b < D:
                assert (x[sl.CONST_B_PROTEIN][:, ch_b] == -1.25).all()
            assert w.degenerate == (7 if ch_b < D else 3)
            if storage in ('f16', 'bf16'):          # the values are the storage type's
                for y in x:
                    assert y.dtype == np.float32 and (sl.round_to_storage(np.nan_to_num(y), storage) == np.nan_to_num(y)).all()
            else:
                assert all(y.dtype == (np.float64 if storage == 'f64' else np.float32) for y in x)
            _check_conditions(w)
            if n == 3 and wi == 0:                   # the expected rows are orc.quantize_matrix's, row for row
                row = 0
                for s, L in enumerate(w.lens):
                    for dom in w.doms[s]:
                        q = orc.quantize_matrix([layer[s] for layer in w.layers], [dom], [n, 20, n, 20])
                        np.testing.assert_array_equal(w.expected[row], q[orc.split_domain(dom, L)[1]], err_msg=f'{w} {dom}')
                        row += 1
    print(f'{storage}x{vec}: closest 127 Z to an integer {min(margins):.3g}')


def test_stage_b_split_and_auto_inputs():
    margins = []
    assert sorted(m for ms in sl.STAGE_B_M.values() for m in ms) == [2, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 96, 97, 112, 113, 128]
    assert all((ms[0] + 15) // 16 == nt == (ms[1] + 15) // 16 and ms[1] == 16 * nt for nt, ms in sl.STAGE_B_M.items())
    for n in sl.STAGE_B_N:
        for ms in sl.STAGE_B_M.values():
            for m in ms:
                w = sl.stage_b_workload(n, m)
                assert len(w.lens) == 27 == w.n_domains and len(w.layers) == 1 and (27 * n) % 16 != 0
                assert (w.D, (w.D + 31) // 32 * 32, w.D - 128) == (131, 160, 3)
                _check_conditions(w)
                margins.append(w.margin)
    w = sl.stage_b_workload(3, 33, 99)
    assert w.D - 64 == 35 and 35 % 4 == 3
    _check_conditions(w)
    w = sl.split_workload()
    assert (w.n, w.m, w.D, w.storage, len(w.layers)) == (3, 80, 260, 'f32', 2)
    rows = [sum(e - b for b, e in orc.split_domain(dom, L)[0]) for L, ds in zip(w.lens, w.doms) for dom in ds]
    assert 2 * len(rows) * 2 < 128 and sum(rows) // len(rows) >= 128 and min(rows) == 40 and all(150 <= L <= 420 for L in w.lens)
    _check_conditions(w)
    q = orc.quantize_matrix([layer[1] for layer in w.layers], w.doms[1], [3, 80, 3, 80])
    for k, dom in enumerate(w.doms[1]):
        np.testing.assert_array_equal(w.expected[3 + k], q[dom])
    margins.append(w.margin)
    for name in sl.AUTO_WAVES:
        w = sl.auto_waves_workload(name)
        _check_conditions(w)
        margins.append(w.margin)
    print(f'closest 127 Z to an integer {min(margins):.3g}')
