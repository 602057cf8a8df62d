"""tests/walk_ladder.py without a GPU: the arithmetic of the two hand-written tables of walk_ab_kernel / walk_gen_kernel builds,
the decoders of the two option words, that the requests of tests/test_walk_ladder_gpu.py end in -- and cover -- the reachable
builds, and the conditions on its inputs, checked by the oracle alone, so that no difference found on the GPU can be argued
away as a tie or as a degenerate channel nobody planted."""

import numpy as np
import pytest

import walk_ladder as wl
from oracle import dct_oracle as orc


def test_table_arithmetic():
    """30 walk_ab_kernel builds and 88 walk_gen_kernel builds, none twice, none unreachable."""
    assert len(wl.WALK_BUILDS) == 30 and len(wl.GEN_BUILDS) == 88
    assert {b for b, why in wl.WALK_BUILDS.items() if why is not None} == set()
    assert {b for b, why in wl.GEN_BUILDS.items() if why is not None} == set()
    walk = lambda **kw: sum(1 for b in wl.WALK_BUILDS if all(getattr(b, k) == v for k, v in kw.items()))
    assert walk(nt=5, win=False) == 3 * 3 * 2              # three storage types x S 3 / 5 / 10 x plain / fused
    assert walk(nt=6) == 6 == walk(nt=6, storage='f32', win=False)
    assert walk(win=True) == 6 == walk(win=True, storage='f32', nt=5)
    assert walk(storage='f64') == 0 and walk(fused=True) == 15
    assert all(b.s in (3, 5, 10) for b in wl.WALK_BUILDS)
    gen = lambda **kw: sum(1 for b in wl.GEN_BUILDS if all(getattr(b, k) == v for k, v in kw.items()))
    for storage, vec in wl.GEN_LAYOUTS:
        assert gen(storage=storage, vec=vec) == (7 + 4) * 2
        assert gen(storage=storage, vec=vec, fused=True) == 4 * 2
    assert gen(ntc=4) == gen(ntc=8) == 44
    assert all(b.n <= wl.GEN_FUSED_MAX_N for b in wl.GEN_BUILDS if b.fused)
    assert {(b.storage, b.vec) for b in wl.GEN_BUILDS} == set(wl.GEN_LAYOUTS)
    # the parameters of the GPU test share the tables out among themselves: every build belongs to exactly one
    owned = [b for s in wl.WALK_STORAGES for S in wl.WALK_S for win in (False, True) for b in wl.walk_builds_of(s, S, win)]
    assert len(owned) == 30 == len(set(owned))
    owned = [b for lay in wl.GEN_LAYOUTS for n in wl.GEN_N for b in wl.gen_builds_of(lay, n)]
    assert len(owned) == 88 == len(set(owned))


def test_option_words_decode():
    """The layout include/dctfp.h documents: one byte per field."""
    assert wl.decode_walk(0) is None and wl.decode_gen(0) is None
    assert wl.decode_walk(1 | 3 << 8 | 5 << 16) == wl.WalkBuild('f32', 3, 5, False, False)
    assert wl.decode_walk(4 | 10 << 8 | 5 << 16 | 1 << 24) == wl.WalkBuild('bf16', 10, 5, True, False)
    assert wl.decode_walk(3 | 5 << 8 | 5 << 16) == wl.WalkBuild('f16', 5, 5, False, False)
    assert wl.decode_walk(1 | 5 << 8 | 6 << 16 | 1 << 24) == wl.WalkBuild('f32', 5, 6, True, False)
    assert wl.decode_walk(1 | 3 << 8 | 5 << 16 | 3 << 24) == wl.WalkBuild('f32', 3, 5, True, True)
    assert wl.decode_walk(1 | 3 << 8 | 5 << 16 | 2 << 24) == wl.WalkBuild('f32', 3, 5, False, True)
    word = 1 | 5 << 8 | 4 << 16 | 4 << 24 | 1 << 32 | 5 << 40 | 1 << 48
    assert wl.decode_gen(word) == wl.GenLaunch(wl.GenBuild('f32', 5, 4, 4, True), 5, 1)
    word = 2 | 8 << 8 | 1 << 16 | 8 << 24 | 0 << 32 | 16 << 40 | 2 << 48
    assert wl.decode_gen(word) == wl.GenLaunch(wl.GenBuild('f64', 8, 1, 8, False), 16, 2)
    for bad in (5, 1 | 3 << 8 | 5 << 16 | 4 << 24, 1 | 3 << 8 | 5 << 16 | 1 << 32):
        with pytest.raises(AssertionError):
            wl.decode_walk(bad)
    for bad in (7, 1 | 2 << 8 | 4 << 16 | 4 << 24 | 2 << 32, 1 | 2 << 8 | 4 << 16 | 4 << 24 | 1 << 56):
        with pytest.raises(AssertionError):
            wl.decode_gen(bad)


def test_rules_by_hand():
    """expected_walk / expected_gen on shapes worked out on paper from choose_route, gen_slot_bytes and gen_wg_per_cu."""
    assert [wl.expected_walk('f32', D, 80, False).s for D in (512, 768, 772, 1280, 1284, 2560)] == [3, 3, 5, 5, 10, 10]
    assert [wl.expected_walk('f32', 640, m, True).nt for m in (65, 80, 81, 96)] == [5, 5, 6, 6]
    assert wl.expected_walk('bf16', 1288, 65, True) == wl.WalkBuild('bf16', 10, 5, True, False)
    assert wl.expected_walk('f32', 516, 80, False, windows=True) == wl.WalkBuild('f32', 3, 5, False, True)
    for storage, D, m in (('f16', 516, 80), ('f16', 640, 81), ('f32', 640, 97), ('f32', 508, 80), ('f32', 2564, 80), ('f64', 640, 80),
                          ('f32', 642, 80)):
        assert not wl.is_walk_shape(storage, True, 3, m, D)
        with pytest.raises(AssertionError):
            wl.expected_walk(storage, D, m, False)
    with pytest.raises(AssertionError):
        wl.expected_walk('f32', 640, 85, False, windows=True)
    assert not wl.is_walk_shape('f32', False, 3, 80, 640) and not wl.is_walk_shape('f32', True, 4, 80, 640)
    # [5, 44] at D = 1280: 5 waves of 256 channels, a slot of 5 x 1280 doubles = 51 200 B: two workgroups per CU with one slot, one
    # with two -> one slot; fused.  At D = 2560: ten waves, 102 400 B -> one slot, still fused; at 2816: eleven waves, plain
    assert wl.expected_gen('f32', True, 5, 44, 1280, True) == wl.GenLaunch(wl.GenBuild('f32', 5, 4, 4, True), 5, 1)
    assert wl.expected_gen('f32', True, 5, 44, 2560, True) == wl.GenLaunch(wl.GenBuild('f32', 5, 4, 4, True), 10, 1)
    assert wl.expected_gen('f32', True, 5, 44, 2816, True) == wl.GenLaunch(wl.GenBuild('f32', 5, 4, 4, False), 11, 1)
    assert wl.expected_gen('f32', True, 6, 44, 1280, True).build.fused is False
    # float64 rows [3, 80] at D = 1280: ten waves of 128 channels, 30 720 B: two workgroups per CU by waves either way -> two slots
    assert wl.expected_gen('f64', True, 3, 80, 1280, False) == wl.GenLaunch(wl.GenBuild('f64', 3, 2, 8, False), 10, 2)
    # one channel per lane, [8, 80] at D = 1021: 16 waves; Y' 8 x 1024 doubles + partial blocks 16 x 8 x 80 = 147 456 B: one slot
    assert wl.gen_slot_bytes(8, 80, 16, 1) == 147456 and wl.gen_slot_bytes(8, 64, 16, 1) == 65536
    assert wl.expected_gen('f32', False, 8, 80, 1021, False) == wl.GenLaunch(wl.GenBuild('f32', 8, 1, 8, False), 16, 1)
    assert not wl.gen_fits(8, 81, 16, 1) and not wl.gen_fits(2, 2, 17, 4)
    # [2, 64] at D = 244: one wave, 4 096 B: 20 workgroups per CU by waves with one slot, 18 by LDS with two -> one slot; at
    # D = 4084: 16 waves, 65 536 B: one workgroup per CU either way -> two slots
    assert wl.expected_gen('f32', True, 2, 64, 244, False) == wl.GenLaunch(wl.GenBuild('f32', 2, 4, 4, False), 1, 1)
    assert wl.expected_gen('f32', True, 2, 64, 4084, True) == wl.GenLaunch(wl.GenBuild('f32', 2, 4, 4, False), 16, 2)
    with pytest.raises(AssertionError):
        wl.expected_gen('f32', True, 3, 80, 640, False)          # walk_ab_kernel's own shape


def test_requests_end_in_reachable_builds():
    """Every request of every parameter of the GPU test ends in a reachable build of the tables, and the requests of a parameter
    cover its reachable builds: what the GPU test asserts at the end of a parameter can hold."""
    for storage in wl.WALK_STORAGES:
        for s in wl.WALK_S:
            cases = wl.walk_cases(storage, s)
            assert len(cases) == (12 if storage == 'f32' else 6)
            got = {wl.expected_walk(storage, D, m, fused) for D, m in cases for fused in (False, True)}
            assert got == wl.walk_builds_of(storage, s), (storage, s)
            assert all(wl.WALK_BUILDS[b] is None for b in got)
            widths = wl.walk_widths(storage, s)
            assert any(D % 8 == 4 for D in widths) == (storage == 'f32') and any((D // 2) % 16 for D in widths)
    for s in wl.WALK_S:
        got = {wl.expected_walk('f32', D, m, fused, windows=True) for D, m in wl.WINDOW_CASES[s] for fused in (False, True)}
        assert got == wl.walk_builds_of('f32', s, win=True), s
        assert {m for _, m in wl.WINDOW_CASES[s]} == {65, 80}
    assert all(not wl.walk_builds_of(st, s, win=True) for st in ('f16', 'bf16') for s in wl.WALK_S)
    # the widths are both ends of each wave count
    for fam, first, step in (('f32', 512, 4), ('half', 512, 8)):
        w = wl.WALK_WIDTHS[fam]
        assert (w[3][0], w[3][-1], w[5][0], w[5][-1], w[10][0], w[10][-1]) == (first, 768, 768 + step, 1280, 1280 + step, 2560)
    for layout in wl.GEN_LAYOUTS:
        storage, vec = layout
        slots, branches = set(), set()
        for n in wl.GEN_N:
            cases = wl.gen_cases(layout, n)
            assert len(set(cases)) == len(cases)
            launches = {(c, fused): wl.expected_gen(storage, vec > 1, n, c.m, c.D, fused) for c in cases for fused in (False, True)}
            got = {g.build for g in launches.values()}
            assert got == wl.gen_builds_of(layout, n), (layout, n)
            assert all(wl.GEN_BUILDS[b] is None for b in got)
            assert {c.m for c in cases} >= {2, 64, 65} and all(c.m < c.D for c in cases)
            for c in cases:        # the ends of an NTC: 2 / 65 and 64 / 128, or where walk_shape, the width or the LDS ends before them
                waves = -(-c.D // (64 * vec))
                assert c.m in (2, 65, 64, 128) or c.m == c.D - 1 or not wl.gen_fits(n, c.m + 1, waves, vec) \
                    or wl.is_walk_shape(storage, vec > 1, n, c.m - 1, c.D), (layout, n, c)
            # (one channel per lane at 16 waves: Y' of n x 1024 doubles and 16 partial blocks of n x cp -- 150 KB hold cp = 96 at
            #  n = 7 and 80 at n = 8; everything else reaches 128 at its widest)
            top = {7: 96, 8: 80}.get(n, 128) if vec == 1 else 128
            assert max(c.m for c in cases if c.D == max(k.D for k in cases)) == top, (layout, n)
            for ntc in (4, 8):
                mine = [g for (c, _), g in launches.items() if g.build.ntc == ntc]
                # (4 channels per lane: a wave's Y' rows are 2 KB each -- 5 x 14, 6 x 12, 7 x 10 and 8 x 9 of them are what 150 KB hold)
                widest = {5: 14, 6: 12, 7: 10, 8: 9}.get(n, 16) if layout == ('f32', 4) else 16
                narrow = 2 if (vec, ntc) == (1, 8) else 1      # (a wave of one channel per lane has 64 channels: no room for m >= 65)
                assert min(g.waves for g in mine) == narrow and max(g.waves for g in mine) == widest, (layout, n)
                if n <= wl.GEN_FUSED_MAX_N:      # every FUSED build at its narrowest and at the ten waves it is bounded to
                    fused_waves = {g.waves for g in mine if g.build.fused}
                    assert min(fused_waves) == narrow and max(fused_waves) == wl.GEN_FUSED_MAX_WAVES, (layout, n, ntc)
            for c in cases:
                lanes = -(-c.D // vec)
                assert lanes % 64 == 61 and (vec == 1 or c.D % vec == 0)        # the width ends inside the last wave
                if vec == 1:                                                     # ... and no row is 16-byte aligned
                    esz = wl.ESIZE[storage]
                    assert (c.col_off * esz) % 16 != 0 and c.D % (16 // esz) != 0 and c.col_off + c.D <= c.ld
                else:
                    assert (c.ld, c.col_off) == (c.D, 0)
                branches.add(-(-c.m // 16) * 16 <= 64 * vec)
            slots |= {g.slots for g in launches.values()}
        assert slots == {1, 2}, layout
        assert branches == ({True, False} if vec == 1 else {True}), layout       # `cp <= 64 * VEC` of gen_slot_bytes
    # float32 rows at N = 3, m = 65 .. 96 are walk_ab_kernel's from 512 to 2560 channels: m = 65 goes no wider than two waves fused
    # (and the full 16 plain), the upper end of NTC 8 -- m = 97 .. 128 -- runs the FUSED build at its ten waves
    wide = [c for c in wl.gen_cases(('f32', 4), 3) if c.D == 2548 and c.m > 64]
    assert [c.m for c in wide] == [97, 128] and wl.GenCase(65, 500, 500, 0) in wl.gen_cases(('f32', 4), 3)
    assert wl.expected_gen('f32', True, 3, 97, 2548, True) == wl.GenLaunch(wl.GenBuild('f32', 3, 4, 8, True), 10, 1)


def _check_conditions(w):
    """What every workload promises, from its own fields (as tests/test_stage_ladder_host.py)."""
    assert w.margin >= wl.TIE_MARGIN, w
    assert 2 * w.n_domains >= 64 and any(len(d) > 1 for d in w.doms), w            # the fuse rule
    assert w.expected.shape == (w.n_domains, len(w.layers) * w.n * w.m)
    assert w.expected.min() >= 0 and w.expected.max() <= 127
    for (row, li) in w.zero_blocks:
        assert li == 0 and not w.expected[row, :w.n * w.m].any(), (w, row, li)
    blocks = w.expected.reshape(w.n_domains, len(w.layers), w.n, w.m)
    for row in range(w.n_domains):
        for li in range(len(w.layers)):
            if (row, li) not in w.zero_blocks:
                assert (blocks[row, li].max(axis=1) == 127).all() and (blocks[row, li].min(axis=1) == 0).all(), (w, row, li)
    assert np.isnan(np.concatenate(w.layers[0])).sum() == 1 and all(np.isfinite(x).all() for x in w.layers[1])
    assert w.degenerate > 1 and len(w.zero_blocks) == w.degenerate + 2
    if w.storage in ('f16', 'bf16'):          # the values are the storage type's
        for x in w.layers[0]:
            assert x.dtype == np.float32 and (wl.round_to_storage(np.nan_to_num(x), w.storage) == np.nan_to_num(x)).all()


def test_proteins_and_domain_lists():
    for n in wl.GEN_N:
        lens, doms = wl.ladder_lens(n), wl.ladder_domains(n)
        assert set(lens) >= {n, n + 1, 16, 17, 300} | {L for L in (7, 8, 9) if L >= n} and min(lens) == n
        n_disc, starts = 0, set()
        for L, ds in zip(lens, doms):
            assert ds[-1] == f'1-{L}'
            if L < 3 * n + 3:
                assert ds == [f'1-{L}']
                continue
            pieces = sorted(p for dom in ds[:-1] for p in orc.split_domain(dom, L)[0])
            assert pieces[0][0] == 0 and pieces[-1][1] == L and all(a[1] == b[0] for a, b in zip(pieces, pieces[1:]))
            assert all(sum(e - b for b, e in orc.split_domain(dom, L)[0]) >= n for dom in ds)
            starts |= {b % 2 for b, _ in pieces}
            first = orc.split_domain(ds[0], L)[0]
            if len(first) == 2:
                assert first[0][0] > first[1][1] and first[1][0] == 0 and first[0][1] == L      # 'c-d,a-b': last + first
                n_disc += 1
        assert n_disc == 1 and starts == {0, 1}                  # parts start at even and at odd rows
    for i, (r0, r1) in enumerate(wl.WINDOW_ROWS):
        assert 201 <= r0 <= 260 and 201 <= r1 <= 260
        L, ds = r0 + r1 - 200, wl.window_domains(r0, r1, i)
        pieces = sorted(p for dom in ds[:-1] for p in orc.split_domain(dom, L)[0])
        assert ds[-1] == f'1-{L}' and pieces[0][0] == 0 and pieces[-1][1] == L and all(a[1] == b[0] for a, b in zip(pieces, pieces[1:]))
        assert all(sum(e - b for b, e in orc.split_domain(dom, L)[0]) >= 3 for dom in ds)
    cuts = {(c - (r0 - 200), r0 - c) for i, (r0, r1) in enumerate(wl.WINDOW_ROWS)
            for dom in wl.window_domains(r0, r1, i)[:-1] for c, _ in orc.split_domain(dom, r0 + r1 - 200)[0] if c}
    assert any(a == 0 for a, _ in cuts) and any(b == 0 for _, b in cuts) and any(a > 0 and b > 0 for a, b in cuts)   # on and inside
    assert {r for rows in wl.WINDOW_ROWS for r in rows} >= {201, 260}


@pytest.mark.parametrize('storage', wl.WALK_STORAGES)
def test_walk_inputs(storage):
    margins = []
    for s in wl.WALK_S:
        for D, m in wl.walk_cases(storage, s):
            w = wl.walk_workload(storage, D, m)
            esz = wl.ESIZE[storage]
            assert (w.D, w.n, w.m, w.col_off, len(w.layers)) == (D, 3, m, 0, 2) and (w.ld * esz) % 16 == 0 and D % (16 // esz) == 0
            assert w.lens == wl.ladder_lens(3) and w.planted == {(0, w.lens.index(129)): (D // 2 - 1,)}
            assert np.isnan(w.layers[0][w.lens.index(95)][50, D // 2])
            _check_conditions(w)
            margins.append(w.margin)
            if (D, m) == wl.walk_cases(storage, s)[0]:            # the expected rows are orc.quantize_matrix's, row for row
                row = 0
                for p, L in enumerate(w.lens):
                    for dom in w.doms[p]:
                        q = orc.quantize_matrix([layer[p] for layer in w.layers], [dom], [3, m, 3, m])
                        np.testing.assert_array_equal(w.expected[row], q[orc.split_domain(dom, L)[1]], err_msg=f'{w} {dom}')
                        row += 1
    print(f'{storage}: closest 127 Z to an integer {min(margins):.3g}')


def test_window_inputs():
    import torch
    margins = []
    for s in wl.WALK_S:
        for D, m in wl.WINDOW_CASES[s]:
            w = wl.window_workload(D, m)
            assert len(w.windows) == 2 and [x.shape[0] for x in w.windows[0]] == [r for rows in wl.WINDOW_ROWS for r in rows]
            assert all(x.dtype == np.float32 and x.shape[1] == D for win in w.windows for x in win)
            # overlapping windows disagree on the rows they share, and the stitched rows are their float32 mean
            a, b = w.windows[1][0], w.windows[1][1]
            r0 = wl.WINDOW_ROWS[0][0]
            assert (a[r0 - 200:] != b[:200]).any()
            mean = ((torch.from_numpy(a[r0 - 200:]) + torch.from_numpy(b[:200])) / 2).numpy()
            np.testing.assert_array_equal(w.layers[1][0][r0 - 200:r0], mean)
            _check_conditions(w)
            margins.append(w.margin)
    print(f'windows: closest 127 Z to an integer {min(margins):.3g}')


@pytest.mark.parametrize('layout', wl.GEN_LAYOUTS, ids=[f'{s}x{v}' for s, v in wl.GEN_LAYOUTS])
def test_gen_inputs(layout):
    storage, vec = layout
    margins = []
    for n in wl.GEN_N:
        for case in wl.gen_cases(layout, n):
            w = wl.gen_workload(layout, n, case)
            assert (w.n, w.m, w.D, w.ld, w.col_off, len(w.layers)) == (n, case.m, case.D, case.ld, case.col_off, 2)
            assert w.lens == wl.ladder_lens(n)
            assert all(x.dtype == (np.float64 if storage == 'f64' else np.float32) for x in w.layers[0])
            _check_conditions(w)
            margins.append(w.margin)
    print(f'{storage}x{vec}: closest 127 Z to an integer {min(margins):.3g}')
