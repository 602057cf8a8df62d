"""Every stage-A and stage-B build of the two-kernel path, by name: each call asks the library which instantiation it launched
("last_stage_a" / "last_stage_b", written by the launchers from their template arguments), compares that with the hand-written
table of tests/stage_ladder.py, and compares the int8 rows with the float64 oracle's -- bit-exact, on inputs that hold no tie
(tests/test_stage_ladder_host.py).  Experiments context, "path" = 1."""

import numpy as np
import pytest

import stage_ladder as sl

pytestmark = pytest.mark.gpu

OPTIONS = ('path', 'a_waves', 'fuse', 'small_b_jobs', 'pack_y')


@pytest.fixture(scope='module')
def dd():
    import torch
    assert torch.cuda.is_available()
    import dctdomain_amd
    return dctdomain_amd


@pytest.fixture
def ctx(dd):
    """The experiments context on the two-kernel path; every option a test may set is put back afterwards."""
    import torch
    from dctdomain_amd import _lib
    c = _lib.experiments_context(torch.cuda.current_device())
    saved = {k: c.get_option(k) for k in OPTIONS}
    try:
        c.set_option('path', 1)
        yield c
    finally:
        for k, v in saved.items():
            c.set_option(k, v)


def run(dd, ctx, w, dev, **opts):
    """One call of workload `w` (dev = sl.to_device(w)) under `opts` -> (rows, last_stage_a, last_stage_b, constant channels
    the call counted).  The rows are compared with the oracle's here: every call of this file ends in that."""
    for k in OPTIONS[1:]:
        ctx.set_option(k, opts.get(k, {'a_waves': 0, 'fuse': 1, 'small_b_jobs': 512, 'pack_y': 1}[k]))
    ctx.set_option('degenerate_channels', 0)
    lbs, table = dev
    out = dd.quantize_batch(lbs, table, ctx=ctx).cpu().numpy().astype(np.int64)
    assert ctx.get_option('last_path') == 1
    a, b = sl.decode_stage_a(ctx.get_option('last_stage_a')), sl.decode_stage_b(ctx.get_option('last_stage_b'))
    assert a is not None and b is not None, (w, opts)
    np.testing.assert_array_equal(out, w.expected, err_msg=f'{w} {opts} {a} {b}')
    return out, a, b, ctx.get_option('degenerate_channels')


@pytest.mark.parametrize('layout', sl.LAYOUTS, ids=[f'{s}x{v}' for s, v in sl.LAYOUTS])
def test_stage_a_builds(dd, ctx, layout):
    """N = 2 .. 8 x every "a_waves" request x fused or not on one domain list per (N, width): the build the library names is
    the table's entry for the request (the clamps of the wave count and the 8 rows in flight of the unfused 16-wave builds
    included), the rows are the oracle's, the planted blocks are 0 and counted, and at the end every reachable build of the
    layout has run and none of the unreachable ones."""
    seen = set()
    for n in sl.N_RANGE:
        for wi in range(len(sl.STAGE_A_WIDTHS[layout])):
            w = sl.stage_a_workload(layout, n, wi)
            dev = sl.to_device(w, dd)
            # (78 jobs: stage B over slabs unless "small_b_jobs" = 0; Y' is packed for N = 3 on the MFMA stage B only)
            forms = [dict()] + ([dict(small_b_jobs=0, pack_y=0), dict(small_b_jobs=0, pack_y=1)] if n == 3 else [])
            for form in forms:
                for a_waves in sl.A_WAVES:
                    for fuse in (0, 1):
                        opts = dict(form, a_waves=a_waves, fuse=fuse)
                        out, a, b, degenerate = run(dd, ctx, w, dev, **opts)
                        packed = form.get('pack_y') == 1
                        assert sl.Build(*a[:6]) == sl.expected_build(layout, n, a_waves, bool(fuse)), (w, opts, a)
                        assert (a.packed, a.split) == (packed, False), (w, opts, a)
                        assert b == (sl.StageB(sl.MFMA, 2, packed, False, False) if form else
                                     sl.StageB(sl.SLAB, 0, False, False, False)), (w, opts, b)
                        for row, li in w.zero_blocks:
                            assert not out[row, li * n * 20:(li + 1) * n * 20].any(), (w, opts, row, li)
                        assert degenerate == w.degenerate, (w, opts)
                        seen.add(sl.Build(*a[:6]))
    assert not seen & sl.builds_of_layout(layout, reachable=False)
    assert seen == sl.builds_of_layout(layout)


@pytest.mark.parametrize('name', list(sl.AUTO_WAVES))
def test_stage_a_auto_waves(dd, ctx, name):
    """"a_waves" = 0: one call per branch of stage_a_waves -- mean rows below 160 -> 2 waves, 160 .. 319 -> 4, from 320 -> 8 (at
    4 channels per lane only with 256 workgroups or more: below that and from 128 rows the small-call rule -> 16 waves, 8 rows
    in flight), 8 channels per lane -> at most 4."""
    w = sl.auto_waves_workload(name)
    _, a, b, _ = run(dd, ctx, w, sl.to_device(w, dd))
    assert sl.Build(*a[:6]) == sl.AUTO_WAVES[name][-1], (w, a)
    assert not a.packed and not a.split and b == sl.StageB(sl.SLAB, 0, False, False, False)


def test_stage_a_split_forms(dd, ctx):
    """The row split (stage_a_split_kernel) and the three ways it is finished: the slab stage B reading the partial sums, and
    the combine kernel writing packed or unpacked Y' for the MFMA stage B."""
    w = sl.split_workload()
    dev = sl.to_device(w, dd)
    split = sl.StageA('f32', 3, 4, 8, 4, False, False, True)
    _, a, b, _ = run(dd, ctx, w, dev)
    assert a == split and b == sl.StageB(sl.SLAB_FROM_SPLIT, 0, False, False, False)
    _, a, b, _ = run(dd, ctx, w, dev, small_b_jobs=0)
    assert a == split and b == sl.StageB(sl.MFMA, 5, True, True, True)
    _, a, b, _ = run(dd, ctx, w, dev, small_b_jobs=0, pack_y=0)
    assert a == split and b == sl.StageB(sl.MFMA, 5, False, True, False)


@pytest.mark.parametrize('nt', list(sl.STAGE_B_M))
def test_stage_b_builds(dd, ctx, nt):
    """Both ends of the kept columns of an NT (16 nt - 15 and 16 nt; 2 for the first) at n = 2, 3, 5, 8: the slab form, the
    unpacked MFMA build (n = 3: with "pack_y" = 0) and, at n = 3, the packed one."""
    for m in sl.STAGE_B_M[nt]:
        for n in sl.STAGE_B_N:
            w = sl.stage_b_workload(n, m)
            dev = sl.to_device(w, dd)
            _, a, b, _ = run(dd, ctx, w, dev)
            assert b == sl.StageB(sl.SLAB, 0, False, False, False), (w, b)
            assert sl.Build(*a[:6]) == sl.Build('f32', n, 1, 2 if n < 4 else 4, 4, False) and not a.packed and not a.split
            for pack_y in ((0, 1) if n == 3 else (1,)):
                _, a, b, _ = run(dd, ctx, w, dev, small_b_jobs=0, pack_y=pack_y)
                packed = n == 3 and pack_y == 1
                assert b == sl.StageB(sl.MFMA, nt, packed, False, False), (w, pack_y, b)
                assert a.packed == packed


def test_stage_b_slab_tail(dd, ctx):
    """D = 99: the second slab of the slab kernel holds 35 channels -- eight rounds of its 4-way unrolled loop and a tail of 3."""
    w = sl.stage_b_workload(3, 33, 99)
    _, a, b, _ = run(dd, ctx, w, sl.to_device(w, dd))
    assert b == sl.StageB(sl.SLAB, 0, False, False, False)
