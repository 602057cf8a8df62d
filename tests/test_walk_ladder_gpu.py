"""Every build of the two one-launch kernels, by name: each call asks the library which instantiation it launched ("last_walk" /
"last_gen", written by the launchers of csrc/k_walk.hip / csrc/k_gen.hip from their template arguments), compares that with the
hand-written tables and rules of tests/walk_ladder.py, and compares the int8 rows with the float64 oracle's -- bit-exact, on
inputs that hold no tie (tests/test_walk_ladder_host.py).  Product context, "path" = 2.

A ladder call has 82 .. 106 jobs and the chip holds 256 workgroups or more at once, so run_length (csrc/dctfp.hip) gives every
plain call ONE job per workgroup: its walk_ab_kernel flushes groups of one job, and a walk_gen_kernel named with two Y' slots
never writes its second.  The word says what was launched, not what was used.  Several jobs per workgroup -- flush groups of
2 .. 4 jobs, several flushes, a loop over jobs, the second slot -- are the two tests at the end of this file, which set
"ab_run_jobs" on the experiments context."""

import numpy as np
import pytest

import walk_ladder as wl

pytestmark = pytest.mark.gpu

OPTIONS = ('path', 'fuse', 'gen_fuse')


@pytest.fixture(scope='module')
def dd():
    import torch
    assert torch.cuda.is_available()
    import dctdomain_amd
    return dctdomain_amd


def _forced(c, extra=()):
    """Context `c` with "path" = 2; every option this file sets is put back afterwards.  The counter "degenerate_channels" cannot
    be put back to what it was: the library lets it be reset to 0 and nothing else (dctfp_set_option), so 0 is where it is left."""
    saved = {k: c.get_option(k) for k in OPTIONS + tuple(extra)}
    try:
        c.set_option('path', 2)
        yield c
    finally:
        for k, v in saved.items():
            c.set_option(k, v)
        c.set_option('degenerate_channels', 0)


@pytest.fixture
def ctx(dd):
    import torch
    yield from _forced(dd.get_context(torch.cuda.current_device()))


@pytest.fixture
def xctx(dd):
    import torch
    from dctdomain_amd import _lib
    yield from _forced(_lib.experiments_context(torch.cuda.current_device()), ('ab_run_jobs',))


def check(ctx, w, out, opts, walk=None, gen=None):
    """What every call of this file ends in: a one-launch kernel ran, it is the build (for the general kernel: with the waves and
    the slots) the table promises, the older options agree with the word, the rows are the oracle's, the planted blocks are 0
    and the constant channel is counted once per job that holds it.  Returns the build."""
    out = out.cpu().numpy().astype(np.int64)
    assert ctx.get_option('last_path') == 2, (w, opts)
    got_walk, got_gen = wl.decode_walk(ctx.get_option('last_walk')), wl.decode_gen(ctx.get_option('last_gen'))
    assert (got_walk, got_gen) == (walk, gen), (w, opts, got_walk, got_gen)
    assert ctx.get_option('last_stage_a') == 0 and ctx.get_option('last_stage_b') == 0
    assert ctx.get_option('last_walk_groups') == (walk.nt if walk else 0), (w, opts)
    assert ctx.get_option('last_gen_fused') == (1 if gen and gen.build.fused else 0), (w, opts)
    np.testing.assert_array_equal(out, w.expected, err_msg=f'{w} {opts} {walk or gen}')
    for row, li in w.zero_blocks:
        assert not out[row, li * w.n * w.m:(li + 1) * w.n * w.m].any(), (w, opts, row, li)
    assert ctx.get_option('degenerate_channels') == w.degenerate, (w, opts)
    return walk or gen.build


def call(dd, ctx, dev, **opts):
    for k, v in opts.items():
        ctx.set_option(k, v)
    ctx.set_option('degenerate_channels', 0)
    lbs, table = dev
    return dd.quantize_batch(lbs, table, ctx=ctx)


@pytest.mark.parametrize('s', wl.WALK_S)
@pytest.mark.parametrize('storage', wl.WALK_STORAGES)
def test_walk_builds(dd, ctx, storage, s):
    """walk_ab_kernel at one wave count on one storage type: three widths x both ends of the kept columns of NT 5 (float32: and of
    NT 6), each workload fused ("fuse" = 1: parts + whole protein, 102 jobs) and plain ("fuse" = 0) on the same device buffers."""
    seen = set()
    for D, m in wl.walk_cases(storage, s):
        w = wl.walk_workload(storage, D, m)
        dev = wl.to_device(w, dd)
        for fuse in (1, 0):
            out = call(dd, ctx, dev, fuse=fuse)
            seen.add(check(ctx, w, out, dict(fuse=fuse), walk=wl.expected_walk(storage, D, m, bool(fuse))))
    assert not seen & wl.walk_builds_of(storage, s, reachable=False)
    assert seen == wl.walk_builds_of(storage, s)


@pytest.mark.parametrize('s', wl.WALK_S)
def test_walk_two_source_builds(dd, ctx, s):
    """The two-source builds (dctfp_quantize_windows: rows two windows share are averaged in the row load) at one wave count:
    sequences of two windows of 201 .. 260 rows, domain lists whose cuts fall on and inside the shared rows, fused and plain."""
    from dctdomain_amd.batch import quantize_windows
    seen = set()
    for D, m in wl.WINDOW_CASES[s]:
        w = wl.window_workload(D, m)
        lbs, win_rows, counts, table = wl.windows_to_device(w, dd)
        for fuse in (1, 0):
            ctx.set_option('fuse', fuse)
            ctx.set_option('degenerate_channels', 0)
            out = quantize_windows(lbs, win_rows, counts, table, ctx=ctx, fallback=False)
            seen.add(check(ctx, w, out, dict(fuse=fuse), walk=wl.expected_walk('f32', D, m, bool(fuse), windows=True)))
    assert seen == wl.walk_builds_of('f32', s, win=True)


@pytest.mark.parametrize('n', wl.GEN_N)
@pytest.mark.parametrize('layout', wl.GEN_LAYOUTS, ids=[f'{s}x{v}' for s, v in wl.GEN_LAYOUTS])
def test_gen_builds(dd, ctx, layout, n):
    """walk_gen_kernel at one N on one memory layout: per NTC both ends of its kept columns at one wave, at the widest the plain
    build allows and (N <= 5) at the widest the FUSED build allows; each workload with fused walks asked for ("gen_fuse" = 1:
    the FUSED build up to N = 5 and ten waves, the plain one beyond) and not ("gen_fuse" = 0) on the same device buffers."""
    storage, vec = layout
    seen = set()
    for case in wl.gen_cases(layout, n):
        w = wl.gen_workload(layout, n, case)
        dev = wl.to_device(w, dd)
        for gen_fuse in (1, 0):
            out = call(dd, ctx, dev, fuse=1, gen_fuse=gen_fuse)
            want = wl.expected_gen(storage, vec > 1, n, case.m, case.D, bool(gen_fuse))
            seen.add(check(ctx, w, out, dict(gen_fuse=gen_fuse), gen=want))
    assert not seen & wl.gen_builds_of(layout, n, reachable=False)
    assert seen == wl.gen_builds_of(layout, n)


RUN_JOBS = (1, 2, 3, 5)


@pytest.mark.parametrize('s', wl.WALK_S)
@pytest.mark.parametrize('storage', wl.WALK_STORAGES)
def test_walk_flush_groups_that_are_not_full(dd, xctx, storage, s):
    """"ab_run_jobs" = 1, 2, 3, 5 (experiments library): workgroups of that many jobs, flushed in groups of G = 4 -- groups that are
    not full, and with 5 jobs a second flush per workgroup, so that the lds_arrived / lds_done counters of the barrier-free flush
    go round more than once.  The middle width of the wave count at m = 80 (float32: and at m = 96, six column groups), plain and
    fused.  The same workloads, the same names, the same bytes."""
    D = wl.walk_widths(storage, s)[1]
    for m in (80, 96) if storage == 'f32' else (80,):
        w = wl.walk_workload(storage, D, m)
        dev = wl.to_device(w, dd)
        for run_jobs in RUN_JOBS:
            for fuse in (1, 0):
                opts = dict(ab_run_jobs=run_jobs, fuse=fuse)
                out = call(dd, xctx, dev, **opts)
                check(xctx, w, out, opts, walk=wl.expected_walk(storage, D, m, bool(fuse)))


@pytest.mark.parametrize('layout', wl.GEN_LAYOUTS, ids=[f'{s}x{v}' for s, v in wl.GEN_LAYOUTS])
def test_gen_several_jobs_per_workgroup(dd, xctx, layout):
    """"ab_run_jobs" = 2, 5 through walk_gen_kernel: a workgroup loops over its jobs, and where the launch has two Y' slots a wave
    writes the next job's Y' into the second while the last arrival still sums the first.  N = 2, 5, 8 at the widest width of each
    NTC's lower end and at the narrowest of its upper end (between them launches of one and of two slots), fused and plain."""
    storage, vec = layout
    slots = set()
    for n in (2, 5, 8):
        cases = wl.gen_cases(layout, n)
        low, high = [c for c in cases if c.m <= 64], [c for c in cases if c.m > 64]
        for case in (max(low, key=lambda c: (c.D, -c.m)), min(high, key=lambda c: (c.D, -c.m))):
            w = wl.gen_workload(layout, n, case)
            dev = wl.to_device(w, dd)
            for run_jobs in (2, 5):
                for gen_fuse in (1, 0):
                    opts = dict(ab_run_jobs=run_jobs, fuse=1, gen_fuse=gen_fuse)
                    out = call(dd, xctx, dev, **opts)
                    want = wl.expected_gen(storage, vec > 1, n, case.m, case.D, bool(gen_fuse))
                    check(xctx, w, out, opts, gen=want)
                    slots.add(want.slots)
    assert slots == {1, 2}, layout
