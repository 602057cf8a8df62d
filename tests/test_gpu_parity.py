"""GPU parity: the HIP path (through the C ABI, via dctdomain_amd) against the golden vectors
made by the reference itself and against the oracle on seeded inputs.  int8: bit-exact."""

import numpy as np
import pytest

import golden_util as gu
import stage_ladder as sl
import walk_ladder as wl
from oracle import dct_oracle as orc
from recipes import make_input

pytestmark = pytest.mark.gpu

ALL_OK = gu.cases(expect='ok')
ALL_ERR = gu.cases(expect='ValueError')


@pytest.fixture(scope='module')
def dd():
    import torch
    assert torch.cuda.is_available()
    import dctdomain_amd
    return dctdomain_amd


def run_fp(dd, layers, domains, qdim, as_tensor=False):
    import torch
    if as_tensor:
        embed = {i: torch.from_numpy(x).cuda() for i, x in enumerate(layers)}
    else:
        embed = {i: x for i, x in enumerate(layers)}
    fp = dd.Fingerprint(pid='t', seq='A' * layers[0].shape[0], embed=embed, domains=list(domains))
    fp.quantize(list(qdim))
    return fp


@pytest.mark.parametrize('case', ALL_OK, ids=gu.case_ids(ALL_OK))
def test_golden_bit_exact(dd, case):
    layers = gu.build_layers(case)
    fp = run_fp(dd, layers, case['domains'], case['qdim'])
    exp = gu.expected(case)
    assert list(fp.quants.keys()) == case['keys']
    assert fp.domains == case['keys']
    for k in exp:
        assert fp.quants[k].dtype == np.int64
        np.testing.assert_array_equal(fp.quants[k], exp[k].astype(np.int64), err_msg=f"{case['id']} {k}")


@pytest.mark.parametrize('case', ALL_ERR, ids=gu.case_ids(ALL_ERR))
def test_golden_errors(dd, case):
    layers = gu.build_layers(case)
    with pytest.raises(ValueError, match='cannot reshape array'):
        run_fp(dd, layers, case['domains'], case['qdim'])


SUBSET = [c for c in ALL_OK if c['id'].startswith(('two_', 'dom_', 'qdim_', 'contact', 'inline', 'deg_', 'c4_'))]


def walk_eligible(case, layers):
    """The shapes dctfp_quantize hands to walk_ab_kernel when path = 2 (dctfp.hip, "which kernels"): n = 3, 64 < m <= 80,
    float32 rows read 4 channels per lane, 512 <= D <= 2560, no domain above 8192 rows -- judged on the LAST layer group,
    the one `last_path` reports."""
    x, n, m = layers[-1], case['qdim'][-2], case['qdim'][-1]
    return n == 3 and 64 < m <= 96 and x.dtype == np.float32 and 512 <= x.shape[1] <= 2560 and x.shape[1] % 4 == 0 \
        and x.shape[0] <= 8192 and len(case['keys']) > 0


@pytest.mark.parametrize('opts', [dict(), dict(a_waves=8), dict(a_waves=16), dict(a_waves=4),
                                  dict(workspace_mb=16), dict(a_waves=2), dict(overlap=1), dict(fuse=0), dict(pack_y=0),
                                  dict(path=1), dict(path=1, fuse=0), dict(path=2), dict(path=2, ab_run_jobs=4), dict(path=2, ab_run_jobs=64),
                                  dict(path=2, ab_run_jobs=1), dict(small_b_jobs=0), dict(path=1, small_b_jobs=1 << 20)],
                         ids=['default', 'w8', 'w16', 'w4', 'smallws', 'w2', 'nooverlap', 'nofuse', 'nopack',
                              'twokernels', 'twokernels_nofuse', 'walk_forced', 'walk_run4', 'walk_run64', 'walk_run1', 'mfmaB_small_calls', 'slabB_always'])
def test_kernel_variants_agree_with_golden(dd, opts):
    """Every kernel configuration the dispatch can pick (and the engineering knobs can force) against the golden subset.
    The knobs live in libdctfp_experiments.so only (same kernels and dispatch as the product, -DDCTFP_EXPERIMENTS), so this
    test drives that library through the batch API."""
    import torch
    from dctdomain_amd import _lib
    ctx = _lib.experiments_context(torch.cuda.current_device())
    saved = {k: ctx.get_option(k) for k in opts}
    try:
        for k, v in opts.items():
            ctx.set_option(k, v)
        for case in SUBSET:
            layers = gu.build_layers(case)
            qd = case['qdim']
            assert all(x.shape[0] == layers[0].shape[0] for x in layers)
            table = dd.PieceTable([layers[0].shape[0]], [case['domains']])
            lbs = [dd.LayerBatch([torch.from_numpy(x).cuda()], qd[2 * i], qd[2 * i + 1]) for i, x in enumerate(layers)]
            out = dd.quantize_batch(lbs, table, ctx=ctx).cpu().numpy()
            if opts.get('path') == 2 and walk_eligible(case, layers):
                # a one-protein call reaches the walk kernel only when it is forced: make sure it did
                assert ctx.get_option('last_path') == 2, f"{case['id']} did not run walk_ab_kernel under {opts}"
            # quants[key] as Fingerprint.quantize assembles it: layer-major, then domain order; a key that occurs twice
            # (two domain strings cleaned to the same key) is extended twice (src/fingerprint.py:184-196)
            got, off = {}, 0
            for i in range(len(layers)):
                nm = qd[2 * i] * qd[2 * i + 1]
                for row, key in enumerate(table.keys):
                    got.setdefault(key, []).append(out[row, off:off + nm])
                off += nm
            exp = gu.expected(case)
            assert list(got) == case['keys']
            for key in exp:
                np.testing.assert_array_equal(np.concatenate(got[key]).astype(np.int64), exp[key].astype(np.int64),
                                              err_msg=f"{case['id']} {key} {opts}")
    finally:
        for k, v in saved.items():
            ctx.set_option(k, v)


def test_intermediates_within_tolerance(dd):
    """North star: intermediate float coefficients within 1e-5 of the scipy reference."""
    arr = gu.arrays()
    checked = 0
    for case in ALL_OK:
        if not case.get('intermediates'):
            continue
        layers = gu.build_layers(case)
        n, m = case['qdim'][0], case['qdim'][1]
        fp = dd.Fingerprint(pid='t', seq='A' * layers[0].shape[0], embed={0: layers[0]})
        x, key = fp.get_doms(layers[0], case['domains'][0])
        assert x.dtype == np.float64
        xo, ko = orc.get_doms(layers[0], case['domains'][0])
        assert key == ko
        np.testing.assert_array_equal(x, xo)
        coef = fp.dct_coefficients(x, n)
        scale = max(1.0, np.abs(arr[f"{case['id']}/coef"]).max())
        np.testing.assert_allclose(coef, arr[f"{case['id']}/coef"], rtol=0, atol=1e-5)
        assert np.abs(coef - arr[f"{case['id']}/coef"]).max() <= 1e-11 * scale      # what we really get
        yp = fp.idct_quant(x, n)
        np.testing.assert_allclose(yp, arr[f"{case['id']}/Yp"], rtol=0, atol=1e-5)
        assert np.abs(yp - arr[f"{case['id']}/Yp"]).max() <= 1e-9
        z = fp.idct_quant(yp.T, m).T
        np.testing.assert_allclose(z, arr[f"{case['id']}/Z"], rtol=0, atol=1e-5)
        assert np.abs(z - arr[f"{case['id']}/Z"]).max() <= 1e-8
        checked += 1
    assert checked >= 6


def test_scale_and_get_doms_methods(dd):
    import torch
    rng = np.random.default_rng(5)
    fp = dd.Fingerprint()
    for n in (1, 3, 80, 1000, 70001):
        v = rng.standard_normal(n)
        got = fp.scale(v)
        with np.errstate(all='ignore'):
            exp = orc.scale(v)
        np.testing.assert_array_equal(np.isnan(got), np.isnan(exp))
        np.testing.assert_allclose(got[~np.isnan(got)], exp[~np.isnan(exp)], rtol=0, atol=0)
    v = np.array([1.0, np.nan, 3.0])
    assert np.isnan(fp.scale(v)).all()
    assert np.isnan(fp.scale(np.array([2.0, 2.0]))).all()
    t = torch.arange(10, dtype=torch.float64, device='cuda')
    out = fp.scale(t)
    assert isinstance(out, torch.Tensor) and out.is_cuda
    np.testing.assert_allclose(out.cpu().numpy(), np.arange(10) / 9.0, rtol=0, atol=0)
    import json, os
    with open(os.path.join(gu.GOLD, 'getdoms_golden.json')) as fh:
        table = json.load(fh)
    for row in table:
        x = np.arange(row['L'] * 4, dtype=np.float32).reshape(row['L'], 4)
        mat, key = fp.get_doms(x, row['dom'])
        assert key == row['key'], row
        assert mat.dtype == np.float64 and mat.shape[1] == 4
        assert [int(v) for v in (mat[:, 0] / 4).astype(int)] == row['rows'], row


def _oracle_rows(layers_per_seq, domains_per_seq, qdim):
    rows, keys = [], []
    for layers, doms in zip(layers_per_seq, domains_per_seq):
        q = orc.quantize(layers, doms, qdim)
        for k, v in q.items():
            rows.append(v)
            keys.append(k)
    return keys, np.stack(rows).astype(np.int8)


def test_ragged_batch_matches_oracle(dd):
    """Many sequences of different lengths, multi-domain, both batch layouts."""
    import torch
    rng = np.random.default_rng(77)
    D = 640
    lens = [3, 17, 64, 158, 333, 500, 701, 1035, 40, 5]
    layers_per_seq, doms_per_seq = [], []
    for i, L in enumerate(lens):
        layers_per_seq.append([make_input('esm', L, D, 9000 + 2 * i), make_input('esm', L, D, 9001 + 2 * i)])
        doms = [f'1-{L}']
        if L >= 40:
            a = L // 3
            doms = [f'1-{a}', f'{a + 1}-{L}', f'1-{a // 2},{a + 5}-{L - 3}', f'1-{L}']
        doms_per_seq.append(doms)
    keys, exp = _oracle_rows(layers_per_seq, doms_per_seq, [3, 80, 3, 80])
    table = dd.PieceTable(lens, doms_per_seq)
    assert table.keys == keys
    # (a) list of per-sequence tensors
    lt = [[torch.from_numpy(ls[k]).cuda() for ls in layers_per_seq] for k in range(2)]
    out = dd.quantize_batch([dd.LayerBatch(lt[0], 3, 80), dd.LayerBatch(lt[1], 3, 80)], table)
    np.testing.assert_array_equal(out.cpu().numpy(), exp)
    # (b) one concatenated tensor per layer + row offsets
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    cat = [torch.cat(lt[k], dim=0) for k in range(2)]
    out2 = dd.quantize_batch([dd.LayerBatch(cat[0], 3, 80, row_offsets=offs),
                              dd.LayerBatch(cat[1], 3, 80, row_offsets=offs)], table)
    np.testing.assert_array_equal(out2.cpu().numpy(), exp)
    # (c) padded leading dimension (ld > D) and float64 storage
    pad = torch.zeros((cat[0].shape[0], D + 64), dtype=torch.float64, device='cuda')
    pad[:, :D] = cat[0].double()
    out3 = dd.quantize_batch([dd.LayerBatch(pad[:, :D], 3, 80, row_offsets=offs)], table)
    np.testing.assert_array_equal(out3.cpu().numpy(), exp[:, :240])
    # (d) unaligned views fall back to the scalar-load kernel and still agree
    shifted = torch.zeros((cat[0].shape[0], D + 1), dtype=torch.float32, device='cuda')
    shifted[:, 1:] = cat[0]
    out4 = dd.quantize_batch([dd.LayerBatch(shifted[:, 1:], 3, 80, row_offsets=offs)], table)
    np.testing.assert_array_equal(out4.cpu().numpy(), exp[:, :240])


def test_headline_shape_sample_and_properties(dd):
    """BASELINE config 2 shape (L=500, D=1280, 2 layers) on a 48-sequence batch:
    oracle parity on a sample plus the size-independent properties."""
    import torch
    n_seq, L, D = 48, 500, 1280
    g = torch.Generator(device='cuda')
    g.manual_seed(4242)
    layers = []
    for _ in range(2):
        x = torch.randn((n_seq * L, D), generator=g, device='cuda')
        x = x * torch.exp(torch.randn((1, D), generator=g, device='cuda')) + 5 * torch.randn((1, D), generator=g, device='cuda')
        x[:, ::97] += 200.0
        layers.append(x)
    offs = np.arange(n_seq) * L
    table = dd.PieceTable.whole_sequences([L] * n_seq)
    lbs = [dd.LayerBatch(x, 3, 80, row_offsets=offs) for x in layers]
    out = dd.quantize_batch(lbs, table).cpu().numpy()
    assert out.shape == (n_seq, 480) and out.dtype == np.int8
    # structural invariants of every committed reference fingerprint
    rows = out.reshape(n_seq, 6, 80)
    assert out.min() >= 0
    assert ((rows == 127).sum(axis=2) == 1).all()
    assert ((rows == 0).sum(axis=2) >= 1).all()
    # oracle on a sample of sequences
    for s in (0, 7, 23, 47):
        ls = [x[s * L:(s + 1) * L].cpu().numpy() for x in layers]
        q = orc.quantize(ls, [f'1-{L}'], [3, 80, 3, 80])[f'1-{L}']
        np.testing.assert_array_equal(out[s].astype(np.int64), q)
    # exact invariances: power-of-two rescaling, batch order, chunked scratch
    out_scaled = dd.quantize_batch([dd.LayerBatch(x * 4.0, 3, 80, row_offsets=offs) for x in layers], table).cpu().numpy()
    np.testing.assert_array_equal(out_scaled, out)
    perm = np.random.default_rng(1).permutation(n_seq)
    out_perm = dd.quantize_batch([dd.LayerBatch(x, 3, 80, row_offsets=offs[perm]) for x in layers], table).cpu().numpy()
    np.testing.assert_array_equal(out_perm, out[perm])
    ctx = dd.get_context(torch.cuda.current_device())
    old = ctx.get_option('workspace_mb')
    try:
        ctx.set_option('workspace_mb', 16)
        out_chunked = dd.quantize_batch(lbs, table).cpu().numpy()
    finally:
        ctx.set_option('workspace_mb', old)
    np.testing.assert_array_equal(out_chunked, out)
    # a domain given as a piece equals the same rows passed as their own sequence
    table_sub = dd.PieceTable([L] * n_seq, [['101-400']] * n_seq)
    out_sub = dd.quantize_batch(lbs, table_sub).cpu().numpy()
    offs_sub = offs + 100
    table_own = dd.PieceTable.whole_sequences([300] * n_seq)
    out_own = dd.quantize_batch([dd.LayerBatch(x, 3, 80, row_offsets=offs_sub) for x in layers], table_own).cpu().numpy()
    np.testing.assert_array_equal(out_sub, out_own)


def test_large_ragged_lengths(dd):
    """BASELINE config 3 flavour: L in [50, 2000], D = 1280, one layer, against the oracle."""
    import torch
    rng = np.random.default_rng(2024)
    lens = [int(v) for v in rng.integers(50, 2001, size=12)] + [2000, 50]
    xs = [make_input('esm', L, 1280, 5000 + i) for i, L in enumerate(lens)]
    table = dd.PieceTable.whole_sequences(lens)
    out = dd.quantize_batch([dd.LayerBatch([torch.from_numpy(x).cuda() for x in xs], 3, 80)], table).cpu().numpy()
    for i, x in enumerate(xs):
        q = orc.quantize([x], [f'1-{lens[i]}'], [3, 80])[f'1-{lens[i]}']
        np.testing.assert_array_equal(out[i].astype(np.int64), q, err_msg=f'L={lens[i]}')


def test_api_errors(dd):
    import torch
    x = torch.zeros((10, 128), device='cuda')
    table = dd.PieceTable([10], [['1-10']])
    with pytest.raises(dd.DctfpError):
        dd.quantize_batch([dd.LayerBatch([x], 9, 80)], table)            # n above DCTFP_MAX_N
    with pytest.raises(dd.DctfpError):
        dd.quantize_batch([dd.LayerBatch([x], 3, 129)], table)           # m above DCTFP_MAX_M
    with pytest.raises(ValueError, match='cannot reshape array'):
        dd.quantize_batch([dd.LayerBatch([x[:, :64]], 3, 80)], table)    # D < m: the reference's reshape error
    bad = dd.PieceTable([10], [['1-10']])
    bad.pieces['n_rows'][0] = 11                                         # piece outside its sequence
    with pytest.raises(dd.DctfpError):
        dd.quantize_batch([dd.LayerBatch([x], 3, 80)], bad)
    with pytest.raises(ValueError):
        dd.LayerBatch([x.cpu()], 3, 80)                                  # host memory is refused


def test_fused_groups_large_batch(dd):
    """RecCut-shaped domain lists (parts tiling the protein + whole protein) stream every row once;
    same int8 as the unfused path and as the oracle, also across chunk boundaries."""
    import torch
    rng = np.random.default_rng(11)
    n_seq, D = 600, 640
    lens = [int(v) for v in rng.integers(60, 400, size=n_seq)]
    doms = []
    for L in lens:
        k = int(rng.integers(1, 6))
        if k == 1 or L < 60:
            doms.append([f'1-{L}'])
            continue
        cuts = sorted(set(int(c) // 8 * 8 for c in rng.integers(10, L - 10, size=k - 1)))
        edges = [0] + cuts + [L]
        parts = [f'{a + 1}-{b}' for a, b in zip(edges[:-1], edges[1:])]
        if len(parts) >= 3 and rng.random() < 0.4:          # a discontinuous domain: first + last part
            parts = [parts[-1] + ',' + parts[0]] + parts[1:-1]
        doms.append(parts + [f'1-{L}'])
    xs = [torch.randn((sum(lens), D), device='cuda') * 3 + 1 for _ in range(2)]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    table = dd.PieceTable(lens, doms)
    lbs = [dd.LayerBatch(x, 3, 80, row_offsets=offs) for x in xs]
    ctx = dd.get_context(torch.cuda.current_device())
    fused = dd.quantize_batch(lbs, table).cpu().numpy()
    old = {k: ctx.get_option(k) for k in ('fuse', 'workspace_mb')}
    try:
        ctx.set_option('fuse', 0)
        plain = dd.quantize_batch(lbs, table).cpu().numpy()
        ctx.set_option('fuse', 1)
        ctx.set_option('workspace_mb', 16)                  # many chunks, groups never split
        chunked = dd.quantize_batch(lbs, table).cpu().numpy()
    finally:
        for k, v in old.items():
            ctx.set_option(k, v)
    np.testing.assert_array_equal(fused, plain)
    np.testing.assert_array_equal(chunked, plain)
    row = 0
    for s in range(0, n_seq, 37):
        first = list(table.owner).index(s)
        a, b = int(offs[s]), int(offs[s]) + lens[s]
        q = orc.quantize([x[a:b].cpu().numpy() for x in xs], doms[s], [3, 80, 3, 80])
        for k, key in enumerate(q):
            np.testing.assert_array_equal(fused[first + k].astype(np.int64), q[key], err_msg=f'seq {s} {key}')


@pytest.mark.parametrize('tdtype', ['float16', 'bfloat16'])
def test_half_precision_storage(dd, tdtype):
    """Embeddings kept in float16 / bfloat16 (a half-precision ESM-2 forward pass) are read natively;
    the result equals the oracle on the same values promoted to float32 (promotion is exact)."""
    import torch
    dt = getattr(torch, tdtype)
    rng = np.random.default_rng(3)
    # (7 rows, not 5: bfloat16 makes whole channels constant over a short domain, and at L = 5 the
    #  reference's pocketfft leaves round-off noise where every other length gives an exact 0/0 -- DESIGN section 2)
    lens = [7, 64, 158, 500, 333]
    doms = [['1-7'], ['1-64'], ['1-81', '82-158', '1-158'], ['1-200', '201-330,401-500', '331-400', '1-500'], ['10-300']]
    for D in (1280, 640, 100):          # 100: not a multiple of 8 -> scalar-load variant
        xs = [[torch.from_numpy(make_input('esm', L, D, 300 + 7 * k + L)).to(dt).cuda() for L in lens] for k in range(2)]
        table = dd.PieceTable(lens, doms)
        out = dd.quantize_batch([dd.LayerBatch(xs[0], 3, 80), dd.LayerBatch(xs[1], 3, 80)], table).cpu().numpy()
        row = 0
        for s in range(len(lens)):
            ls = [xs[k][s].float().cpu().numpy() for k in range(2)]
            q = orc.quantize(ls, doms[s], [3, 80, 3, 80])
            for key, exp in q.items():
                np.testing.assert_array_equal(out[row].astype(np.int64), exp, err_msg=f'{tdtype} D={D} seq {s} {key}')
                row += 1
        assert row == table.n_domains
    # the drop-in class keeps half tensors as they are
    fp = dd.Fingerprint(pid='h', seq='A' * 158, embed={15: xs[0][2], 21: xs[1][2]}, domains=list(doms[2]))
    fp.quantize([3, 80, 3, 80])
    q = orc.quantize([xs[0][2].float().cpu().numpy(), xs[1][2].float().cpu().numpy()], doms[2], [3, 80, 3, 80])
    for k in q:
        np.testing.assert_array_equal(fp.quants[k], q[k])


def test_extremes(dd):
    """Empty inputs, one very long domain, many layers with mixed qdim, a batch of minimal domains."""
    import torch
    # nothing to do
    t0 = dd.PieceTable([10], [['11-20']])
    assert t0.n_domains == 0
    x = torch.zeros((10, 128), device='cuda')
    out = dd.quantize_batch([dd.LayerBatch([x], 3, 80)], t0)
    assert out.shape == (0, 240)
    fp = dd.Fingerprint(pid='e', seq='A' * 10, embed={0: x}, domains=['11-20', '0-5'])
    fp.quantize([3, 80])
    assert fp.quants == {} and fp.domains == []
    # a 30 000-row domain (titin-sized), against the closed-form oracle
    L, D = 30000, 128
    xl = make_input('esm', L, D, 31337)
    q = orc.quantize_matrix([xl], [f'1-{L}', f'2-{L - 1}'], [3, 80])
    fpl = dd.Fingerprint(pid='t', seq='A' * L, embed={0: xl}, domains=[f'1-{L}', f'2-{L - 1}'])
    fpl.quantize([3, 80])
    for k in q:
        np.testing.assert_array_equal(fpl.quants[k], q[k])
    # five layers, mixed qdim and widths, float64 + float32 storage
    Ls = 77
    mats = {0: make_input('esm', Ls, 640, 1), 1: make_input('gauss', Ls, 640, 2).astype(np.float64),
            2: make_input('esm', Ls, 200, 3), 3: make_input('contact', Ls, Ls, 4), 4: make_input('smooth', Ls, 1280, 5)}
    qd = [3, 80, 5, 44, 2, 100, 4, 64, 8, 128]
    doms = ['1-77', '1-30,41-77', '31-40']
    fp5 = dd.Fingerprint(pid='m', seq='A' * Ls, embed=mats, domains=list(doms))
    fp5.quantize(qd)
    q5 = orc.quantize([np.asarray(v) for v in mats.values()], doms, qd)
    assert list(fp5.quants) == list(q5)
    for k in q5:
        np.testing.assert_array_equal(fp5.quants[k], q5[k], err_msg=k)
    # 20 000 minimal domains (3 rows each) in one call
    n = 20000
    big = torch.from_numpy(make_input('gauss', 3 * n, 96, 77)).cuda()
    tb = dd.PieceTable.whole_sequences([3] * n)
    ob = dd.quantize_batch([dd.LayerBatch(big, 3, 80, row_offsets=np.arange(n) * 3)], tb).cpu().numpy()
    host = big.cpu().numpy()
    for s in (0, 1, 9999, 19999):
        qs = orc.quantize([host[3 * s:3 * s + 3]], ['1-3'], [3, 80])['1-3']
        np.testing.assert_array_equal(ob[s].astype(np.int64), qs)


def test_randomised_shapes_against_oracle(dd):
    """Seeded fuzz over shapes the fixed cases may miss: odd widths (scalar-load variant), widths that are
    not multiples of 32, unaligned row strides, 1-8 kept points, 1-128 kept channels, float32 / float64 /
    float16 storage, RecCut-shaped and arbitrary domain lists, several proteins per call."""
    import torch
    rng = np.random.default_rng(987654321)
    n_cases = 60
    for case in range(n_cases):
        n_seq = int(rng.integers(1, 5))
        D = int(rng.choice([33, 64, 96, 100, 127, 160, 320, 640, 644, 1280]))
        n_layers = int(rng.integers(1, 4))
        qd = []
        for _ in range(n_layers):
            n = int(rng.integers(2, 9)) if rng.random() < 0.5 else 3
            m = int(rng.integers(2, min(D - 1, 128) + 1)) if rng.random() < 0.5 else min(80, D - 1)
            qd += [n, m]
        n_max = max(qd[0::2])
        lens, doms = [], []
        for _ in range(n_seq):
            L = int(rng.integers(n_max + 20, 400))
            style = rng.random()
            if style < 0.4:                                   # RecCut shape: parts tile the protein + whole
                k = int(rng.integers(2, 5))
                cuts = sorted(set(int(c) for c in rng.integers(n_max, L - n_max, size=k - 1)))
                edges = [0] + cuts + [L]
                edges = [e for i, e in enumerate(edges) if i == 0 or e - edges[i - 1] >= n_max or e == L]
                if L - edges[-2] < n_max:
                    edges.pop(-2)
                parts = [f'{a + 1}-{b}' for a, b in zip(edges[:-1], edges[1:])]
                d = parts + [f'1-{L}'] if len(parts) > 1 else [f'1-{L}']
            elif style < 0.7:                                 # arbitrary, overlapping, discontinuous
                d = []
                for _ in range(int(rng.integers(1, 4))):
                    a = int(rng.integers(1, L - n_max))
                    b = int(rng.integers(a + n_max, L + 1))
                    if rng.random() < 0.3 and b - a > 2 * n_max + 4:
                        mid = (a + b) // 2
                        d.append(f'{mid + 1}-{b},{a}-{mid - 2}')
                    else:
                        d.append(f'{a}-{b}')
            else:
                d = [f'1-{L}']
            lens.append(L)
            doms.append(d)
        dtype = rng.choice(['float32', 'float32', 'float64', 'float16'])
        pad = int(rng.choice([0, 0, 1, 4, 7]))                 # extra columns -> odd leading dimension
        layers_np, lbs = [], []
        for li in range(n_layers):
            per_seq_np, per_seq_t = [], []
            for s, L in enumerate(lens):
                x = make_input('esm' if rng.random() < 0.7 else 'gauss', L, D, 50_000 + 97 * case + 13 * li + s)
                t = torch.from_numpy(x).to(getattr(torch, dtype))
                buf = torch.zeros((L, D + pad), dtype=t.dtype, device='cuda')
                buf[:, :D] = t.cuda()
                view = buf[:, :D]
                per_seq_t.append(view)
                per_seq_np.append(view.float().cpu().numpy() if dtype != 'float64' else view.cpu().numpy())
            layers_np.append(per_seq_np)
            lbs.append(dd.LayerBatch(per_seq_t, qd[2 * li], qd[2 * li + 1]))
        table = dd.PieceTable(lens, doms)
        out = dd.quantize_batch(lbs, table).cpu().numpy()
        row = 0
        for s in range(n_seq):
            q = {}
            for li in range(n_layers):                          # one oracle call per layer keeps the columns apart
                ql = orc.quantize_matrix([layers_np[li][s]], doms[s], qd[2 * li:2 * li + 2])
                for key, v in ql.items():
                    q.setdefault(key, []).append(v)
            # oracle merges duplicate keys; the batch API keeps one row per input domain -> compare per input domain
            for dom in doms[s]:
                exp = np.concatenate([orc.quantize_matrix([layers_np[li][s]], [dom], qd[2 * li:2 * li + 2])[orc.split_domain(dom, lens[s])[1]]
                                      for li in range(n_layers)])
                np.testing.assert_array_equal(out[row].astype(np.int64), exp,
                                              err_msg=f'case {case} seq {s} dom {dom} D={D} qd={qd} {dtype} pad={pad}')
                row += 1
        assert row == table.n_domains


def test_config4_batch_with_reference_goldens_inside(dd):
    """BASELINE config 4 as stated, at scale: 2 400 proteins, D = 2560, L <= 500, RecCut-shaped domain lists
    (parts + whole protein, discontinuous parts) through ONE quantize_batch call with fused walks, the scratch cut
    into several chunks.  The reference-generated golden cases `c4_D2560_*` (tests/golden/make_golden.py section 8)
    and the D = 2560 queue_cpu cases (make_golden_reccut.py) sit inside the batch -- first, last and at positions
    that land on chunk boundaries -- and must come out bit-exact; a sample of the filler is checked against the
    oracle; fused, unfused and small-scratch runs must agree on every byte."""
    import json
    import os
    import torch
    D = 2560
    gold = [c for c in ALL_OK if c['id'].startswith('c4_D2560_')]
    assert len(gold) >= 9
    with open(os.path.join(gu.GOLD, 'reccut_golden.json')) as fh:
        rc_cases = [c for c in json.load(fh)['cases'] if c.get('pipeline', {}).get('D') == D]
    rc_arr = np.load(os.path.join(gu.GOLD, 'reccut_golden.npz'))
    assert len(rc_cases) >= 8
    members = []                                   # (layers [2 x (L, D) float32], domains, expected {key: int8})
    for c in gold:
        members.append((gu.build_layers(c), c['domains'], gu.expected(c)))
    for c in rc_cases:
        pl = c['pipeline']
        ls = [make_input('esm', c['L'], D, sd) for sd in pl['seeds']]
        members.append((ls, c['domains'], {k: rc_arr[f"{c['id']}/q/{i}"] for i, k in enumerate(pl['keys'])}))
    n_seq = 2400
    rng = np.random.default_rng(404)
    slots = sorted(set([0, n_seq - 1] + [int(v) for v in np.linspace(1, n_seq - 2, len(members) - 2)]))
    assert len(slots) == len(members)
    where = dict(zip(slots, range(len(members))))
    lens, doms = [], []
    for s in range(n_seq):
        if s in where:
            ls, dm, _ = members[where[s]]
            lens.append(ls[0].shape[0])
            doms.append(list(dm))
            continue
        L = int(rng.integers(100, 501))
        k = int(rng.integers(1, 7))
        if k == 1:
            lens.append(L)
            doms.append([f'1-{L}'])
            continue
        cuts = sorted(set(int(c) for c in rng.integers(22, L - 22, size=k - 1)))
        edges = [0] + cuts + [L]
        edges = [e for i, e in enumerate(edges) if i == 0 or e == L or e - edges[i - 1] >= 22]
        if L - edges[-2] < 22:
            edges.pop(-2)
        parts = [f'{a + 1}-{b}' for a, b in zip(edges[:-1], edges[1:])]
        if len(parts) >= 3 and rng.random() < 0.3:
            parts = [parts[-1] + ',' + parts[0]] + parts[1:-1]          # RecCut's discontinuous form: 'c-d,a-b'
        lens.append(L)
        doms.append(parts + [f'1-{L}'] if len(parts) > 1 else [f'1-{L}'])
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    g = torch.Generator(device='cuda')
    g.manual_seed(44)
    xs = []
    for k in range(2):
        x = torch.randn((int(sum(lens)), D), generator=g, device='cuda')
        x = x * torch.exp(torch.randn((1, D), generator=g, device='cuda')) + 5 * torch.randn((1, D), generator=g, device='cuda')
        x[:, 5::101] += 200.0
        for s, mi in where.items():
            x[int(offs[s]):int(offs[s]) + lens[s]] = torch.from_numpy(members[mi][0][k]).cuda()
        xs.append(x)
    table = dd.PieceTable(lens, doms)
    assert table.n_domains * 2 >= 4 * 2048                               # enough jobs for the 4-chunk plan
    lbs = [dd.LayerBatch(x, 3, 80, row_offsets=offs) for x in xs]
    ctx = dd.get_context(torch.cuda.current_device())
    assert ctx.get_option('fuse') == 1
    out = dd.quantize_batch(lbs, table).cpu().numpy()
    first = {}
    for row, s in enumerate(table.owner):
        first.setdefault(s, row)
    # 1. the reference's own outputs
    n_gold_rows = 0
    for s, mi in where.items():
        _, dm, exp = members[mi]
        keys = table.keys[first[s]:first[s] + len(exp)]
        assert keys == list(exp), (s, keys)
        for i, k in enumerate(exp):
            np.testing.assert_array_equal(out[first[s] + i], np.asarray(exp[k]).astype(np.int8), err_msg=f'slot {s} {k}')
            n_gold_rows += 1
    assert n_gold_rows >= 60
    # 2. filler sample against the oracle
    for s in [v for v in range(3, n_seq, 211) if v not in where]:
        a, b = int(offs[s]), int(offs[s]) + lens[s]
        q = orc.quantize([x[a:b].cpu().numpy() for x in xs], doms[s], [3, 80, 3, 80])
        for i, k in enumerate(q):
            np.testing.assert_array_equal(out[first[s] + i].astype(np.int64), q[k], err_msg=f'seq {s} {k}')
    # 3. every byte: unfused path, small scratch (many chunks, groups never split)
    old = {k: ctx.get_option(k) for k in ('fuse', 'workspace_mb')}
    try:
        ctx.set_option('workspace_mb', 64)
        small = dd.quantize_batch(lbs, table).cpu().numpy()
        ctx.set_option('fuse', 0)
        plain = dd.quantize_batch(lbs, table).cpu().numpy()
    finally:
        for k, v in old.items():
            ctx.set_option(k, v)
    np.testing.assert_array_equal(small, out)
    np.testing.assert_array_equal(plain, out)
    rows = out.reshape(-1, 6, 80)
    assert ((rows == 127).sum(axis=2) == 1).all() and ((rows == 0).sum(axis=2) >= 1).all()


def test_walk_kernel_widths_and_kept_columns_against_oracle(dd):
    """The walk kernel contracts stage B in even/odd halves over channel pairs (d, D-1-d) and column pairs (c, m-1-c):
    widths where D/2 is not a multiple of 4 (D % 8 == 4: two lanes hold the same four channels) or of 16 (zero-padded
    pair groups), odd m (the middle column is its own mirror) and every wave count (3, 5, 10), forced through the walk
    kernel (path=2) with RecCut-shaped and plain domain lists, a NaN channel and a constant channel among them.  Eight jobs a
    call: choose_route fuses walks from 64 jobs, so these are the PLAIN builds, asserted by name ("last_walk"); the FUSED builds
    see these widths in tests/test_walk_ladder_gpu.py."""
    import torch
    rng = np.random.default_rng(20261004)
    ctx = dd.get_context(torch.cuda.current_device())
    shapes = [(512, 80), (516, 80), (644, 75), (768, 80), (772, 80), (1000, 80), (1028, 65), (1284, 79), (1288, 70), (2052, 72),
              (2556, 80), (2560, 77), (640, 80), (1280, 66)]
    try:
        ctx.set_option('path', 2)
        for ci, (D, m) in enumerate(shapes):
            lens, doms = [], []
            for s in range(3):
                L = int(rng.integers(40, 160))
                if s < 2:                                       # parts tile the protein + whole protein (fused walk)
                    cut = int(rng.integers(10, L - 10))
                    doms.append([f'1-{cut}', f'{cut + 1}-{L}', f'1-{L}'])
                else:
                    doms.append([f'1-{L}', f'3-{L - 2}'])
                lens.append(L)
            xs = []
            for s, L in enumerate(lens):
                x = make_input('esm', L, D, 70_000 + 31 * ci + s)
                if s == 1:
                    x[:, D // 2 - 1] = 0.25                     # constant channel next to the fold line -> its layer block is 0
                if s == 2:
                    x[5, D - 3] = np.nan
                xs.append(x)
            ts = [torch.from_numpy(x).cuda() for x in xs]
            ctx.set_option('degenerate_channels', 0)
            out = dd.quantize_batch([dd.LayerBatch(ts, 3, m)], dd.PieceTable(lens, doms)).cpu().numpy()
            assert ctx.get_option('last_path') == 2
            assert wl.decode_walk(ctx.get_option('last_walk')) == wl.expected_walk('f32', D, m, False), (D, m)
            row = 0
            for s in range(3):
                for dom in doms[s]:
                    if s == 1:      # constant channel: 0/0 -> NaN -> 0 (the lengths where the reference's FFT leaves round-off
                        assert not out[row].any()               # noise instead are fenced in tests/test_fences.py)
                    else:
                        exp = orc.quantize_matrix([xs[s]], [dom], [3, m])[orc.split_domain(dom, lens[s])[1]]
                        np.testing.assert_array_equal(out[row].astype(np.int64), exp, err_msg=f'D={D} m={m} seq {s} dom {dom}')
                    row += 1
            assert row == out.shape[0]
            # the constant channel of protein 1 is seen once per job that streams it (3 jobs), whatever lanes hold it
            assert ctx.get_option('degenerate_channels') == 3, (D, m)
    finally:
        ctx.set_option('path', 0)


def test_result_slots_survive_a_buffer_change_between_layer_groups(dd):
    """One protein whose layers differ in their row count is enqueued group by group into the pinned result buffer;
    when the second group does not fit, a new buffer is taken and the first group's slot must still be read from the
    old one (and stay alive until the stream has been waited for)."""
    import dctdomain_amd.fingerprint as fpm
    L, D = 90, 640
    x0 = make_input('esm', L, D, 9101)
    x1 = make_input('esm', L + 7, D, 9102)
    doms = ['1-40', '20-90']
    warm = dd.Fingerprint(pid='w', seq='A' * L, embed={0: x0}, domains=list(doms))
    warm.quantize([3, 80])                                    # the thread's buffer exists now
    st = fpm._RESULTS
    first = len(doms) * 240
    st.used = st.pin.numel() - first - 16                     # room for the first group only
    old = st.pin
    fp = dd.Fingerprint(pid='t', seq='A' * L, embed={0: x0, 1: x1}, domains=list(doms))
    fp.quantize([3, 80, 3, 80])
    assert st.pin is not old
    for dom in doms:
        exp = np.concatenate([orc.quantize_matrix([x0], [dom], [3, 80])[dom], orc.quantize_matrix([x1], [dom], [3, 80])[dom]])
        np.testing.assert_array_equal(fp.quants[dom], exp)


def test_midsize_calls_fused_walks_with_both_stage_b_forms(dd):
    """Between a protein per call and a batch: 44 multi-domain proteins in one call (64 <= jobs < 256: fused stage A, Y'
    unpacked, stage B over 64-channel slabs) against the oracle, and byte for byte against the MFMA stage B (packed Y')
    and the unfused form of the same call."""
    import torch
    rng = np.random.default_rng(4242)
    D = 640
    ctx = dd.get_context(torch.cuda.current_device())
    lens, doms, xs = [], [], []
    for s in range(44):
        L = int(rng.integers(60, 260))
        k = int(rng.integers(1, 4))
        if k == 1:
            d = [f'1-{L}']
        else:
            cuts = sorted(set(int(c) for c in rng.integers(22, L - 22, size=k - 1)))
            e = [0] + cuts + [L]
            e = [v for i, v in enumerate(e) if i == 0 or v == L or v - e[i - 1] >= 22]
            if L - e[-2] < 22:
                e.pop(-2)
            parts = [f'{a + 1}-{b}' for a, b in zip(e[:-1], e[1:])]
            d = parts + [f'1-{L}'] if len(parts) > 1 else [f'1-{L}']
        lens.append(L)
        doms.append(d)
        xs.append([make_input('esm', L, D, 88_000 + 2 * s + li) for li in range(2)])
    table = dd.PieceTable(lens, doms)
    assert 64 <= 2 * table.n_domains < 256
    lbs = [dd.LayerBatch([torch.from_numpy(x[li]).cuda() for x in xs], 3, 80) for li in range(2)]
    from dctdomain_amd import _lib
    xctx = _lib.experiments_context(torch.cuda.current_device())      # (the slab / MFMA stage-B switch is an engineering knob)
    saved = {k: xctx.get_option(k) for k in ('small_b_jobs', 'fuse')}
    try:
        out = dd.quantize_batch(lbs, table).cpu().numpy()
        assert ctx.get_option('last_path') == 1
        assert (dd.quantize_batch(lbs, table, ctx=xctx).cpu().numpy() == out).all()
        xctx.set_option('small_b_jobs', 0)
        assert (dd.quantize_batch(lbs, table, ctx=xctx).cpu().numpy() == out).all()
        xctx.set_option('small_b_jobs', saved['small_b_jobs'])
        xctx.set_option('fuse', 0)
        assert (dd.quantize_batch(lbs, table, ctx=xctx).cpu().numpy() == out).all()
    finally:
        for k, v in saved.items():
            xctx.set_option(k, v)
    row = 0
    for s in range(44):
        for dom in doms[s]:
            exp = np.concatenate([orc.quantize_matrix([xs[s][li]], [dom], [3, 80])[dom] for li in range(2)])
            np.testing.assert_array_equal(out[row].astype(np.int64), exp, err_msg=f'seq {s} dom {dom}')
            row += 1
    assert row == table.n_domains


@pytest.mark.parametrize('tdtype', ['float16', 'bfloat16'])
def test_half_precision_fused_walks(dd, tdtype):
    """Multi-domain proteins in half precision in one call large enough to be fused (>= 64 jobs: the parts and the whole
    protein fed from the same rows; 4 channels per lane for half-precision rows): against the oracle on the same values
    promoted to float32, and byte for byte against the unfused form.  About 100 jobs, fewer than the 256 the default "path"
    wants for the walk kernel: this is the TWO-KERNEL path -- its fused stage-A build at 4 channels per lane and its plain one at
    8, asserted by name ("last_stage_a"); the walk kernel's FUSED half-precision builds run in tests/test_walk_ladder_gpu.py."""
    import torch
    dt = getattr(torch, tdtype)
    storage = {'float16': 'f16', 'bfloat16': 'bf16'}[tdtype]
    rng = np.random.default_rng(77)
    ctx = dd.get_context(torch.cuda.current_device())
    for D in (640, 1000):
        lens, doms, xs = [], [], []
        for s in range(14):
            L = int(rng.integers(90, 240))
            c1, c2 = int(L * 0.3), int(L * 0.62)
            d = [f'1-{c1}', f'{c1 + 1}-{c2}', f'{c2 + 1}-{L}', f'1-{L}'] if s % 3 else [f'{c2 + 1}-{L},1-{c1}', f'{c1 + 1}-{c2}', f'1-{L}']
            lens.append(L)
            doms.append(d)
            xs.append([torch.from_numpy(make_input('esm', L, D, 41_000 + 2 * s + li)).to(dt).cuda() for li in range(2)])
        table = dd.PieceTable(lens, doms)
        assert 2 * table.n_domains >= 64
        lbs = [dd.LayerBatch([x[li] for x in xs], 3, 80) for li in range(2)]
        out = dd.quantize_batch(lbs, table).cpu().numpy()
        a = sl.decode_stage_a(ctx.get_option('last_stage_a'))
        assert ctx.get_option('last_path') == 1 and ctx.get_option('last_walk') == 0
        assert (a.storage, a.n, a.vec, a.fused) == (storage, 3, 4, True), (D, a)
        ctx.set_option('fuse', 0)
        try:
            assert (dd.quantize_batch(lbs, table).cpu().numpy() == out).all()
            a = sl.decode_stage_a(ctx.get_option('last_stage_a'))
            assert ctx.get_option('last_path') == 1 and (a.storage, a.n, a.vec, a.fused) == (storage, 3, 8, False), (D, a)
        finally:
            ctx.set_option('fuse', 1)
        row = 0
        for s in range(len(lens)):
            ls = [xs[s][li].float().cpu().numpy() for li in range(2)]
            for dom in doms[s]:
                exp = np.concatenate([orc.quantize_matrix([ls[li]], [dom], [3, 80])[orc.split_domain(dom, lens[s])[1]] for li in range(2)])
                np.testing.assert_array_equal(out[row].astype(np.int64), exp, err_msg=f'{tdtype} D={D} seq {s} {dom}')
                row += 1
        assert row == table.n_domains


@pytest.mark.parametrize('tdtype', ['float16', 'bfloat16'])
def test_walk_kernel_on_half_precision_rows(dd, tdtype):
    """The walk kernel reads float16 / bfloat16 rows as 8 bytes per lane (4 channels, like float32): forced (path=2) on
    small batches of whole proteins and of multi-domain proteins at the three wave counts, against the oracle on the same
    values promoted to float32.  Nine jobs a call, fewer than the 64 choose_route fuses walks from: the PLAIN builds, asserted by
    name ("last_walk"); the FUSED ones run in tests/test_walk_ladder_gpu.py."""
    import torch
    dt = getattr(torch, tdtype)
    storage = {'float16': 'f16', 'bfloat16': 'bf16'}[tdtype]
    rng = np.random.default_rng(515)
    ctx = dd.get_context(torch.cuda.current_device())
    try:
        ctx.set_option('path', 2)
        for D, m in ((640, 80), (1000, 75), (1280, 80), (2560, 72)):
            lens, doms, xs = [], [], []
            for s in range(5):
                L = int(rng.integers(60, 200))
                if s % 2:
                    c = int(L * 0.45)
                    doms.append([f'1-{c}', f'{c + 1}-{L}', f'1-{L}'])
                else:
                    doms.append([f'1-{L}'])
                lens.append(L)
                xs.append(torch.from_numpy(make_input('esm', L, D, 61_000 + 10 * s + D)).to(dt).cuda())
            out = dd.quantize_batch([dd.LayerBatch(xs, 3, m)], dd.PieceTable(lens, doms)).cpu().numpy()
            assert ctx.get_option('last_path') == 2, (D, m)
            assert wl.decode_walk(ctx.get_option('last_walk')) == wl.expected_walk(storage, D, m, False), (D, m)
            row = 0
            for s in range(5):
                x = xs[s].float().cpu().numpy()
                for dom in doms[s]:
                    exp = orc.quantize_matrix([x], [dom], [3, m])[orc.split_domain(dom, lens[s])[1]]
                    np.testing.assert_array_equal(out[row].astype(np.int64), exp, err_msg=f'{tdtype} D={D} m={m} seq {s} {dom}')
                    row += 1
            assert row == out.shape[0]
    finally:
        ctx.set_option('path', 0)


def test_one_protein_per_call_bit_exact(dd):
    """A protein at a time -- the reference's calling pattern -- through the small-call path (stage A over row chunks, stage B
    over 64-channel slabs): bit-exact against the oracle over widths that end inside a slab, kept columns below and above 64,
    domain lists with discontinuous parts, NaN / inf, GPU and host embeddings, and call after call on one context."""
    import torch
    ctx = dd.get_context(torch.cuda.current_device())
    rng = np.random.default_rng(2024)
    shapes = [(500, 1280, [3, 80, 3, 80]), (500, 1280, [3, 80, 3, 80]), (129, 640, [3, 80, 3, 65]), (1999, 2560, [3, 80, 3, 80]),
              (300, 1000, [3, 70, 3, 33]), (128, 520, [3, 16, 3, 80]), (777, 1284, [3, 80]), (256, 2048, [3, 72, 3, 72, 3, 72])]
    for rep, (L, D, qdim) in enumerate(shapes):
        k = len(qdim) // 2
        layers = [make_input('esm' if i == 0 else 'gauss', L, D, 1000 * rep + i).astype(np.float32) for i in range(k)]
        if rep == 1:      # degenerate values: the (layer, domain) blocks they touch become 0, the others must not notice
            layers[0][7, 5] = np.nan
            layers[1][L - 60:, 9] = np.inf
        cuts = [int(rng.integers(130, L // 2 - 20)), int(rng.integers(L // 2 + 20, L - 130))] if L >= 400 else []
        doms = [f'1-{L}']
        if cuts:
            doms = [f'1-{cuts[0]}', f'{cuts[0] + 1}-{cuts[1]}', f'1-{cuts[0] // 2},{cuts[1] + 1}-{L}', f'1-{L}']
        want = orc.quantize(layers, doms, qdim)
        for embed in ({i: torch.from_numpy(x).cuda() for i, x in enumerate(layers)}, {i: x for i, x in enumerate(layers)}):
            fp = dd.Fingerprint(pid=f'small{rep}', seq='A' * L, embed=embed, domains=list(doms))
            fp.quantize(list(qdim))
            if (L, D) == (500, 1280) and torch.is_tensor(embed[0]):
                # 8 jobs x 5 slabs: what split_rows_over_workgroups and "small_b_jobs" promise for such a call
                assert sl.decode_stage_a(ctx.get_option('last_stage_a')) == sl.StageA('f32', 3, 4, 8, 4, False, False, True)
                assert sl.decode_stage_b(ctx.get_option('last_stage_b')) == sl.StageB(sl.SLAB_FROM_SPLIT, 0, False, False, False)
            assert list(fp.quants) == list(want)
            for key in want:
                np.testing.assert_array_equal(fp.quants[key], want[key], err_msg=f'L={L} D={D} {qdim} {key}')
    # a handful of proteins per call through the batch API
    lens = [150, 400, 260]
    layers = [[make_input('esm', L, 1280, 50 + 3 * s + i) for s, L in enumerate(lens)] for i in range(2)]
    table = dd.PieceTable(lens, [[f'1-{L}'] for L in lens])
    lbs = [dd.LayerBatch([torch.from_numpy(x).cuda() for x in layers[i]], 3, 80) for i in range(2)]
    out = dd.quantize_batch(lbs, table, ctx=ctx).cpu().numpy()
    for s, L in enumerate(lens):
        q = orc.quantize([layers[0][s], layers[1][s]], [f'1-{L}'], [3, 80, 3, 80])
        np.testing.assert_array_equal(out[s].astype(np.int64), q[f'1-{L}'])
