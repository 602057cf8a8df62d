"""The single-matrix methods of the drop-in ``Fingerprint`` -- ``idct_quant``, ``dct_coefficients``, ``scale``, ``get_doms`` --
and the three C entry points behind them (``dctfp_idct_quant``, ``dctfp_scale``, ``dctfp_gather_rows``) at their edges.

idct_quant / dct_coefficients are held against the longdouble rule of tests/idct_rule.py on its case matrix: widths that end
inside, on and just past a 64-thread workgroup, num from 1 to n_rows, nine ways of handing the matrix in.  The bound is not
chosen by eye: per case

    |GPU - longdouble| <= 8 * e_ref + floor

e_ref = the float64 scipy oracle's own worst error against the same longdouble values on the same input (measured in
tests/test_idct_rule_host.py), floor = 4 ulp of the largest magnitude among the column's values.  8 covers another order of
summation over up to 2 000 terms with fma; it is not to be widened to make a case pass.

Measured worst ratio  GPU error / (8 * e_ref + floor)  per recipe on an MI355X (1.0 = the bound):

    recipe   coefficients   scaled values
    esm      0.138          0.012
    gauss    0.098          0.246
    ramp     0.140          0.250
    big      0.083          0.056
    small    0.083          0.156

scale is compared with numpy float64 for equality; get_doms with the oracle's for equality; the error codes are read
straight through ctypes on the product library.  No test here launches anything out of bounds: every refusal is checked on
buffers large enough for the call had it gone through.
"""

import ctypes as C
import warnings

import numpy as np
import pytest

import idct_rule as rule
from oracle import dct_oracle as orc

pytestmark = pytest.mark.gpu

IDS = [c['id'] for c in rule.CASES]
NAN = float('nan')


@pytest.fixture(scope='module')
def dd():
    import torch
    assert torch.cuda.is_available()
    import dctdomain_amd
    return dctdomain_amd


@pytest.fixture(scope='module')
def fp(dd):
    return dd.Fingerprint()


def poison(*shape):
    """A NaN-filled float64 block of the size the method is about to allocate, freed again: the caching allocator hands the
    same block back, so an element the kernel fails to write reads NaN, not the right value of an earlier identical call."""
    import torch
    t = torch.full(shape, NAN, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    del t


def hand_in(case, x):
    """The promoted matrix ``x`` (float32 / float64 numpy) in the form the case names -> (argument, tensor expected back)."""
    import torch
    form = case['form']
    if form in ('np32', 'np64'):
        return x, False
    if form == 'np16':
        a = x.astype(np.float16)
        assert (a.astype(np.float32) == x).all()
        return a, False
    if form == 'npi32':
        a = x.astype(np.int32)
        assert (a == x).all()
        return a, False
    if form == 'np64T':
        a = np.ascontiguousarray(x.T).T
        assert not a.flags['C_CONTIGUOUS'] or min(a.shape) == 1
        return a, False
    if form == 'cuda32':
        return torch.from_numpy(x).cuda(), True
    if form == 'slice':
        wide = torch.full((x.shape[0], x.shape[1] + 9), NAN, dtype=torch.float32, device='cuda')
        wide[:, 3:3 + x.shape[1]] = torch.from_numpy(x).cuda()
        t = wide[:, 3:3 + x.shape[1]]
        assert t.data_ptr() % 16 == 12 and (x.shape[0] == 1 or t.stride(0) > x.shape[1])
        return t, True
    if form == 'cuda32T':
        return torch.from_numpy(np.ascontiguousarray(x.T)).cuda().T, True
    if form == 'bf16':
        t = torch.from_numpy(x).cuda().to(torch.bfloat16)
        assert (t.to(torch.float32).cpu().numpy() == x).all()
        return t, True
    raise KeyError(form)


def to_numpy(got, want_tensor):
    import torch
    if want_tensor:
        assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float64
        return got.cpu().numpy()
    assert isinstance(got, np.ndarray) and got.dtype == np.float64
    return got


def check_bound(got, ref, e_ref, axis, what):
    """``|got - ref| <= 8 e_ref + floor`` element by element, NaN exactly where the rule has NaN; prints the worst ratio."""
    assert got.shape == ref.shape, what
    nan_ref = np.isnan(ref)
    assert (np.isnan(got) == nan_ref).all(), f'{what}: NaN pattern differs'
    if nan_ref.all():
        print(f'RATIO {what} all-NaN')
        return 0.0
    with np.errstate(all='ignore'):
        err = np.abs(got.astype(rule.LD) - ref).astype(np.float64)
        bound = np.broadcast_to(8.0 * e_ref + rule.ulp_floor(ref, axis), ref.shape)
        ratio = float((err[~nan_ref] / bound[~nan_ref]).max())
    print(f'RATIO {what} err {err[~nan_ref].max():.3e} e_ref {e_ref:.3e} ratio {ratio:.3f}')
    assert ratio <= 1.0, f'{what}: GPU error is {ratio:.2f} x (8 e_ref + floor), e_ref = {e_ref:.3e}'
    return ratio


# -------------------------------------------------------------------------------------------------------------------
# idct_quant / dct_coefficients
# -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', rule.CASES, ids=IDS)
def test_idct_quant_matches_the_rule(fp, case):
    x, _, scaled = rule.reference(case)
    arg, want_tensor = hand_in(case, x)
    poison(case['num'], case['n_cols'])
    got = to_numpy(fp.idct_quant(arg, case['num']), want_tensor)
    if case['num'] == 1:
        assert np.isnan(got).all()               # one value per column: 0/0
    check_bound(got, scaled, rule.oracle_error(case)[1], 0, f"scaled {case['recipe']} {case['id']}")


@pytest.mark.parametrize('case', rule.CASES, ids=IDS)
def test_dct_coefficients_match_the_rule(fp, case):
    x, coef, _ = rule.reference(case)
    arg, want_tensor = hand_in(case, x)
    poison(case['n_cols'], case['num'])
    got = to_numpy(fp.dct_coefficients(arg, case['num']), want_tensor)
    check_bound(got, coef, rule.oracle_error(case)[0], 1, f"coef {case['recipe']} {case['id']}")


def test_num_above_the_rows_returns_the_rows(fp):
    x = np.random.default_rng(21).standard_normal((5, 65)).astype(np.float32)
    full = fp.idct_quant(x, 5)
    for num in (6, 80, 70000):
        got = fp.idct_quant(x, num)
        assert got.shape == (5, 65)
        np.testing.assert_array_equal(got, full)
        assert fp.dct_coefficients(x, num).shape == (65, 5)


def test_non_default_stream(fp):
    """The call goes onto torch's current stream: its result is complete once THAT stream is synchronised."""
    import torch
    case = next(c for c in rule.CASES if c['id'].startswith('257x130_num128'))
    x, coef, scaled = rule.reference(case)
    stream = torch.cuda.Stream()
    t = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    poison(case['num'], case['n_cols'])
    with torch.cuda.stream(stream):
        got = fp.idct_quant(t, case['num'])
        got_c = fp.dct_coefficients(t, case['num'])
        v = torch.from_numpy(np.random.default_rng(4).standard_normal(1025)).cuda()
        sc = fp.scale(v)
        rows, _ = fp.get_doms(t, '3-9,200-257')
    stream.synchronize()
    e_coef, e_scaled = rule.oracle_error(case)
    check_bound(got.cpu().numpy(), scaled, e_scaled, 0, 'scaled stream')
    check_bound(got_c.cpu().numpy(), coef, e_coef, 1, 'coef stream')
    vh = v.cpu().numpy()
    np.testing.assert_array_equal(sc.cpu().numpy(), (vh - vh.min()) / (vh.max() - vh.min()))
    np.testing.assert_array_equal(rows.cpu().numpy(), np.concatenate([x[2:9], x[199:257]]).astype(np.float64))


DEGENERATE = ('nan', '+inf', '-inf', 'const', 'lastbit')


def plant(x, kind, col):
    y = x.copy()
    row = 0 if col == 0 else x.shape[0] // 2      # (row 0 is the row the kernel shifts by)
    if kind == 'nan':
        y[row, col] = np.nan
    elif kind == '+inf':
        y[row, col] = np.inf
    elif kind == '-inf':
        y[row, col] = -np.inf
    else:
        y[:, col] = 200.125
        if kind == 'lastbit':
            y[row, col] = np.nextafter(y.dtype.type(200.125), y.dtype.type(1000))
    return y


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('kind', DEGENERATE)
def test_degenerate_column_stays_in_its_column(fp, kind, dtype):
    """A NaN, an infinity or a constant makes ITS column NaN and leaves every other column's bits alone: the kernels never mix
    columns.  A column constant but for one last-bit change is no constant: finite, and within the bound of the rule."""
    x = rule.recipe_matrix('esm', 257, 130, 77).astype(dtype)
    num = 5
    base_s, base_c = fp.idct_quant(x, num), fp.dct_coefficients(x, num)
    assert np.isfinite(base_s).all()
    for col in (0, 63, 64, 129):
        y = plant(x, kind, col)
        poison(num, 130)
        s, c = fp.idct_quant(y, num), fp.dct_coefficients(y, num)
        others = np.arange(130) != col
        assert (s[:, others].view(np.uint64) == base_s[:, others].view(np.uint64)).all(), (kind, col)
        assert (c[others].view(np.uint64) == base_c[others].view(np.uint64)).all(), (kind, col)
        if kind != 'lastbit':
            assert np.isnan(s[:, col]).all(), (kind, col)
            continue
        assert np.isfinite(s[:, col]).all() and s[:, col].min() == 0.0 and s[:, col].max() == 1.0
        y64 = y[:, col:col + 1].astype(np.float64)
        rc, rs = rule.idct_quant(y64, num)
        with np.errstate(all='ignore'), warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)
            e_s = rule.max_err(orc.idct_quant(y64, num), rs)
            e_c = rule.max_err(orc.coefficients(y64, num), rc)
        # its own worst case, from the arithmetic (u = 2^-53): d_t = x_t - x_0 is exact; every cosine is good to 1 ulp = 2u and
        # the compensated sum adds u of the result, so |err fs_k| <= 3u D with D = sum |d_t|; the inverse over k = 1..num-1
        # passes that on and adds as much again, |err y_j| <= 6u (num - 1) D; the scale of values with range R turns it into
        # at most 4 |err y| / R, and its subtraction and division add 4u
        d = np.abs(y64[:, 0] - y64[0, 0]).sum()
        y_rule = rule.resampled(y64, num)[1][:, 0]
        r = float(y_rule.max() - y_rule.min()) / (np.sqrt(2.0 / y64.shape[0]) * np.sqrt(2.0 / num))
        u = 2.0 ** -53
        worst = 4 * 6 * u * (num - 1) * d / r + 4 * u
        err = float(np.abs(s[:, col].astype(rule.LD) - rs[:, 0]).max())
        print(f'LASTBIT col {col} err {err:.3e} worst case {worst:.3e} e_ref {e_s:.3e}')
        assert err <= worst, (col, err, worst)
        if np.isfinite(e_s):
            check_bound(s[:, col:col + 1], rs, e_s, 0, f'scaled lastbit col {col}')
        # (else: the float64 oracle itself returns NaN for this column -- with the change in row 0, scipy's transform of the
        #  float64 column comes out exactly constant -- so it has no error to scale the bound by; the worst case above holds)
        check_bound(c[col:col + 1], rc, e_c, 1, f'coef lastbit col {col}')


@pytest.mark.parametrize('n_cols', [1, 63, 64, 65, 130])
def test_forward_kernel_writes_nothing_past_the_width(dd, n_cols):
    """Straight through the C entry: the matrix is a column slice of a wider one and the outputs lie inside larger
    NaN-filled blocks.  What follows the (n_cols, num) coefficients and the (num, n_cols) values must still be NaN
    afterwards: a column guard off by one writes column n_cols of the slice there."""
    import torch
    from dctdomain_amd import _lib
    n_rows, num, slack = 64, 5, 64
    rng = np.random.default_rng(50 + n_cols)
    wide = torch.from_numpy(rng.standard_normal((n_rows, n_cols + 70)).astype(np.float32)).cuda()
    x = wide[:, 3:3 + n_cols]
    coef = torch.full(((n_cols + slack) * num,), NAN, dtype=torch.float64, device='cuda')
    scaled = torch.full((num * n_cols + slack * num,), NAN, dtype=torch.float64, device='cuda')
    ctx = _lib.get_context(torch.cuda.current_device())
    stream = torch.cuda.current_stream()
    _lib.check(ctx._lib.dctfp_idct_quant(ctx.handle, x.data_ptr(), _lib.DCTFP_F32, n_rows, n_cols, wide.stride(0), num,
                                         scaled.data_ptr(), coef.data_ptr(), C.c_void_p(stream.cuda_stream)))
    torch.cuda.synchronize()
    coef, scaled = coef.cpu().numpy(), scaled.cpu().numpy()
    assert np.isnan(coef[n_cols * num:]).all(), 'coefficients written past column n_cols - 1'
    assert np.isnan(scaled[n_cols * num:]).all()
    rc, rs = rule.idct_quant(x.cpu().numpy(), num)
    xh = x.cpu().numpy().astype(np.float64)
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        e_c, e_s = rule.max_err(orc.coefficients(xh, num), rc), rule.max_err(orc.idct_quant(xh, num), rs)
    check_bound(coef[:n_cols * num].reshape(n_cols, num), rc, e_c, 1, f'coef fence {n_cols}')
    check_bound(scaled[:n_cols * num].reshape(num, n_cols), rs, e_s, 0, f'scaled fence {n_cols}')


# -------------------------------------------------------------------------------------------------------------------
# the tie to the hot path
# -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('d,length,seed', rule.HOT_CASES)
def test_methods_compose_to_quantize(dd, fp, d, length, seed):
    """``Z = idct_quant(idct_quant(x, 3).T, 80).T`` by the methods, against ``quantize([3, 80])`` of the same matrix:
    q == trunc(127 Z) wherever 127 Z is at least 1e-6 away from an integer (the scale's own exact 0 and 1 included: they are
    integers in any arithmetic), and at most 0.1 % of a case may be closer than that."""
    x = rule.hot_matrix(d, length, seed)
    z = fp.idct_quant(fp.idct_quant(x, 3).T, 80).T
    assert z.shape == (3, 80)
    one = dd.Fingerprint(pid='t', seq='A' * length, embed={0: x}, domains=[f'1-{length}'])
    one.quantize([3, 80])
    q = one.quants[f'1-{length}'].reshape(3, 80)
    near = rule.near_integer(z)
    assert near.mean() <= 1e-3
    np.testing.assert_array_equal(np.trunc(127.0 * z)[~near].astype(np.int64), q[~near])


# -------------------------------------------------------------------------------------------------------------------
# scale
# -------------------------------------------------------------------------------------------------------------------

def np_scale(v):
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        return (v - np.min(v)) / (np.max(v) - np.min(v))


def same(got, exp):
    """Equal element for element (atol = 0), NaN where and only where numpy has NaN."""
    np.testing.assert_array_equal(np.isnan(got), np.isnan(exp))
    np.testing.assert_array_equal(got[~np.isnan(exp)], exp[~np.isnan(exp)])


LENGTHS = (1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 1025, 70001)
SPOTS = (0, 63, 64, 255, 256, -1)


@pytest.mark.parametrize('n', LENGTHS)
def test_scale_matches_numpy(fp, n):
    rng = np.random.default_rng(900 + n)
    v = rng.standard_normal(n)
    poison(n)
    got = fp.scale(v)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (n,)
    same(got, np_scale(v))
    if n == 1:
        assert np.isnan(got).all()
    # the unique minimum / maximum at every wave of the workgroup, in the tail past 256 and at the very end
    spots = sorted({s % n for s in SPOTS if -n <= s < n})
    for i in spots:
        for j in spots:
            if i == j:
                continue
            w = v.copy()
            w[i], w[j] = -50.0 - i, 60.0 + j
            got = fp.scale(w)
            same(got, np_scale(w))
            assert got[i] == 0.0 and got[j] == 1.0
    for at in {n - 1, 255 % n}:                   # one NaN, seen by one lane only
        w = v.copy()
        w[at] = np.nan
        assert np.isnan(fp.scale(w)).all()
    assert np.isnan(fp.scale(np.full(n, 3.25))).all()            # max == min


def test_scale_infinities_zeros_and_denormals(fp):
    rng = np.random.default_rng(31)
    for n in (65, 257, 1025):
        v = rng.standard_normal(n)
        for plant_at in ([(n - 1, np.inf)], [(0, -np.inf)], [(64, np.inf), (n - 1, -np.inf)], [(3, np.inf), (n - 2, np.inf)]):
            w = v.copy()
            for i, val in plant_at:
                w[i] = val
            same(fp.scale(w), np_scale(w))
        w = np.where(rng.random(n) < 0.5, -0.0, 0.0)
        same(fp.scale(w), np_scale(w))                            # -0.0 == 0.0: max == min, all NaN
        assert np.isnan(fp.scale(w)).all()
        w[n // 2] = 1.5
        same(fp.scale(w), np_scale(w))
        w = rng.integers(-40, 40, n) * 5e-324 * 1000.0            # denormals
        assert (np.abs(w) < np.finfo(np.float64).tiny).all() and len(np.unique(w)) > 2
        same(fp.scale(w), np_scale(w))
        w = v * 1e-310
        same(fp.scale(w), np_scale(w))


def test_scale_shapes_and_tensors(fp):
    import torch
    rng = np.random.default_rng(32)
    m = rng.standard_normal((7, 93))
    got = fp.scale(m)
    assert got.shape == (7, 93)
    same(got, np_scale(m))
    same(fp.scale(m.T), np_scale(m.T))                            # non-contiguous numpy
    t = torch.from_numpy(rng.standard_normal((300, 6))).cuda()
    view = t[::2, 1:4]
    assert not view.is_contiguous()
    got = fp.scale(view)
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float64 and got.shape == view.shape
    same(got.cpu().numpy(), np_scale(view.cpu().numpy()))
    t32 = torch.from_numpy(rng.standard_normal(513).astype(np.float32)).cuda()
    got = fp.scale(t32)
    assert got.dtype == torch.float64 and got.is_cuda
    same(got.cpu().numpy(), np_scale(t32.cpu().numpy().astype(np.float64)))
    v32 = rng.standard_normal(257).astype(np.float32)            # float32 numpy: promoted
    same(fp.scale(v32), np_scale(v32.astype(np.float64)))


# -------------------------------------------------------------------------------------------------------------------
# get_doms
# -------------------------------------------------------------------------------------------------------------------

def domains(n_rows):
    """Domain strings for a matrix of ``n_rows`` >= 700 rows: 1, 2 and 40 pieces, a repeated piece, single rows, one long piece
    beside many one-row pieces (the grid is sized by the longest), 600 rows (at 1 280 columns more than 2 048 x 256 elements:
    the stride loop goes round again), pieces the cleaning drops."""
    return ['20-25', '1-1', f'{n_rows}-{n_rows}', '5-9,300-340', '20-25,20-25',
            ','.join(f'{7 * i + 1}-{7 * i + 1 + i % 5}' for i in range(40)),
            ','.join(f'{i}-{i}' for i in range(3, 40, 2)),
            '2-2,' * 30 + '50-400,' + ','.join(f'{i}-{i}' for i in range(600, 640)),
            '41-640', f'1-{n_rows}', f'10-20,{n_rows + 1}-{n_rows + 5},30-40,50-60', f'{n_rows - 3}-{n_rows + 9}']


def masked(x, pieces):
    """``x`` with every row outside the pieces set to NaN: a row gathered from the wrong place shows as NaN."""
    keep = np.zeros(x.shape[0], dtype=bool)
    for b, e in pieces:
        keep[max(b, 0):e] = True
    y = x.copy()
    y[~keep] = np.nan
    return y


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('n_cols', [1, 3, 257, 1280])
def test_get_doms_matches_the_oracle(fp, n_cols, dtype):
    import torch
    n_rows = 701
    x = np.random.default_rng(600 + n_cols).standard_normal((n_rows, n_cols)).astype(dtype)
    for dom in domains(n_rows):
        pieces, key = orc.split_domain(dom, n_rows)
        y = masked(x, pieces)
        exp, _ = orc.get_doms(y, dom)
        assert exp.shape[0] > 0 and not np.isnan(exp).any()
        poison(*exp.shape)
        got, got_key = fp.get_doms(y, dom)
        assert got_key == key
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == exp.shape
        assert not np.isnan(got).any(), dom
        np.testing.assert_array_equal(got, exp, err_msg=dom)
        # the same rows out of a column slice of a wider CUDA tensor: ld > n_cols
        wide = torch.full((n_rows, n_cols + 9), NAN, dtype=torch.from_numpy(y).dtype, device='cuda')
        wide[:, 3:3 + n_cols] = torch.from_numpy(y).cuda()
        poison(*exp.shape)
        got, got_key = fp.get_doms(wide[:, 3:3 + n_cols], dom)
        assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float64 and got_key == key
        np.testing.assert_array_equal(got.cpu().numpy(), exp, err_msg=dom)


def test_get_doms_that_cleans_to_nothing(fp):
    import torch
    x = np.random.default_rng(7).standard_normal((30, 65)).astype(np.float32)
    for dom in ('31-40', '40-50,31-35'):
        exp, key = orc.get_doms(x, dom)
        got, got_key = fp.get_doms(x, dom)
        assert got_key == key and exp.shape == (0, 65)
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (0, 65)
        got, _ = fp.get_doms(torch.from_numpy(x).cuda(), dom)
        assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (0, 65)


# -------------------------------------------------------------------------------------------------------------------
# error codes of the three entry points
# -------------------------------------------------------------------------------------------------------------------

class Direct:
    """The product library through ctypes, on buffers large enough for every refused call had it gone through."""

    def __init__(self):
        import torch
        from dctdomain_amd import _lib
        self.torch, self.L = torch, _lib
        self.ctx = _lib.get_context(torch.cuda.current_device())
        self.lib = self.ctx._lib
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.x = torch.from_numpy(np.random.default_rng(8).standard_normal((70000, 1)).astype(np.float32)).cuda()
        self.out = torch.full((70000,), NAN, dtype=torch.float64, device='cuda')
        self.out2 = torch.full((70000,), NAN, dtype=torch.float64, device='cuda')
        self.good = None

    def last_error(self):
        return self.lib.dctfp_last_error().decode()

    def idct(self, n_rows, n_cols, ld, num, dtype=None, vec=True, scaled=True, coef=True):
        return self.lib.dctfp_idct_quant(self.ctx.handle, self.x.data_ptr() if vec else None, self.L.DCTFP_F32 if dtype is None else dtype,
                                         n_rows, n_cols, ld, num, self.out.data_ptr() if scaled else None,
                                         self.out2.data_ptr() if coef else None, self.stream)

    def good_idct(self):
        """A correct call on the same context: 64 rows x 5 columns of the buffer, num 3, the right answer."""
        self.out.fill_(NAN)
        self.out2.fill_(NAN)
        assert self.idct(64, 5, 5, 3) == self.L.DCTFP_OK
        self.torch.cuda.synchronize()
        if self.good is None:
            xh = self.x[:320].cpu().numpy().reshape(64, 5)
            rc, rs = rule.idct_quant(xh, 3)
            x64 = xh.astype(np.float64)
            self.good = (rc, rs, rule.max_err(orc.coefficients(x64, 3), rc), rule.max_err(orc.idct_quant(x64, 3), rs))
        rc, rs, e_c, e_s = self.good
        check_bound(self.out[:15].cpu().numpy().reshape(3, 5), rs, e_s, 0, 'scaled after a refusal')
        check_bound(self.out2[:15].cpu().numpy().reshape(5, 3), rc, e_c, 1, 'coef after a refusal')
        assert self.torch.isnan(self.out[15:]).all() and self.torch.isnan(self.out2[15:]).all()


@pytest.fixture(scope='module')
def direct(dd):
    return Direct()


def test_idct_quant_refusals(direct):
    L = direct.L
    refusals = [('num > n_rows', dict(n_rows=64, n_cols=5, ld=5, num=65), L.DCTFP_ERR_SHAPE),
                ('num = 65536', dict(n_rows=70000, n_cols=1, ld=1, num=65536), L.DCTFP_ERR_LIMIT),
                ('ld < n_cols', dict(n_rows=64, n_cols=5, ld=4, num=3), L.DCTFP_ERR_INVALID),
                ('num = 0', dict(n_rows=64, n_cols=5, ld=5, num=0), L.DCTFP_ERR_INVALID),
                ('float16', dict(n_rows=64, n_cols=5, ld=5, num=3, dtype=L.DCTFP_F16), L.DCTFP_ERR_INVALID),
                ('bfloat16', dict(n_rows=64, n_cols=5, ld=5, num=3, dtype=L.DCTFP_BF16), L.DCTFP_ERR_INVALID),
                ('NULL matrix', dict(n_rows=64, n_cols=5, ld=5, num=3, vec=False), L.DCTFP_ERR_INVALID)]
    for name, kw, code in refusals:
        direct.out.fill_(NAN)
        direct.torch.cuda.synchronize()
        assert direct.idct(**kw) == code, name
        assert 'dctfp_idct_quant' in direct.last_error(), name
        direct.torch.cuda.synchronize()
        assert direct.torch.isnan(direct.out).all(), f'{name}: refused, yet something was written'
        direct.good_idct()
    # both outputs NULL: accepted, runs the forward kernel into the scratch
    assert direct.idct(64, 5, 5, 3, scaled=False, coef=False) == L.DCTFP_OK
    direct.torch.cuda.synchronize()
    direct.good_idct()


def test_scale_refusal(direct):
    L, torch = direct.L, direct.torch
    v = torch.from_numpy(np.random.default_rng(9).standard_normal(300)).cuda()
    out = torch.full((300,), NAN, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    assert direct.lib.dctfp_scale(direct.ctx.handle, v.data_ptr(), 0, out.data_ptr(), direct.stream) == L.DCTFP_ERR_INVALID
    assert 'dctfp_scale' in direct.last_error()
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    assert direct.lib.dctfp_scale(direct.ctx.handle, v.data_ptr(), 300, out.data_ptr(), direct.stream) == L.DCTFP_OK
    torch.cuda.synchronize()
    same(out.cpu().numpy(), np_scale(v.cpu().numpy()))


def test_gather_rows_refusals(direct):
    L, torch = direct.L, direct.torch
    n_rows, n_cols = 40, 3
    x = torch.from_numpy(np.random.default_rng(10).standard_normal((n_rows + 8, n_cols)).astype(np.float32)).cuda()
    out = torch.full((65536 + 64, n_cols), NAN, dtype=torch.float64, device='cuda')

    def gather(rec, n_pieces):
        return direct.lib.dctfp_gather_rows(direct.ctx.handle, x.data_ptr(), L.DCTFP_F32, n_rows, n_cols, n_cols, rec.ctypes.data,
                                            n_pieces, out.data_ptr(), direct.stream)

    def pieces(spans):
        rec = np.zeros(len(spans), dtype=L.PIECE_DTYPE)
        rec['row_start'] = [s for s, _ in spans]
        rec['n_rows'] = [n for _, n in spans]
        return rec

    many = pieces([(i % n_rows, 1) for i in range(65536)])
    refusals = [('a piece ending one row past the matrix', pieces([(0, 4), (n_rows - 3, 4)]), 2),
                ('n_pieces = 0', pieces([(0, 4)]), 0),
                ('n_pieces = 65536', many, 65536)]
    for name, rec, n in refusals:
        torch.cuda.synchronize()
        assert gather(rec, n) == L.DCTFP_ERR_INVALID, name
        assert 'dctfp_gather_rows' in direct.last_error(), name
        torch.cuda.synchronize()
        assert torch.isnan(out).all(), f'{name}: refused, yet something was written'
        good = pieces([(5, 3), (n_rows - 4, 4)])
        assert gather(good, 2) == L.DCTFP_OK
        torch.cuda.synchronize()
        xh = x.cpu().numpy().astype(np.float64)
        np.testing.assert_array_equal(out[:7].cpu().numpy(), np.concatenate([xh[5:8], xh[n_rows - 4:n_rows]]))
        assert torch.isnan(out[7:]).all()
        out.fill_(NAN)
