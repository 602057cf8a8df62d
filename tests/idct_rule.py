"""``Fingerprint.idct_quant`` (src/fingerprint.py:126-142 of the reference) restated in closed form in ``numpy.longdouble``
-- TEST HELPER, no GPU, no scipy.

    f[c, k]   = s_k * sum_t cos(pi k (2t+1) / (2N)) x[t, c]         orthonormal DCT-II along axis 0 (N = n_rows)
    y[j, c]   = sum_{k < num} s'_k cos(pi k (2j+1) / (2 num)) f[c, k]  its inverse at length ``num`` on the kept ``num``
    out[j, c] = (y[j, c] - min_j y) / (max_j y - min_j y)           min-max scale per column

with s_0 = sqrt(1/N), s_k = sqrt(2/N) (s' the same at length ``num``).  Every cosine takes its argument reduced exactly in
integers to [0, pi/4] first, so a table entry is good to the last bits of the 64-bit mantissa.

For k >= 1 the first row is subtracted from every row before the sum (sum_t cos(pi k (2t+1) / (2N)) = 0, so this changes
nothing in exact arithmetic).  It makes the rule well defined where the reference is not: an exactly constant column has
y == 0 exactly, max == min, and scales to 0/0 = NaN -- what the product documents (CONSTANT_CHANNEL_NOTE); without the shift
a constant column would scale the rule's own 1e-19 round-off.

NaN rule: a column with a NaN among its ``num`` values y is NaN throughout; max == min gives NaN.  (An infinity in a column
makes every y of it an infinity or a NaN, and (inf - inf) / inf is NaN: NaN throughout as well.)

The module also holds the case matrix the GPU tests of the single-matrix API run (``CASES``), so that the host tests measure
the float64 oracle's own error ``e_ref`` on exactly those inputs.
"""

from __future__ import annotations

import functools
import warnings

import numpy as np

LD = np.longdouble
# an 80-bit x87 long double (64-bit mantissa) or better; a host where long double is a double must fail loudly, not skip
assert np.finfo(LD).eps < 2e-19, f'numpy.longdouble has eps {np.finfo(LD).eps}: this helper needs an 80-bit long double'

PI = LD('3.14159265358979323846264338327950288419716939937510')


def cos_table(n_out: int, n: int) -> np.ndarray:
    """``C[k, t] = cos(pi k (2t+1) / (2n))``, k < n_out, t < n, as longdouble; argument reduced in integers."""
    assert 4 * max(n_out, 1) * (2 * n + 1) < 2 ** 62
    k = np.arange(n_out, dtype=np.int64)[:, None]
    t = np.arange(n, dtype=np.int64)[None, :]
    q = 2 * n
    p = (k * (2 * t + 1)) % (2 * q)               # cos(pi p / q), period 2q
    p = np.where(p > q, 2 * q - p, p)             # cos(2 pi - a) = cos(a):   p in [0, q]
    neg = 2 * p > q
    p = np.where(neg, q - p, p)                   # cos(pi - a) = -cos(a):    p in [0, q/2]
    use_sin = 4 * p > q                           # cos(a) = sin(pi/2 - a):   argument in [0, pi/4]
    num = np.where(use_sin, q - 2 * p, 2 * p).astype(LD)     # over 2q
    arg = PI * num / LD(2 * q)
    val = np.where(use_sin, np.sin(arg), np.cos(arg))
    return np.where(neg, -val, val).astype(LD)


def _norms(n_out: int, n: int) -> np.ndarray:
    s = np.full(n_out, np.sqrt(LD(2) / LD(n)), dtype=LD)
    s[0] = np.sqrt(LD(1) / LD(n))
    return s


def coefficients(x, num: int) -> np.ndarray:
    """``f[:, :num]`` of src/fingerprint.py:137 for an (n_rows, n_cols) matrix: (n_cols, min(num, n_rows)) longdouble."""
    x = np.asarray(x).astype(LD)
    n = x.shape[0]
    k = min(int(num), n)
    with np.errstate(all='ignore'):
        f = np.empty((k, x.shape[1]), dtype=LD)
        f[0] = x.sum(axis=0)
        if k > 1:
            f[1:] = cos_table(k, n)[1:] @ (x - x[0:1])
        return (f * _norms(k, n)[:, None]).T


def resampled(x, num: int):
    """(coefficients (n_cols, k), y (k, n_cols) before the scale), k = min(num, n_rows), both longdouble.  y leaves the k = 0
    term out: it is the same for every j and drops out of the min-max scale, and without it a constant column is exactly 0,
    not its mean +- round-off."""
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        coef = coefficients(x, num)
        k = coef.shape[1]
        basis = cos_table(k, k) * _norms(k, k)[:, None]                  # [k, j]
        y = basis[1:].T @ coef.T[1:] if k > 1 else np.zeros((k, coef.shape[0]), dtype=LD)
        return coef, y


def idct_quant(x, num: int, want_y: bool = False):
    """(coefficients (n_cols, k), scaled values (k, n_cols)), k = min(num, n_rows), both longdouble."""
    coef, y = resampled(x, num)
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        bad = np.isnan(y).any(axis=0)
        mx = np.where(np.isnan(y), -np.inf, y).max(axis=0)
        mn = np.where(np.isnan(y), np.inf, y).min(axis=0)
        den = mx - mn
        den = np.where(den == 0, LD('nan'), den)
        scaled = (y - mn) / den
        scaled[:, bad] = LD('nan')
        return (coef, scaled, y) if want_y else (coef, scaled)


# ------------------------------------------------------------------------------------------------------------------
# The case matrix of tests/test_single_matrix_gpu.py (and of the e_ref table in tests/test_idct_rule_host.py)
# ------------------------------------------------------------------------------------------------------------------

N_COLS = (1, 63, 64, 65, 130, 1280)
#: (n_rows, num) run at EVERY width: every num edge 1, 2, 3, 5, 80, 128, num == n_rows at 1, 2, 5 and 64, and every
#: n_rows but 2000
ROWS_NUM = ((1, 1), (2, 2), (3, 2), (3, 1), (5, 3), (5, 5), (64, 5), (64, 64), (257, 80), (257, 128))
#: the long transform (2 000 terms per sum) where it is cheap, once at the full width, and num == n_rows == 257
EXTRA = ((2000, 63, 128), (2000, 130, 128), (2000, 65, 80), (2000, 1280, 80), (2000, 64, 2), (2000, 1, 2000), (257, 65, 257))

RECIPES = ('esm', 'gauss', 'big', 'small', 'ramp')
#: how the matrix reaches the method.  np16 / npi32 / bf16: the values are rounded to that type first and the expected
#: values are those of the promoted matrix.  slice: columns 3 .. 3 + n_cols of a wider CUDA tensor (ld > n_cols, base
#: pointer 12 bytes into a row).  np64T / cuda32T: the transposed view of an (n_cols, n_rows) matrix, as the reference's own
#: second call ``idct_quant(a.T, m)``.
FORMS = ('np32', 'np64', 'np16', 'npi32', 'cuda32', 'slice', 'np64T', 'cuda32T', 'bf16')


def _cases():
    shapes = [(r, c, k) for c in N_COLS for r, k in ROWS_NUM] + list(EXTRA)
    out = []
    for i, (r, c, k) in enumerate(shapes):
        recipe, form = RECIPES[i % len(RECIPES)], FORMS[i % len(FORMS)]
        if recipe in ('big', 'small') and form in ('np16', 'npi32'):
            recipe = 'esm'                       # (1e30 is no float16 and no int32)
        out.append(dict(id=f'{r}x{c}_num{k}_{recipe}_{form}', n_rows=r, n_cols=c, num=k, recipe=recipe, form=form, seed=1000 + i))
    return out


CASES = _cases()


def recipe_matrix(recipe: str, n_rows: int, n_cols: int, seed: int) -> np.ndarray:
    """float64 (n_rows, n_cols).  esm: per-channel scale and offset and a few channels offset by +-200 (the cancellation the
    first-row shift exists for); gauss; big / small: gauss times 1e30 / 1e-30; ramp: gauss with a pure ramp in one column."""
    rng = np.random.default_rng(seed)
    if recipe == 'esm':                          # (tests/golden/recipes.py 'esm', kept in float64)
        ch_scale = np.exp(rng.standard_normal(n_cols))
        ch_off = 5.0 * rng.standard_normal(n_cols)
        idx = rng.choice(n_cols, size=max(1, n_cols // 100), replace=False)
        ch_off[idx] += 200.0 * rng.choice([-1.0, 1.0], size=len(idx))
        return rng.standard_normal((n_rows, n_cols)) * ch_scale + ch_off
    x = rng.standard_normal((n_rows, n_cols))
    if recipe == 'big':
        x *= 1e30
    elif recipe == 'small':
        x *= 1e-30
    elif recipe == 'ramp':
        x[:, n_cols // 2] = 0.25 * np.arange(n_rows) - 3.0
    elif recipe != 'gauss':
        raise KeyError(recipe)
    return x


def promoted_matrix(case) -> np.ndarray:
    """The matrix of a case as the kernels see it after promotion: float32 or float64 numpy, C order."""
    x = recipe_matrix(case['recipe'], case['n_rows'], case['n_cols'], case['seed'])
    form = case['form']
    if form == 'np16':
        return x.astype(np.float16).astype(np.float32)
    if form == 'npi32':
        return np.rint(x * 16).astype(np.int32).astype(np.float64)
    if form == 'bf16':
        import torch
        return torch.from_numpy(x.astype(np.float32)).to(torch.bfloat16).to(torch.float32).numpy()
    if form in ('np64', 'np64T'):
        return x
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _reference(index: int):
    case = CASES[index]
    x = promoted_matrix(case)
    coef, scaled, y = idct_quant(x, case['num'], want_y=True)
    return x, coef, scaled, y


def reference(case):
    """(promoted matrix, coefficients, scaled values) of a case of ``CASES``; computed once, shared, not to be written to."""
    out = _reference(CASES.index(case))
    for a in out:
        a.setflags(write=False)
    return out[:3]


def reference_y(case):
    """The resampled values of a case before the scale, (num, n_cols) longdouble."""
    return _reference(CASES.index(case))[3]


def max_err(got, ref) -> float:
    """max |got - ref| over the elements where ``ref`` is finite (0.0 where none is)."""
    ref = np.asarray(ref)
    ok = np.isfinite(ref)
    if not ok.any():
        return 0.0
    with np.errstate(all='ignore'):
        return float(np.abs(np.asarray(got).astype(LD)[ok] - ref[ok]).max())


@functools.lru_cache(maxsize=None)
def _oracle_error(index: int):
    from oracle import dct_oracle as orc
    case = CASES[index]
    x, coef, scaled = reference(case)
    x64 = np.asarray(x, dtype=np.float64)
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        return max_err(orc.coefficients(x64, case['num']), coef), max_err(orc.idct_quant(x64, case['num']), scaled)


def oracle_error(case):
    """``e_ref`` of a case: max |float64 scipy oracle - longdouble rule| of (the coefficients, the scaled values), over the
    elements where the rule is finite."""
    return _oracle_error(CASES.index(case))


def ulp_floor(ref, axis: int) -> np.ndarray:
    """4 ulp (float64) of the largest finite magnitude of each column of the INPUT matrix's results: ``axis`` is the axis of
    ``ref`` that runs over one column's values (1 for coefficients (n_cols, k), 0 for scaled values (k, n_cols))."""
    mag = np.where(np.isfinite(ref), np.abs(ref), 0).max(axis=axis, keepdims=True).astype(np.float64)
    return 4.0 * np.spacing(mag)


#: the matrices of the tie to the hot path: (D, L, seed), recipe 'esm' in float32, qdim [3, 80], one domain 1-L
HOT_CASES = ((640, 25, 11), (1280, 300, 12), (640, 300, 13))
NEAR = 1e-6          # 127 z closer to an integer than this: trunc() may go either way, the element is not compared


def hot_matrix(d: int, length: int, seed: int) -> np.ndarray:
    from recipes import make_input
    return make_input('esm', length, d, seed)


def near_integer(z) -> np.ndarray:
    """Elements of z whose 127 z is closer than NEAR to an integer WITHOUT being one of the scale's own exact values: every row
    of a min-max scale holds an exact 0.0 and an exact 1.0 ((min - min) / den, den / den) in any arithmetic; 127 * 0 and
    127 * 1 are integers by construction, not by accident, and stay compared."""
    v = 127.0 * np.asarray(z, dtype=np.float64)
    with np.errstate(all='ignore'):
        return (np.abs(v - np.rint(v)) < NEAR) & (z != 0.0) & (z != 1.0)
