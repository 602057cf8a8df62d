"""The longdouble rule of ``idct_quant`` (tests/idct_rule.py) against the float64 scipy oracle and the committed golden
intermediates -- CPU only.  It also measures the yardstick of tests/test_single_matrix_gpu.py: for every case of
``idct_rule.CASES``

    e_ref = max |float64 oracle - longdouble rule|        (coefficients; scaled values)

The bounds asserted here come from the oracle's arithmetic, not from what it gives: an FFT of length 2N in float64 has a
relative l2 error of a few eps * log2(2N) (Higham, Accuracy and Stability, 24.1), and ||f||_2 = ||x||_2 <= sqrt(N) max|x| for
an orthonormal transform, so every coefficient of a column is off by at most

    E_f = 8 eps log2(2N + 2) sqrt(N) max|x_col|

(8: the pre- and post-twiddles of a DCT by FFT on top of the butterflies).  The inverse of length num adds its own share of
the same form and passes E_f on with norm 1: |y err| <= E_y = 2 sqrt(num) E_f.  A min-max scale of values with range R turns
that into at most 4 E_y / R ((y - mn) and (mx - mn) each carry 2 E_y).

Worst e_ref per recipe over the case matrix, measured with scipy 1.15.3 (python tests/test_idct_rule_host.py prints every
case):

    recipe   coefficients / max|coef|   scaled values
    esm       2.83e-16                   1.04e-13
    gauss     4.35e-16                   1.05e-15
    ramp      1.65e-16                   4.75e-15
    big       3.80e-16                   4.66e-16
    small     4.35e-16                   5.69e-16

(esm: the channels offset by +-200 lose the digits of the offset in the oracle, which does not shift by the first row.)
"""

import json
import warnings

import numpy as np
import pytest

import golden_util as gu
import idct_rule as rule
from oracle import dct_oracle as orc

EPS = np.finfo(np.float64).eps
IDS = [c['id'] for c in rule.CASES]


def test_long_double_is_80_bit():
    assert np.finfo(np.longdouble).eps < 2e-19


def test_case_matrix_covers_every_axis_value_and_edge_pair():
    rows = {c['n_rows'] for c in rule.CASES}
    cols = {c['n_cols'] for c in rule.CASES}
    assert rows == {1, 2, 3, 5, 64, 257, 2000} and cols == {1, 63, 64, 65, 130, 1280}
    for n_cols in cols:
        nums = {c['num'] for c in rule.CASES if c['n_cols'] == n_cols}
        assert {1, 2, 3, 5, 80, 128} <= nums, n_cols
        assert any(c['num'] == c['n_rows'] and c['num'] > 1 for c in rule.CASES if c['n_cols'] == n_cols)
    assert {c['form'] for c in rule.CASES} == set(rule.FORMS)
    assert {c['recipe'] for c in rule.CASES} == set(rule.RECIPES)
    assert all(1 <= c['num'] <= c['n_rows'] for c in rule.CASES)
    assert len(set(IDS)) == len(IDS)


def test_cosines_are_exact_where_they_are_known():
    c = rule.cos_table(7, 6)                     # cos(pi k (2t+1) / 12)
    assert c[3, 0] == np.sqrt(rule.LD(2)) / 2 or abs(c[3, 0] - np.sqrt(rule.LD(2)) / 2) <= np.finfo(rule.LD).eps
    assert c[6, 0] == 0 and c[6, 5] == 0         # cos(pi/2), cos(11 pi / 2): exact zeros, not 6e-17
    assert c[2, 1] == 0                          # cos(pi 2 3 / 12)
    assert (c[0] == 1).all()
    big = rule.cos_table(128, 2000)
    assert abs(big.sum(axis=1)[1:]).max() < 2000 * np.finfo(rule.LD).eps      # sum_t cos(pi k (2t+1) / 2N) = 0


def _bounds(x, num):
    n = x.shape[0]
    colmax = np.abs(np.asarray(x, dtype=np.float64)).max(axis=0)
    e_f = 8 * EPS * np.log2(2 * n + 2) * np.sqrt(n) * colmax                   # per column
    return e_f, 2 * np.sqrt(num) * e_f


@pytest.mark.parametrize('case', rule.CASES, ids=IDS)
def test_rule_agrees_with_the_scipy_oracle(case):
    x, coef, scaled = rule.reference(case)
    x64 = np.asarray(x, dtype=np.float64)
    num = case['num']
    assert coef.shape == (case['n_cols'], num) and scaled.shape == (num, case['n_cols'])
    assert coef.dtype == np.longdouble and scaled.dtype == np.longdouble
    e_f, e_y = _bounds(x, num)
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        oc = orc.coefficients(x64, num)
        osc = orc.idct_quant(x64, num)
    y = rule.reference_y(case)
    assert np.isfinite(coef).all()
    assert (np.abs(oc - coef) <= e_f[:, None] + 1e-300).all(), np.abs(oc - coef).max()
    if num == 1:
        assert np.isnan(scaled).all()            # one value: 0/0
        return
    rng_y = y.max(axis=0) - y.min(axis=0)
    const = np.isnan(scaled).any(axis=0)
    assert (const == (rng_y == 0)).all()         # NaN exactly where the column is constant (int32 rounding makes some)
    ok = ~const
    with np.errstate(all='ignore'):
        bound = (4 * e_y / rng_y.astype(np.float64))[None, :]
        err = np.abs(osc - scaled).astype(np.float64)
    # (where the bound itself passes 1 the oracle has no correct digit left: a column nearly constant next to its offset)
    assert (err[:, ok] <= bound[:, ok]).all(), (err[:, ok] / bound[:, ok]).max()
    e_coef, e_scaled = rule.oracle_error(case)
    assert np.isfinite(e_coef) and np.isfinite(e_scaled)
    assert ((scaled[:, ok] >= 0) & (scaled[:, ok] <= 1)).all()
    assert (scaled[:, ok].min(axis=0) == 0).all() and (scaled[:, ok].max(axis=0) == 1).all()


def test_rule_agrees_with_the_golden_intermediates():
    """coef, Yp, Z of the golden cases that carry them were written by the reference itself (scipy, float64)."""
    arr = gu.arrays()
    checked = 0
    for case in gu.cases(expect='ok'):
        if not case.get('intermediates'):
            continue
        layers = gu.build_layers(case)
        n, m = case['qdim'][0], case['qdim'][1]
        x, _ = orc.get_doms(layers[0], case['domains'][0])
        coef, yp, y = rule.idct_quant(x, n, want_y=True)
        e_f, e_y = _bounds(x, n)
        assert (np.abs(arr[f"{case['id']}/coef"] - coef) <= e_f[:, None]).all(), case['id']
        r = (y.max(axis=0) - y.min(axis=0)).astype(np.float64)
        assert (np.abs(arr[f"{case['id']}/Yp"] - yp) <= (4 * e_y / r)[None, :]).all(), case['id']
        # second call, on the rule's own Y' (values in [0, 1]: the golden Y' differs from it by the bound just checked, and
        # the scale passes that on divided by the range of the resampled row)
        yp64 = yp.astype(np.float64)
        _, z, y2 = rule.idct_quant(yp64.T, m, want_y=True)
        r2 = (y2.max(axis=0) - y2.min(axis=0)).astype(np.float64)
        e_f2, e_y2 = _bounds(yp64.T, m)
        carried = 4 * np.sqrt(yp64.shape[1]) * np.abs(arr[f"{case['id']}/Yp"] - yp64).max()
        assert (np.abs(arr[f"{case['id']}/Z"].T - z) <= ((4 * e_y2 + carried) / r2)[None, :]).all(), case['id']
        checked += 1
    assert checked >= 6


def test_rule_nan_inf_and_constant_columns():
    rng = np.random.default_rng(3)
    base = rng.standard_normal((40, 6))
    _, ref = rule.idct_quant(base, 5)
    for value in (np.nan, np.inf, -np.inf):
        x = base.copy()
        x[17, 2] = value
        coef, s = rule.idct_quant(x, 5)
        assert np.isnan(s[:, 2]).all()
        keep = [0, 1, 3, 4, 5]
        assert (s[:, keep] == ref[:, keep]).all()
    x = base.copy()
    x[:, 4] = 200.125
    _, s = rule.idct_quant(x, 5)
    assert np.isnan(s[:, 4]).all() and np.isfinite(s[:, :4]).all()
    x[7, 4] = np.nextafter(200.125, 1000.0)
    _, s = rule.idct_quant(x, 5)
    assert np.isfinite(s[:, 4]).all() and s[:, 4].max() == 1 and s[:, 4].min() == 0


@pytest.mark.parametrize('d,length,seed', rule.HOT_CASES)
def test_hot_path_seeds_keep_clear_of_integers(d, length, seed):
    """The GPU tie between the methods and ``quantize`` skips elements whose 127 z lies within 1e-6 of an integer; at most
    0.1 % of a case may be skipped.  The seeds are chosen so that the float64 oracle alone stays under that cap, and the
    longdouble rule agrees with the oracle's int8 wherever neither is that close."""
    x = rule.hot_matrix(d, length, seed)
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        z = orc.idct_quant(orc.idct_quant(x.astype(np.float64), 3).T, 80).T
        q = orc.quantize([x], [f'1-{length}'], [3, 80])[f'1-{length}']
    assert z.shape == (3, 80)
    near = rule.near_integer(z)
    assert near.mean() <= 1e-3
    assert (np.trunc(127.0 * z)[~near].astype(np.int64) == q.reshape(3, 80)[~near]).all()
    _, yp = rule.idct_quant(x, 3)
    _, zl = rule.idct_quant(yp.astype(np.float64).T, 80)
    zl = zl.T
    both = ~near & ~rule.near_integer(zl.astype(np.float64))
    assert (np.trunc(127 * zl)[both].astype(np.int64) == q.reshape(3, 80)[both]).all()


def e_ref_table():
    """Every case's e_ref and the worst per recipe, as printed into this module's docstring."""
    lines, worst = [], {}
    for case in rule.CASES:
        _, coef, _ = rule.reference(case)
        e_coef, e_scaled = rule.oracle_error(case)
        rel = e_coef / float(np.abs(coef).max())
        lines.append(f"{case['id']:40s} coef {e_coef:9.3e} (rel {rel:9.3e})   scaled {e_scaled:9.3e}")
        w = worst.setdefault(case['recipe'], [0.0, 0.0])
        w[0], w[1] = max(w[0], rel), max(w[1], e_scaled)
    return lines, worst


if __name__ == '__main__':
    lines, worst = e_ref_table()
    print('\n'.join(lines))
    for recipe, (a, b) in worst.items():
        print(f'    {recipe:8s} {a:9.2e}                  {b:9.2e}')
    print(json.dumps(worst))
