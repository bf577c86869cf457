"""CPU: the numpy restatement of linear scaling (tests/linear_scaling_ref.py) against numpy.linalg.lstsq and hand cases, and the
rewrite rule on hand-made rows."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import linear_scaling_ref as LS  # noqa: E402
import sr_grad_ref as R  # noqa: E402
import subtree_ref as S  # noqa: E402


def test_matches_lstsq_on_well_conditioned_rows(rng):
    D = 257
    y = rng.normal(0, 2, D).astype(np.float32)
    P = np.stack([rng.normal(rng.uniform(-3, 3), rng.uniform(0.1, 2), D) for _ in range(200)]).astype(np.float32)
    P[:20] += (0.5 * y)[None, :]   # some rows that do explain the labels
    ref = LS.scaling(P, y)
    keep = ref["kappa"] < 1e4
    assert keep.sum() > 150
    for t in np.flatnonzero(keep):
        A = np.stack([np.ones(D), P[t].astype(np.float64)], axis=1)
        (a, b), res, _, _ = np.linalg.lstsq(A, y.astype(np.float64), rcond=None)
        np.testing.assert_allclose([ref["a"][t], ref["b"][t]], [a, b], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(ref["loss"][t], res[0] / D, rtol=1e-9, atol=1e-9 * ref["syy_D"])


def test_hand_cases(rng):
    D = 100
    y = rng.uniform(-1, 3, D).astype(np.float32)
    y64 = y.astype(np.float64)
    P = np.stack([y, (3 * y64 - 2).astype(np.float32), np.full(D, 0.75, np.float32), y]).astype(np.float32)
    P[3, 17] = np.nan
    ref = LS.scaling(P, y)
    # T = y
    np.testing.assert_allclose([ref["b"][0], ref["a"][0], ref["loss"][0]], [1, 0, 0], atol=1e-12)
    # T = 3 y - 2 (rounded to float32 row by row): y = (T + 2) / 3 up to that rounding
    np.testing.assert_allclose([ref["b"][1], ref["a"][1]], [1 / 3, 2 / 3], rtol=1e-6)
    assert 0 <= ref["loss"][1] < 1e-12
    # T constant: the mean of the labels and their variance, kappa 0
    assert ref["b"][2] == 0 and ref["a"][2] == y64.mean() == ref["ybar"] and ref["loss"][2] == ref["syy_D"] == np.var(y64)
    assert ref["kappa"][2] == 0
    # one NaN row
    assert all(np.isnan(ref[k][3]) for k in ("loss", "a", "b", "kappa"))
    # D = 1
    one = LS.scaling(np.array([[2.5], [np.inf]], np.float32), np.array([4.0], np.float32))
    assert one["b"][0] == 0 and one["a"][0] == 4.0 and one["loss"][0] == 0 and np.isnan(one["loss"][1])
    # a coefficient beyond float32: all NaN
    tiny = LS.scaling(np.array([[0, 1e-45, 0, 1e-45]], np.float32), np.array([0, 1e30, 0, 1e30], np.float32))
    assert np.isnan(tiny["loss"][0]) and np.isnan(tiny["a"][0]) and np.isnan(tiny["b"][0])


def test_tolerance_grows_with_the_condition_number():
    rtol, atol = LS.tolerance(np.array([0.0, 1.0, 1e8, np.inf, np.nan]), 5000, 2.0)
    assert atol == 2e-6 and rtol[0] == 1e-6 and rtol[3] == rtol[4] == 1e-6
    np.testing.assert_allclose(rtol[2], 1e-6 + 1e8 * 5000 * 2.0 ** -52)


def test_wrap_rule_on_hand_rows():
    B, V, C = R.T_BFUNC, R.T_VAR, R.T_CONST
    value = np.zeros((5, 8), np.float32)
    type_ = np.zeros((5, 8), np.int16)
    size = np.zeros((5, 8), np.int16)
    value[0, :3], type_[0, :3], size[0, :3] = [R.F_SUB, 0, 1], [B, V, V], [3, 1, 1]         # fits: 3 + 4 <= 8
    value[1, :5], type_[1, :5], size[1, :5] = [R.F_SUB, R.F_MUL, 0, 1, 2.0], [B, B, V, V, C], [5, 3, 1, 1, 1]   # 5 + 4 > 8
    value[2, :1], type_[2, :1], size[2, :1] = [1], [V], [1]                                  # NaN slope
    value[3, :1], type_[3, :1], size[3, :1] = [R.F_ADD], [B], [1]                             # malformed
    value[4, :1], type_[4, :1], size[4, :1] = [0.5], [C], [1]
    coef = np.array([[0.25, -2], [1, 1], [0, np.nan], [1, 1], [np.inf, 1]], np.float32)
    ov, ot, os_, applied = LS.wrap_rows(value, type_, size, coef, 8)
    assert list(applied) == [1, 0, 0, 0, 0]
    assert list(ov[0]) == [R.F_ADD, R.F_MUL, R.F_SUB, 0, 1, -2, 0.25, 0] and list(ot[0]) == [B, B, B, V, V, C, C, 0]
    assert list(os_[0]) == [7, 5, 3, 1, 1, 1, 1, 0] and S.check_prefix_tree(ot[0], os_[0])
    for t in (1, 2, 3, 4):
        assert np.array_equal(ov[t], value[t]) and np.array_equal(ot[t], type_[t]) and np.array_equal(os_[t], size[t])
    ov, ot, os_, applied = LS.wrap_rows(value, type_, size, coef, 12)   # grown rows: row 1 fits now
    assert ov.shape == (5, 12) and list(applied) == [1, 1, 0, 0, 0] and os_[1, 0] == 9 and list(ov[1, 7:]) == [1, 1, 0, 0, 0]
    assert np.array_equal(ov[3, :8], value[3]) and not ov[3, 8:].any()


def test_refit_bound_covers_float32_evaluation(rng):
    D = 300
    y = rng.uniform(-2, 2, D).astype(np.float32)
    P = rng.normal(0, 1, (50, D)).astype(np.float32) + rng.uniform(-5, 5, (50, 1)).astype(np.float32)
    ref = LS.scaling(P, y)
    a32, b32 = ref["a"].astype(np.float32), ref["b"].astype(np.float32)
    wrapped = (P * b32[:, None]) + a32[:, None]   # float32: fl(fl(p b) + a)
    mse = np.mean((y.astype(np.float64)[None, :] - wrapped.astype(np.float64)) ** 2, axis=1)
    assert np.all(np.abs(mse - ref["loss"]) <= LS.refit_bound(P, a32, b32, ref["loss"]))
