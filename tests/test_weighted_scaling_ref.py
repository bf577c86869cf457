"""CPU: the numpy restatement of weighted linear scaling (tests/weighted_scaling_ref.py) against numpy.linalg.lstsq on sqrt(w)-scaled
columns, against the loss taken straight from its definition, against the unweighted restatement (tests/linear_scaling_ref.py), and
every rule of include/evogp_hip.h evogp_hip_sr_weighted_scaling on hand-made predictions."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import linear_scaling_ref as LS  # noqa: E402
import weighted_scaling_ref as WS  # noqa: E402


def _weights(rng, K, D):
    W = rng.uniform(0.5, 2, (K, D)).astype(np.float32)
    W[rng.random((K, D)) < 0.3] = 0
    W[:, :2] = np.maximum(W[:, :2], np.float32(0.5))   # (every row weights at least two data rows)
    return W


def _case(rng, pop, D):
    P = rng.normal(0.0, 2.0, (pop, D)).astype(np.float32) + rng.uniform(-3, 3, (pop, 1)).astype(np.float32)
    y = rng.normal(1.0, 1.5, D).astype(np.float32)
    return P, y


@pytest.mark.parametrize("D", [2, 3, 17, 64])
def test_fit_is_the_weighted_least_squares_solution(rng, D):
    P, y = _case(rng, 12, D)
    W = _weights(rng, 3, D)
    ref = WS.scaling(P, y, W)
    sw = np.sqrt(W[0].astype(np.float64))
    for t in range(12):
        A = np.stack([sw, sw * P[t].astype(np.float64)], axis=1)
        sol, _, rank, _ = np.linalg.lstsq(A, sw * y.astype(np.float64), rcond=None)
        if rank < 2:
            continue
        # lstsq solves by an SVD of a matrix whose condition number is about sqrt(kappa): its own error is cond * 2^-52 times a
        # modest constant, relative to the size of the solution
        tol = 64 * 2.0 ** -52 * max(ref["kappa"][t], 1.0) * (np.abs(sol).max() + 1.0)
        assert abs(ref["a"][t] - sol[0]) <= tol and abs(ref["b"][t] - sol[1]) <= tol, (t, ref["a"][t], ref["b"][t], sol)
    assert np.isfinite(ref["a"]).all()


@pytest.mark.parametrize("K", [None, 1, 2, 8])
def test_loss_is_the_weighted_squared_error_of_the_fitted_model(rng, K):
    D = 50
    P, y = _case(rng, 20, D)
    W = None if K is None else _weights(rng, K, D)
    ref = WS.scaling(P, y, W)
    direct = WS.direct_loss(P, y, W, ref["a"], ref["b"])
    assert ref["loss"].shape == direct.shape == (20, K or 1)
    # both are float64 sums of at most D terms of the size of the loss; the closed form subtracts terms of the size of b^2 M and V
    scale = ref["V_W"][None, :] + direct
    assert np.all(np.abs(ref["loss"] - direct) <= 1e-12 * scale * np.maximum(ref["kappa"], 1.0)[:, None])
    # the fit minimises column 0: no other coefficients give less there
    for da, db in ((1e-3, 0), (-1e-3, 0), (0, 1e-3), (0, -1e-3)):
        other = WS.direct_loss(P, y, W, ref["a"] + da, ref["b"] + db)
        assert np.all(other[:, 0] >= direct[:, 0])


@pytest.mark.parametrize("D", [1, 2, 40, 300])
def test_unit_weights_are_plain_linear_scaling(rng, D):
    P, y = _case(rng, 16, D)
    P[3] = 0.75            # a flat tree
    P[5, D // 2] = np.inf  # a NaN tree
    plain = LS.scaling(P, y)
    for W in (None, np.ones(D, np.float32), np.ones((1, D), np.float32)):
        ref = WS.scaling(P, y, W)
        assert np.array_equal(np.isnan(ref["a"]), np.isnan(plain["a"]))
        ok = np.isfinite(plain["a"])
        for name, got in (("loss", ref["loss"][:, 0]), ("a", ref["a"]), ("b", ref["b"])):
            # two float64 evaluations of one closed form, one centred and one not: the uncentred one carries kappa
            tol = 1e-12 * np.maximum(plain["kappa"][ok], 1.0) * (np.abs(plain[name][ok]) + plain["syy_D"])
            assert np.all(np.abs(got[ok] - plain[name][ok]) <= tol), name
        assert ref["b"][3] == 0 and ref["kappa"][3] == 0
        assert abs(ref["V_W"][0] - plain["syy_D"]) <= 1e-12 * plain["syy_D"] + 1e-300


def test_rules_on_hand_made_predictions(rng):
    D = 12
    y = np.arange(D, dtype=np.float32) * 0.5 - 1.0
    x = np.linspace(-1, 2, D).astype(np.float32)
    train = (np.arange(D) < 8).astype(np.float32)
    W = np.stack([train, 1 - train])
    P = np.stack([x, np.full(D, 0.75, np.float32), x - x, np.where(train > 0, np.float32(2.0), x).astype(np.float32), x, x, x])
    P[4, 9] = np.inf    # held out of row 0, weighted in row 1
    P[5, 2] = np.nan    # weighted in row 0
    P[6] = np.where(train > 0, np.float32(0.0), np.float32(-0.0))   # zeros of both signs: min == max, flat
    ref = WS.scaling(P, y, W)
    # 0: y is an affine map of the row index and so of x: the fit is exact on both rows
    assert abs(ref["b"][0] - 0.5 * (D - 1) / 3.0) < 1e-6 and np.all(ref["loss"][0] < 1e-10)
    # 1, 2, 6: flat trees: slope 0, the intercept is the row-0 weighted mean of the labels, both columns from the same formula
    ybar_train = y[:8].astype(np.float64).mean()
    for t in (1, 2, 3, 6):
        assert ref["b"][t] == 0 and ref["kappa"][t] == 0 and abs(ref["a"][t] - ybar_train) < 1e-12, t
        assert abs(ref["loss"][t, 0] - ((y[:8] - ybar_train) ** 2).mean()) < 1e-12
        assert abs(ref["loss"][t, 1] - ((y[8:] - ybar_train) ** 2).mean()) < 1e-12   # 3: varies on the held-out rows only
    # 4: not finite where only row 1 looks: column 0 and the coefficients stand, column 1 is NaN
    assert np.isfinite(ref["a"][4]) and np.isfinite(ref["b"][4]) and np.isfinite(ref["loss"][4, 0]) and np.isnan(ref["loss"][4, 1])
    assert ref["loss"][4, 0] == ref["loss"][0, 0] and ref["b"][4] == ref["b"][0]
    # 5: not finite where row 0 looks: everything NaN
    assert np.isnan(ref["a"][5]) and np.isnan(ref["b"][5]) and np.isnan(ref["loss"][5]).all()
    # the converse of 4: row 0 sees the infinite prediction
    conv = WS.scaling(P[4:5], y, W[::-1])
    assert np.isnan(conv["a"][0]) and np.isnan(conv["loss"][0]).all()
    # one weighted row in row 0: flat, whatever the predictions
    one = np.zeros(D, np.float32)
    one[3] = 1.5
    r1 = WS.scaling(P[:1], y, np.stack([one, 1 - train]))
    assert r1["b"][0] == 0 and r1["a"][0] == float(y[3]) and r1["loss"][0, 0] == 0 and r1["kappa"][0] == 0
    # one weighted row in a score column: the squared residual of that row
    r2 = WS.scaling(P[:1], y, np.stack([train, one]))
    want = (r2["a"][0] + r2["b"][0] * float(x[3]) - float(y[3])) ** 2
    assert abs(r2["loss"][0, 1] - want) <= 1e-12 + 1e-9 * want
    # a float32 overflow of a coefficient: everything NaN
    tiny = WS.scaling((x * np.float32(1e-30))[None].astype(np.float32) * np.float32(1e-12), y, W)
    assert np.isnan(tiny["a"][0]) and np.isnan(tiny["loss"][0]).all()
    # weight rows that may not be used
    for bad in (np.zeros(D, np.float32), np.where(np.arange(D) == 1, -1.0, train).astype(np.float32),
                np.where(np.arange(D) == 1, np.inf, train).astype(np.float32), np.where(np.arange(D) == 1, np.nan, train).astype(np.float32)):
        first = WS.scaling(P[:2], y, np.stack([bad, 1 - train]))
        assert np.isnan(first["a"]).all() and np.isnan(first["loss"]).all()
        score = WS.scaling(P[:2], y, np.stack([train, bad, 1 - train]))
        base = WS.scaling(P[:2], y, W)
        assert np.isnan(score["loss"][:, 1]).all() and np.array_equal(score["loss"][:, [0, 2]], base["loss"])
        assert np.array_equal(score["a"], base["a"]) and np.array_equal(score["b"], base["b"])


def test_weight_scaling_and_column_independence(rng):
    D = 40
    P, y = _case(rng, 10, D)
    W = _weights(rng, 3, D)
    ref = WS.scaling(P, y, W)
    # a power of two moves no bit (every sum is multiplied exactly); any other factor moves the results by rounding only
    for f in (np.float32(4.0), np.float32(2.0 ** -7)):
        for rows in ([0], [2], [0, 1, 2]):
            Ws = W.copy()
            Ws[rows] *= f
            got = WS.scaling(P, y, Ws)
            for name in ("loss", "a", "b"):
                assert np.array_equal(got[name], ref[name]), (f, rows, name)
    W3 = W.copy()
    W3[0] *= np.float32(3.0)
    W3 = W3.astype(np.float32)
    exact3 = np.array_equal(W3[0].astype(np.float64), W[0].astype(np.float64) * 3.0)   # (a float32 weight times 3 may round)
    got = WS.scaling(P, y, W3)
    if exact3:
        assert np.allclose(got["loss"], ref["loss"], rtol=1e-9, atol=0) and np.allclose(got["b"], ref["b"], rtol=1e-9, atol=0)
    # column k of a K-row call is column 1 of the 2-row call with rows (0, k)
    for k in (1, 2):
        two = WS.scaling(P, y, W[[0, k]])
        assert np.array_equal(two["loss"][:, 1], ref["loss"][:, k]) and np.array_equal(two["loss"][:, 0], ref["loss"][:, 0])
        assert np.array_equal(two["a"], ref["a"]) and np.array_equal(two["b"], ref["b"])


def test_check_against_accepts_itself_and_rejects_a_wrong_value(rng):
    D = 30
    P, y = _case(rng, 8, D)
    W = _weights(rng, 2, D)
    ref = WS.scaling(P, y, W)
    f32 = lambda x: x.astype(np.float32)   # noqa: E731
    assert WS.check_against(ref, f32(ref["loss"]), f32(ref["a"]), f32(ref["b"]), D, what="self") == 0.0
    wrong = f32(ref["loss"]).copy()
    wrong[2, 1] *= np.float32(1.001)
    with pytest.raises(AssertionError):
        WS.check_against(ref, wrong, f32(ref["a"]), f32(ref["b"]), D)
    nan = f32(ref["loss"]).copy()
    nan[1, 0] = np.nan
    with pytest.raises(AssertionError):
        WS.check_against(ref, nan, f32(ref["a"]), f32(ref["b"]), D)
