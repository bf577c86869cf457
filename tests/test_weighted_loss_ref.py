"""CPU: the numpy restatement of the weighted losses (tests/weighted_loss_ref.py) against values computed by hand and against the
identities that tie the five kinds together."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import weighted_loss_ref as WL  # noqa: E402

# three trees on four rows; residuals r = P - y
Y = np.array([1.0, 2.0, 0.0, -1.0], np.float32)
P = np.array([[1.5, 1.0, 0.25, -1.0],      # r =  0.5, -1, 0.25, 0
              [4.0, 2.0, -3.0, -1.0],      # r =  3, 0, -3, 0
              [1.0, 2.0, 0.0, 1.0]],       # r =  0, 0, 0, 2
             np.float32)
W = np.array([[1.0, 1.0, 1.0, 1.0], [2.0, 0.0, 1.0, 1.0]], np.float32)


def _f32(x):
    return np.float32(x)


def test_hand_computed_values_of_every_kind():
    # tree 0, weights 1: r = .5, -1, .25, 0
    got = WL.weighted_loss(P, Y, W, "mse")
    assert got.dtype == np.float32 and got.shape == (3, 2)
    assert got[0, 0] == _f32((0.25 + 1 + 0.0625 + 0) / 4) and got[0, 1] == _f32((2 * 0.25 + 0.0625 + 0) / 4)
    assert got[1, 0] == _f32(18 / 4) and got[1, 1] == _f32((2 * 9 + 9) / 4) and got[2, 0] == _f32(1.0) and got[2, 1] == _f32(1.0)
    got = WL.weighted_loss(P, Y, W, "mae")
    assert got[0, 0] == _f32(1.75 / 4) and got[0, 1] == _f32((1 + 0.25) / 4) and got[1, 1] == _f32(9 / 4)
    # huber, delta 0.5: |r| <= .5 -> r^2 / 2, else .5 (|r| - .25)
    got = WL.weighted_loss(P, Y, W, "huber", 0.5)
    assert got[0, 0] == _f32((0.125 + 0.375 + 0.03125 + 0) / 4) and got[1, 0] == _f32((1.375 + 1.375) / 4)
    assert got[0, 1] == _f32((2 * 0.125 + 0.03125) / 4)
    # pinball, tau 0.25: r_y = y - p = -r; r_y >= 0 -> .25 r_y, else -.75 r_y
    got = WL.weighted_loss(P, Y, W, "pinball", 0.25)
    assert got[0, 0] == _f32((0.75 * 0.5 + 0.25 * 1 + 0.75 * 0.25 + 0) / 4)
    assert got[1, 0] == _f32((0.75 * 3 + 0.25 * 3) / 4) and got[2, 1] == _f32(0.75 * 2 / 4)
    # log cosh
    got = WL.weighted_loss(P, Y, None, "logcosh")
    assert got.shape == (3, 1)
    want = [sum(math.log(math.cosh(r)) for r in row) / 4 for row in ([0.5, -1, 0.25, 0], [3, 0, -3, 0], [0, 0, 0, 2])]
    assert np.allclose(got[:, 0], want, rtol=1e-6, atol=0)
    assert WL.rho(1e6, "logcosh") == 1e6 - math.log(2) and WL.rho(0.0, "logcosh") == 0.0   # no overflow; log cosh 0
    # a (D,) weight vector is one row, None is a row of ones
    assert np.array_equal(WL.weighted_loss(P, Y, W[1], "mae"), WL.weighted_loss(P, Y, W[1:], "mae"))
    assert np.array_equal(WL.weighted_loss(P, Y, None, "mae"), WL.weighted_loss(P, Y[:, None], W[:1], "mae"))


def test_identities_between_the_kinds(rng):
    Pr = rng.normal(0, 2, (50, 200)).astype(np.float32)
    y = rng.normal(0, 1, 200).astype(np.float32)
    Wr = rng.uniform(0, 2, (3, 200)).astype(np.float32)
    Wr[rng.random((3, 200)) < 1 / 3] = 0
    mse, mae = (WL.weighted_loss(Pr, y, Wr, k).astype(np.float64) for k in ("mse", "mae"))
    big = float(np.abs(Pr.astype(np.float64) - y).max()) * 2
    small = float(np.abs(Pr.astype(np.float64) - y).min()) / 2
    assert small > 0
    # every |r| <= delta: mse / 2;  every |r| > delta: delta (mae - delta / 2)
    assert np.allclose(WL.weighted_loss(Pr, y, Wr, "huber", big), mse / 2, rtol=3e-7, atol=0)
    assert np.allclose(WL.weighted_loss(Pr, y, Wr, "huber", small), small * (mae - small / 2), rtol=3e-7, atol=0)
    assert np.allclose(WL.weighted_loss(Pr, y, Wr, "pinball", 0.5), mae / 2, rtol=3e-7, atol=0)
    # pinball puts the weight on the side tau says: under-prediction (y > p) costs tau, over-prediction 1 - tau
    lo, hi = WL.weighted_loss(Pr, y, Wr, "pinball", 0.1), WL.weighted_loss(Pr, y, Wr, "pinball", 0.9)
    assert np.allclose(lo.astype(np.float64) + hi, mae, rtol=3e-7, atol=0)
    # log cosh lies between the Huber bounds: huber_1(r) - (1 - log 2)... precisely  |r| - log 2 <= log cosh r <= min(r^2 / 2, |r|)
    lc = WL.weighted_loss(Pr, y, Wr, "logcosh").astype(np.float64)
    h1 = WL.weighted_loss(Pr, y, Wr, "huber", 1.0).astype(np.float64)
    assert np.all(lc <= h1 * (1 + 1e-6)) and np.all(lc <= mse / 2 * (1 + 1e-6)) and np.all(lc <= mae * (1 + 1e-6))
    assert np.all(lc >= (mae - math.log(2)) * (1 - 1e-6)) and np.all(lc >= h1 * (1 - 1e-6) - (math.log(2) - 0.5)) and np.all(lc >= 0)


def test_zero_weight_rule_and_unusable_weight_rows():
    Pn = P.copy()
    Pn[0, 1] = np.nan      # tree 0 is undefined on row 1, which column 1 gives no weight
    Pn[1, 1] = np.inf
    Pn[2, 0] = -np.inf     # row 0 has weight in both columns
    got = WL.weighted_loss(Pn, Y, W, "mse")
    clean = WL.weighted_loss(P, Y, W, "mse")
    assert np.isnan(got[0, 0]) and got[0, 1] == clean[0, 1]
    assert np.isnan(got[1, 0]) and got[1, 1] == clean[1, 1]
    assert np.isnan(got[2, 0]) and np.isnan(got[2, 1])
    # (what case_errors @ W gives instead: 0 * NaN)
    with np.errstate(invalid="ignore"):
        assert np.isnan(((Pn[0].astype(np.float64) - Y) ** 2 * W[1]).sum())
    # a negative weight, a NaN weight, an infinite weight, a row of zeros: NaN for every tree, the other columns untouched
    for poison in (-1.0, np.nan, np.inf, None):
        Wb = np.stack([W[0], W[1], W[1]])
        if poison is None:
            Wb[1] = 0
        else:
            Wb[1, 2] = poison
        got = WL.weighted_loss(P, Y, Wb, "mae")
        want = WL.weighted_loss(P, Y, W, "mae")
        assert np.isnan(got[:, 1]).all() and np.array_equal(got[:, 0], want[:, 0]) and np.array_equal(got[:, 2], want[:, 1])
    # the mean may overflow float32: +inf, not NaN
    huge = np.full((1, 4), 3e38, np.float32)
    with np.errstate(over="ignore"):
        assert WL.weighted_loss(huge, -huge[0], None, "mse")[0, 0] == np.inf


def test_tolerance_terms():
    assert WL.tolerance(1) == 2.0 ** -23 + 2.0 ** -52
    assert WL.tolerance(4096, "huber") == 2.0 ** -23 + 2.0 ** -40
    assert WL.tolerance(4096, "logcosh") == 2.0 ** -23 + 2.0 ** -39
    with pytest.raises(ValueError):
        WL.rho(1.0, "cauchy")
