"""The numpy float64 restatement of evogp_hip_sr_weighted_loss (include/evogp_hip.h; evogp_amd/csrc/sr_wloss.hip), on given predictions.

    loss[t, k] = ( sum_d W[k, d] * rho(P[t, d] - y[d]) ) / sum_d W[k, d]        r = float64(P) - float64(y), rho in float64

    a row with W[k, d] == 0 is not looked at in column k;  a column is NaN where a row WITH weight has a non-finite prediction (a
    malformed tree is a row of NaN predictions here), and for every tree where W[k] holds a negative or non-finite weight or sums to 0;
    the result is float32(S / Wsum).

``tolerance(D, kind)`` -- derived, not measured.  Device and restatement evaluate the same float64 expression on the same float32
predictions and differ in three things only:
  * the output is rounded to float32 once: a relative 2^-24, and 2^-23 covers the case where the two float64 quotients fall on either
    side of a rounding boundary;
  * the float64 sum of D terms is taken in another order.  Every term W * rho is >= 0, so nothing cancels: any order of summation is
    within (D - 1) 2^-53 of the exact sum relative to the sum itself (Higham, Accuracy and Stability, eq. 4.4, with sum |x_i| = |sum
    x_i|), hence two orders within D 2^-52 of each other, the same bound on Wsum included since the weights are >= 0 too;
  * log-cosh calls the float64 exp and log1p of two libraries: a few units of 2^-53 on terms of size log 2 + |r|, against a term
    that is rho itself; 2^-40 is 8192 such units and holds while the weighted mean of rho is above ~1e-12 of log 2 + |r|, which every
    tree that is not an exact fit satisfies.  The other four kinds are sums and products that round identically.
"""
import numpy as np

KINDS = {"mse": 0, "mae": 1, "huber": 2, "pinball": 3, "logcosh": 4}
T_CONST = 1


def rho(r, kind, param=None):
    """float64 rho(r) for r = p - y"""
    r = np.asarray(r, np.float64)
    a = np.abs(r)
    with np.errstate(invalid="ignore", over="ignore"):
        if kind == "mse":
            return r * r
        if kind == "mae":
            return a
        if kind == "huber":
            d = float(param)
            return np.where(a <= d, r * r * 0.5, d * (a - d * 0.5))
        if kind == "pinball":
            tau, ry = float(param), -r
            return np.where(ry >= 0, tau * ry, (tau - 1.0) * ry)
        if kind == "logcosh":
            return a + np.log1p(np.exp(-2.0 * a)) - np.log(2.0)
    raise ValueError(kind)


def weighted_loss(P, y, W, kind, param=None):
    """(pop, K) float32 from predictions ``P`` (pop, D) float32, labels ``y`` (D,) or (D, 1), weights ``W`` (K, D), (D,) or None"""
    P = np.asarray(P, np.float32)
    y = np.asarray(y, np.float32).reshape(-1)
    pop, D = P.shape
    W = np.ones((1, D), np.float32) if W is None else np.asarray(W, np.float32).reshape(-1, D)
    rr = rho(P.astype(np.float64) - y.astype(np.float64)[None, :], kind, param)
    out = np.full((pop, W.shape[0]), np.nan, np.float32)
    for k in range(W.shape[0]):
        w = W[k].astype(np.float64)
        if not np.all(np.isfinite(w)) or np.any(w < 0) or w.sum() == 0:
            continue
        on = w != 0
        bad = ~np.isfinite(P[:, on]).all(axis=1)
        with np.errstate(invalid="ignore", over="ignore"):
            s = (rr[:, on] * w[on][None, :]).sum(axis=1)
            out[:, k] = np.where(bad, np.nan, s / w.sum()).astype(np.float32)
    return out


def tolerance(D, kind="mse"):
    """the relative tolerance between the device and ``weighted_loss`` on the same predictions (the module docstring derives it)"""
    return 2.0 ** -23 + D * 2.0 ** -52 + (2.0 ** -40 if kind == "logcosh" else 0.0)


def check(got, want, D, kind, what=""):
    """equal NaN masks and EVERY finite entry within ``tolerance``; returns the worst error in units of the tolerance"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, np.flatnonzero(np.isnan(got) != np.isnan(want))[:8])
    ok = ~np.isnan(want)
    g, w = got[ok].astype(np.float64), want[ok].astype(np.float64)
    same = g == w   # (+inf against +inf)
    with np.errstate(invalid="ignore"):
        off = np.where(same, 0.0, np.abs(g - w))
    tol = tolerance(D, kind) * np.abs(w)
    worst = np.flatnonzero(~(off <= tol))
    assert worst.size == 0, (what, kind, worst[:5], g[worst[:5]], w[worst[:5]])
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.max(np.where(same, 0.0, off / tol), initial=0.0))
