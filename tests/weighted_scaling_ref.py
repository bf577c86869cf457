"""TEST-ONLY: linear scaling under sample weights with held-out scoring (csrc/sr_wscale.hip, include/evogp_hip.h
evogp_hip_sr_weighted_scaling) restated in two-pass numpy float64.

``scaling(P, y, W)`` takes the (pop, D) float32 predictions, the labels and the weights -- None (every weight 1), (D,) or (K, D); row 0
is the FIT row, every row is a SCORE row -- and returns a dict of float64 arrays
    loss (pop, K)   a, b (pop,): intercept and slope   kappa (pop,)
and ``V_W`` (K,) = V_k / W_k.  With W_k = sum_d W[k, d], ybar0 = sum_d W[0, d] y_d / W_0, v = y - ybar0 and, per row k over the data rows
with W[k, d] != 0, m_k the weighted mean of p, M_k = sum w (p - m_k)^2, vbar_k = sum w v / W_k, c_k = sum w (p - m_k)(v - vbar_k),
V_k = sum w (v - vbar_k)^2:
    flat (min p == max p over the rows row 0 weights, or M_0 <= 0, or one such row):   b = 0, a = ybar0 + vbar_0
    otherwise:                                                                         b = c_0 / M_0, a = ybar0 + vbar_0 - b m_0
    delta_k = b (m_k - m_0) - (vbar_k - vbar_0);   loss_k = max(0, b^2 M_k - 2 b c_k + V_k + W_k delta_k^2) / W_k
    a non-finite prediction on a row column k weights: loss_k NaN; if k = 0: everything NaN.  a or b not finite as float32: everything NaN
    a weight row with a negative or non-finite weight or a sum of 0: NaN for every tree -- everywhere if it is row 0, in column k otherwise
``kappa`` is the largest p^2 over the data rows weighted in ANY column, divided by M_0 / W_0 (0 for a flat tree, NaN for a NaN tree):
it bounds the cancellation of the uncentred sums and of the pilot-shifted ones alike.

``tolerance`` and ``check_against`` follow tests/linear_scaling_ref.py, where the derivation is: rtol = 1e-6 + kappa D 2^-52, and for the
loss atol = 1e-6 V_k / W_k (the loss is a difference of terms of that size)."""
import numpy as np


def _rows(W, D):
    if W is None:
        return np.ones((1, D), np.float64)
    W = np.asarray(W, np.float32).reshape(-1, D)
    return W.astype(np.float64)


def scaling(P, y, W=None):
    P = np.asarray(P, np.float32)
    pop, D = P.shape
    y64 = np.asarray(y, np.float64).reshape(-1)
    assert y64.shape == (D,)
    Wd = _rows(W, D)
    K = Wd.shape[0]
    on = Wd != 0
    with np.errstate(invalid="ignore", over="ignore"):
        wsum = Wd.sum(axis=1)
    usable = np.array([bool(np.isfinite(Wd[k]).all() and (Wd[k] >= 0).all() and wsum[k] != 0) for k in range(K)])
    out = {"loss": np.full((pop, K), np.nan), "a": np.full(pop, np.nan), "b": np.full(pop, np.nan), "kappa": np.full(pop, np.nan),
           "V_W": np.full(K, np.nan), "usable": usable}
    if not usable[0]:
        return out
    w0, i0 = Wd[0][on[0]], on[0]
    ybar0 = (w0 * y64[i0]).sum() / wsum[0]
    v = y64 - ybar0
    vbar, V = np.full(K, np.nan), np.full(K, np.nan)
    for k in np.flatnonzero(usable):
        wk, vk = Wd[k][on[k]], v[on[k]]
        vbar[k] = (wk * vk).sum() / wsum[k]
        V[k] = (wk * (vk - vbar[k]) ** 2).sum()
    out["V_W"] = V / wsum
    any_on = on[usable].any(axis=0)
    for t in range(pop):
        p = P[t]
        p0 = p[i0]
        if not np.isfinite(p0).all():
            continue
        p64 = p.astype(np.float64)
        m0 = (w0 * p64[i0]).sum() / wsum[0]
        M0 = (w0 * (p64[i0] - m0) ** 2).sum()
        c0 = (w0 * (p64[i0] - m0) * (v[i0] - vbar[0])).sum()
        flat = p0.min() == p0.max() or M0 <= 0 or p0.size == 1
        b = 0.0 if flat else c0 / M0
        a = ybar0 + vbar[0] - (0.0 if flat else b * m0)
        with np.errstate(over="ignore"):
            if not (np.isfinite(np.float32(a)) and np.isfinite(np.float32(b))):
                continue
        out["a"][t], out["b"][t] = a, b
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            out["kappa"][t] = 0.0 if flat else np.max(p64[any_on] ** 2) / (M0 / wsum[0])
        for k in np.flatnonzero(usable):
            wk, pk, vk = Wd[k][on[k]], p64[on[k]], v[on[k]]
            if not np.isfinite(p[on[k]]).all():
                continue
            mk = (wk * pk).sum() / wsum[k]
            Mk = (wk * (pk - mk) ** 2).sum()
            ck = (wk * (pk - mk) * (vk - vbar[k])).sum()
            delta = b * (mk - m0) - (vbar[k] - vbar[0])
            num = b * b * Mk - 2.0 * b * ck + V[k] + wsum[k] * delta * delta
            out["loss"][t, k] = (0.0 if num < 0 else num) / wsum[k]
    return out


def direct_loss(P, y, W, a, b):
    """(pop, K): sum_d W[k, d] (a + b p_d - y_d)^2 / W_k over the rows with weight, straight from the definition"""
    P64 = np.asarray(P, np.float32).astype(np.float64)
    pop, D = P64.shape
    y64 = np.asarray(y, np.float64).reshape(-1)
    Wd = _rows(W, D)
    out = np.full((pop, Wd.shape[0]), np.nan)
    for k in range(Wd.shape[0]):
        i = Wd[k] != 0
        with np.errstate(invalid="ignore", over="ignore"):
            r = a[:, None] + b[:, None] * P64[:, i] - y64[None, i]
            out[:, k] = (Wd[k][None, i] * r * r).sum(axis=1) / Wd[k].sum()
    return out


def tolerance(kappa, D, V_W):
    kap = np.where(np.isfinite(kappa), kappa, 0.0)   # (rows without a finite kappa are not compared)
    return 1e-6 + kap * D * 2.0 ** -52, 1e-6 * np.asarray(V_W, np.float64)


def check_against(ref, loss, a, b, D, kappa_limit=1e8, what=""):
    """assert the device's (loss (pop, K), a, b) against ``scaling``'s result: equal NaN masks, every finite entry of a tree with
    kappa < kappa_limit within its tolerance; returns the share of finite trees left out for their kappa"""
    loss, a, b = (np.asarray(x, np.float64) for x in (loss, a, b))
    loss = loss.reshape(len(a), -1)
    assert loss.shape == ref["loss"].shape, (what, loss.shape, ref["loss"].shape)
    nan_tree = np.isnan(ref["a"])
    for got in (a, b):
        assert np.array_equal(np.isnan(got), nan_tree), (what, np.flatnonzero(np.isnan(got) != nan_tree)[:8])
    nan_loss = np.isnan(ref["loss"])
    assert np.array_equal(np.isnan(loss), nan_loss), (what, np.argwhere(np.isnan(loss) != nan_loss)[:8])
    finite = ~nan_tree
    with np.errstate(invalid="ignore"):
        cmp = finite & (ref["kappa"] < kappa_limit)
    rtol, atol_loss = tolerance(ref["kappa"], D, ref["V_W"])
    worst = 0.0

    def one(name, got, want, atol, mask):
        nonlocal worst
        with np.errstate(invalid="ignore"):
            off = np.abs(got - want)
            tol = rtol * np.abs(want) + atol
        bad = np.flatnonzero(mask & ~(off <= tol))
        assert bad.size == 0, (what, name, bad[:5], got[bad[:5]], want[bad[:5]], tol[bad[:5]], ref["kappa"][bad[:5]])
        if mask.any():
            with np.errstate(invalid="ignore", divide="ignore"):
                q = off[mask] / tol[mask]
            worst = max(worst, float(np.nanmax(np.where(tol[mask] > 0, q, 0.0))))

    one("a", a, ref["a"], 0.0, cmp)
    one("b", b, ref["b"], 0.0, cmp)
    for k in range(loss.shape[1]):
        one(f"loss[{k}]", loss[:, k], ref["loss"][:, k], atol_loss[k], cmp & ~nan_loss[:, k])
    excluded = float((finite & ~cmp).sum()) / max(int(finite.sum()), 1)
    print(f"{what}: {int(cmp.sum())} of {int(finite.sum())} finite trees compared ({excluded:.1%} left out for kappa >= {kappa_limit:g}), "
          f"{int(nan_tree.sum())} NaN trees, {int(nan_loss.sum())} NaN entries, worst |got-want|/tol {worst:.3g}")
    return excluded
