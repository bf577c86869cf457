"""TEST-ONLY: linear scaling (csrc/sr_scale.hip, include/evogp_hip.h evogp_hip_sr_linear_scaling / evogp_hip_wrap_linear) restated in
numpy float64.

``scaling(P, y)`` takes the (pop, D) float32 predictions and the labels and returns a dict of (pop,) float64 arrays
    loss, a (intercept), b (slope)   NaN for a row with a non-finite prediction (a malformed tree's predictions are NaN)
    kappa                            the condition number (Spp/D) / var of the closed form (0 for a tree whose predictions are one value:
                                     nothing cancels; inf where only the rounding of the sums made var <= 0)
and the scalars ybar, syy_D.  With ybar the float64 mean of the labels, v = y - ybar, Syy = sum v^2, Sp = sum p, Spp = sum p^2,
Spv = sum p v, var = Spp/D - (Sp/D)^2, cov = Spv/D:
    min p == max p, or var <= 0, or D == 1:   b = 0, a = ybar, loss = Syy/D
    otherwise:                                b = cov/var, a = ybar - b Sp/D, loss = max(0, Syy/D - b cov)
    a or b not finite as float32:             all three NaN

``tolerance(kappa, D, syy_D)`` -> ``(rtol, atol_loss)``: rtol = 1e-6 + kappa D 2^-52 (the float32 rounding of the output, plus the
order of the float64 sums amplified by the cancellation in var), atol_loss = 1e-6 Syy/D for the loss only (it is itself a difference
of two terms of the size of Syy/D).

``wrap_rows`` restates the rewrite T -> ADD(MUL(T, slope), intercept); ``refit_bound`` bounds |MSE(wrapped tree) - scaled loss|."""
import numpy as np

from subtree_ref import live_len, well_formed

F_ADD, F_MUL, T_CONST, T_BFUNC = 1, 3, 1, 3


def scaling(P, y):
    P = np.asarray(P, np.float32)
    pop, D = P.shape
    y64 = np.asarray(y, np.float64).reshape(-1)
    assert y64.shape == (D,)
    ybar = y64.mean()
    v = y64 - ybar
    syy_D = float((v * v).sum() / D)
    out = {k: np.full(pop, np.nan) for k in ("loss", "a", "b", "kappa")}
    for t in range(pop):
        p = P[t]
        if not np.isfinite(p).all():
            continue
        p64 = p.astype(np.float64)
        mean = p64.sum() / D
        msq = (p64 * p64).sum() / D
        var = msq - mean * mean
        cov = (p64 * v).sum() / D
        if p.min() == p.max() or var <= 0 or D == 1:
            # decided exactly on the predictions: nothing cancels, kappa 0; a var <= 0 that only the rounding of the sums produced: inf
            a, b, loss, kappa = ybar, 0.0, syy_D, (0.0 if p.min() == p.max() else np.inf)
        else:
            b = cov / var
            a = ybar - b * mean
            loss = max(0.0, syy_D - b * cov)
            kappa = msq / var
        with np.errstate(over="ignore"):
            if not (np.isfinite(np.float32(a)) and np.isfinite(np.float32(b))):
                continue
        out["loss"][t], out["a"][t], out["b"][t], out["kappa"][t] = loss, a, b, kappa
    out["ybar"], out["syy_D"] = float(ybar), syy_D
    return out


def tolerance(kappa, D, syy_D):
    kap = np.where(np.isfinite(kappa), kappa, 0.0)   # (rows without a finite kappa are not compared)
    return 1e-6 + kap * D * 2.0 ** -52, 1e-6 * syy_D


def check_against(ref, loss, a, b, D, kappa_limit=1e8, what=""):
    """assert the device's (loss, a, b) against ``scaling``'s result: equal NaN masks, every finite row with kappa < kappa_limit within
    its tolerance; returns the share of finite rows left out for their kappa"""
    loss, a, b = (np.asarray(x, np.float64) for x in (loss, a, b))
    nan_ref = np.isnan(ref["loss"])
    for got in (loss, a, b):
        assert np.array_equal(np.isnan(got), nan_ref), (what, np.flatnonzero(np.isnan(got) != nan_ref)[:8])
    finite = ~nan_ref
    with np.errstate(invalid="ignore"):
        cmp = finite & (ref["kappa"] < kappa_limit)
    rtol, atol_loss = tolerance(ref["kappa"], D, ref["syy_D"])
    worst = 0.0
    for name, got, atol in (("loss", loss, atol_loss), ("a", a, 0.0), ("b", b, 0.0)):
        want = ref[name]
        with np.errstate(invalid="ignore"):
            off = np.abs(got - want)
            tol = rtol * np.abs(want) + atol
        bad = np.flatnonzero(cmp & ~(off <= tol))
        assert bad.size == 0, (what, name, bad[:5], got[bad[:5]], want[bad[:5]], tol[bad[:5]], ref["kappa"][bad[:5]])
        if cmp.any():
            with np.errstate(invalid="ignore", divide="ignore"):
                q = off[cmp] / tol[cmp]
            worst = max(worst, float(np.nanmax(np.where(tol[cmp] > 0, q, 0.0))))
    excluded = float((finite & ~cmp).sum()) / max(int(finite.sum()), 1)
    print(f"{what}: {int(cmp.sum())} of {int(finite.sum())} finite rows compared ({excluded:.1%} left out for kappa >= {kappa_limit:g}), "
          f"{int(nan_ref.sum())} NaN rows, worst |got-want|/tol {worst:.3g}")
    return excluded


def wrap_rows(value, type_, size, coef, out_len):
    """-> (value, type, size, applied): the rule of evogp_hip_wrap_linear; coef is (pop, 2) = intercept, slope"""
    value, type_, size = np.asarray(value, np.float32), np.asarray(type_, np.int16), np.asarray(size, np.int16)
    coef = np.asarray(coef, np.float32)
    pop, L = value.shape
    assert out_len >= L
    ov, ot, os_ = np.zeros((pop, out_len), np.float32), np.zeros((pop, out_len), np.int16), np.zeros((pop, out_len), np.int16)
    applied = np.zeros(pop, np.uint8)
    for t in range(pop):
        n = live_len(size[t], L)
        a, b = coef[t]
        if well_formed(type_[t], n) and np.isfinite(a) and np.isfinite(b) and n + 4 <= out_len:
            ov[t, 0], ot[t, 0], os_[t, 0] = F_ADD, T_BFUNC, n + 4
            ov[t, 1], ot[t, 1], os_[t, 1] = F_MUL, T_BFUNC, n + 2
            ov[t, 2:n + 2], ot[t, 2:n + 2], os_[t, 2:n + 2] = value[t, :n], type_[t, :n], size[t, :n]
            ov[t, n + 2], ot[t, n + 2], os_[t, n + 2] = b, T_CONST, 1
            ov[t, n + 3], ot[t, n + 3], os_[t, n + 3] = a, T_CONST, 1
            applied[t] = 1
        else:
            ov[t, :L], ot[t, :L], os_[t, :L] = value[t], type_[t], size[t]
    return ov, ot, os_, applied


def refit_bound(P, a, b, loss):
    """per tree: how far the plain MSE of the wrapped tree, which computes fl(fl(p b) + a) in float32, may lie from the scaled loss.
    Every prediction moves by at most delta = 2^-22 max_d(|b p_d| + |a|) (two roundings of relative size 2^-24 each on values of at
    most that size, and the coefficients' own float32 rounding, 2^-24 each), so a root mean square of residuals r changes by at most
    delta and its square by 2 r delta + delta^2."""
    P = np.asarray(P, np.float64)
    a, b, loss = (np.asarray(x, np.float64) for x in (a, b, loss))
    with np.errstate(invalid="ignore"):
        delta = 2.0 ** -22 * np.max(np.abs(b[:, None] * P) + np.abs(a)[:, None], axis=1)
        return 2.0 * np.sqrt(loss) * delta + delta * delta
