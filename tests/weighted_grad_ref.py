"""TEST-ONLY: a float64 numpy restatement of the weighted tuning passes (evogp_hip_sr_weighted_gradient and
evogp_hip_sr_weighted_normal_eq, include/evogp_hip.h) on top of the forward semantics and adjoint table of tests/sr_grad_ref.py, the
packing and step of tests/sr_lm_ref.py and the rho of tests/weighted_loss_ref.py.  Single-output trees, one weight row.

    loss[t]    = sum_{d: w_d != 0} w_d rho(r_d) / Wsum           r_d = tree_t(X[d]) - y[d], Wsum = sum_d w_d
    grad[t][i] = sum_d (w_d rho'(r_d) / Wsum) J_i[d]             at CONST nodes, 0 elsewhere;  J_i = d pred / d value[t][i]
    normal[t]  = A_ij = sum_d w_d J_i J_j / Wsum, b_i = sum_d w_d J_i r_d / Wsum  over the first K constants, packed as sr_lm_ref's

``forest_wgrad(value, type, size, X, y, w, kind, param)`` -> ``(loss, grad, gabs)`` and ``forest_wnormal_eq(value, type, size, X, y, w)``
-> ``(loss, normal, nabs)``; gabs / nabs are the same sums over absolute values, the scale of the per-entry tolerance of the GPU tests.
``w`` None: every weight 1.  A row with w_d == 0 is not looked at: the walk runs on the other rows only.  NaN loss and zero rows for a
malformed tree, for a tree whose prediction on a weighted row is not finite in float32, and for every tree when ``w`` holds a negative or
non-finite weight or sums to 0.  ``lm_optimize`` is sr_lm_ref's loop on the weighted normal equations; ``comparable_grad`` and
``comparable_normal`` are the exclusion rule of the GPU tests (tests/test_gpu_sr_grad.py), stated once so that the CPU suite can check
that the reference alone leaves enough trees for the committed seeds."""
import zlib

import numpy as np

import sr_grad_ref as R
import sr_lm_ref as LM
import weighted_loss_ref as WL
from grad_trees import ALL_FUNCS, ARITH, random_forest

KINDS = [("mse", None), ("mae", None), ("huber", 0.5), ("pinball", 0.8), ("logcosh", None)]   # the GPU tests' kinds and parameters


def drho(r, kind, param=None):
    """float64 d rho / d r; 0 at the kinks r == 0 of mae and pinball"""
    r = np.asarray(r, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if kind == "mse":
            return 2.0 * r
        if kind == "mae":
            return np.sign(r)
        if kind == "huber":
            d = float(param)
            return np.where(np.abs(r) <= d, r, d * np.sign(r))
        if kind == "pinball":
            tau = float(param)
            return np.where(r < 0, -tau, np.where(r > 0, 1.0 - tau, 0.0))
        if kind == "logcosh":
            return np.tanh(r)
    raise ValueError(kind)


def tree_adjoints(value, type_, size, X):
    """one single-output tree: ``(pred[D], {i: J_i[D]})`` over EVERY CONST node i of the live prefix, or None for a malformed tree
    (sr_lm_ref.tree_jacobian's walk, which keeps the first K constants only)"""
    L = len(value)
    D, var_len = X.shape
    n = min(max(int(size[0]), 0), L)
    nodes = [R.decode(type_[i], value[i], False, var_len, 1) for i in range(n)]
    h = 0
    for i in reversed(range(n)):
        h += 1 - R.ARITY[nodes[i][0]]
        if h < 1:
            return None
    if n <= 0 or h != 1:
        return None
    X = X.astype(np.float64)
    val, kids = [None] * n, [None] * n
    stack = []
    for i in reversed(range(n)):
        kind, f, _ = nodes[i]
        if kind == "C":
            val[i] = np.full(D, f)
        elif kind == "V":
            val[i] = X[:, f]
        else:
            k = [stack.pop() for _ in range(R.ARITY[kind])]
            kids[i] = k
            ops = [val[j] for j in k]
            if kind == "U":
                val[i] = R.unary(f, ops[0])
            elif kind == "B":
                val[i] = R.binary(f, ops[0], ops[1])
            else:
                val[i] = np.where(ops[0] > 0, ops[1], ops[2])
        stack.append(i)
    adj = [None] * n
    adj[0] = np.ones(D)
    zero = np.zeros(D)
    for i in range(n):
        kind, f, _ = nodes[i]
        if kind in "CV":
            continue
        g, k = adj[i], kids[i]
        ops = [val[j] for j in k]
        with np.errstate(all="ignore"):
            if kind == "U":
                d = [R.unary_adjoint(f, ops[0], val[i], g)]
            elif kind == "B":
                d = list(R.binary_adjoint(f, ops[0], ops[1], val[i], g))
            else:
                take_b = ops[0] > 0
                d = [zero, np.where(take_b, g, 0.0), np.where(take_b, 0.0, g)]
        for j, dj in zip(k, d):
            adj[j] = np.broadcast_to(dj, (D,))
    return val[0], {i: adj[i] for i in range(n) if nodes[i][0] == "C"}


def _rows(X, y, w):
    """the rows that carry weight: ``(X, y, w, Wsum)`` restricted to them, or None for a weight row that may not be used"""
    X, y = np.asarray(X), np.asarray(y, np.float64).reshape(-1)
    w = np.ones(len(y)) if w is None else np.asarray(w, np.float32).astype(np.float64)
    if not np.all(np.isfinite(w)) or np.any(w < 0) or w.sum() == 0:
        return None
    on = w != 0
    return X[on], y[on], w[on], float(w.sum())


def _walk(value, type_, size, X):
    """``tree_adjoints``, or None also when a prediction is not finite in float32"""
    out = tree_adjoints(value, type_, size, X)
    with np.errstate(all="ignore"):
        if out is None or not np.isfinite(out[0].astype(np.float32)).all():
            return None
    return out


def forest_wgrad(value, type_, size, X, y, w, kind, param=None):
    value, type_, size = np.asarray(value), np.asarray(type_), np.asarray(size)
    pop, L = value.shape
    loss, grad, gabs = np.full(pop, np.nan), np.zeros((pop, L)), np.zeros((pop, L))
    rows = _rows(X, y, w)
    if rows is None:
        return loss, grad, gabs
    Xk, yk, wk, wsum = rows
    for t in range(pop):
        out = _walk(value[t], type_[t], size[t], Xk)
        if out is None:
            continue
        pred, J = out
        with np.errstate(all="ignore"):
            r = pred - yk
            loss[t] = np.sum(wk * WL.rho(r, kind, param)) / wsum
            seed = wk * drho(r, kind, param) / wsum
            for i, Ji in J.items():
                grad[t, i] = np.sum(seed * Ji)
                gabs[t, i] = np.sum(np.abs(seed * Ji))
    return loss, grad, gabs


def forest_wnormal_eq(value, type_, size, X, y, w):
    value, type_, size = np.asarray(value), np.asarray(type_), np.asarray(size)
    pop = value.shape[0]
    NT = len(LM.TRI)
    loss, normal, nabs = np.full(pop, np.nan), np.zeros((pop, LM.WORDS)), np.zeros((pop, LM.WORDS))
    rows = _rows(X, y, w)
    if rows is None:
        return loss, normal, nabs
    Xk, yk, wk, wsum = rows
    for t in range(pop):
        out = _walk(value[t], type_[t], size[t], Xk)
        if out is None:
            continue
        pred, J = out
        cidx = LM.optimised_consts(type_[t], size[t])
        with np.errstate(all="ignore"):
            r = pred - yk
            loss[t] = np.sum(wk * r * r) / wsum
            for k, (i, j) in enumerate(LM.TRI):
                if cidx[j] >= 0:
                    term = wk * J[cidx[i]] * J[cidx[j]]
                    normal[t, k], nabs[t, k] = np.sum(term) / wsum, np.sum(np.abs(term)) / wsum
            for i in range(LM.K):
                if cidx[i] >= 0:
                    term = wk * J[cidx[i]] * r
                    normal[t, NT + i], nabs[t, NT + i] = np.sum(term) / wsum, np.sum(np.abs(term)) / wsum
    return loss, normal, nabs


def lm_optimize(value, type_, size, X, y, w, steps, damping=1e-3):
    """sr_lm_ref.lm_optimize on the weighted normal equations: -> (value, loss, accepted[steps][pop])"""
    value = np.array(value, np.float32)
    pop = value.shape[0]

    def neq(v):
        with np.errstate(all="ignore"):
            l, n, _ = forest_wnormal_eq(v, type_, size, X, y, w)
            return l.astype(np.float32), n.astype(np.float32)

    loss, normal = neq(value)
    accepted = np.zeros((steps, pop), bool)
    if steps > 0:
        cand = np.empty_like(value)
        lam = np.full(pop, damping, np.float32)
        LM.lm_step(value, type_, size, cand, loss, normal, loss, normal, lam, 2)
        for k in range(steps):
            loss_c, normal_c = neq(cand)
            accepted[k] = loss_c < loss
            LM.lm_step(value, type_, size, cand, loss, normal, loss_c, normal_c, lam, 3 if k + 1 < steps else 1)
    return value, loss, accepted


# ---- the cases of the GPU comparison and their exclusion rule ---------------------------------------------------------------------
CASES = [(f, L, D) for f in ("arith", "all") for L in (64, 128) for D in (1, 63, 65, 600)]
POP = 24


def make_case(funcs, gp_len, D, pop=POP, var_len=3):
    """24 trees, X uniform on [0.5, 1.5], y on [-1, 1], w = U(0.5, 2) with 30 % of the rows at 0 (at D = 1 the one row keeps its weight)"""
    rng = np.random.default_rng([20261020, zlib.crc32(f"{funcs}-{gp_len}-{D}-{pop}".encode())])
    value, type_, size = random_forest(rng, pop, gp_len, ARITH if funcs == "arith" else ALL_FUNCS, var_len, 1, max_depth=5)
    X = rng.uniform(0.5, 1.5, (D, var_len)).astype(np.float32)
    y = rng.uniform(-1, 1, (D, 1)).astype(np.float32)
    w = rng.uniform(0.5, 2, D).astype(np.float32)
    w[rng.random(D) < 0.3] = 0
    if not w.any():
        w[0] = 1.0
    return value, type_, size, X, y, w


def _comparable(oracle, run, value, type_, size, X, y, w, use_mse):
    """the exclusion rule of test_gradient_matches_float64_reference on the result of ``run(value, X) -> (loss, rows, scale)``: a tree
    is compared when its float64 loss is finite, its fp32 loss is ulp-stable on the rows that carry weight (``oracle``: the fixture,
    or None to leave the probe out) and nudging every constant and input by a relative 2^-22 (two draws of random signs) moves no
    entry by more than 1e-4 of its scale"""
    from helpers import per_tree_tolerance

    with np.errstate(all="ignore"):
        want_loss, want, scale = run(value, X)
        stable = np.isfinite(want_loss)
        if oracle is not None:
            on = w != 0
            Xo, yo = np.ascontiguousarray(X[on]), np.ascontiguousarray(y[on])
            ref, tol, unstable = per_tree_tolerance(oracle, (value, type_, size), Xo, yo, use_mse=use_mse)
            stable &= ~unstable & (tol <= 1e-4 * np.abs(ref) + 1e-6)
        is_c = type_.astype(np.int32) == R.T_CONST
        for k in range(2):
            jr = np.random.default_rng(k)
            vj = np.where(is_c, value * (1 + 2.0 ** -22 * jr.choice([-1, 1], value.shape)), value).astype(np.float32)
            Xj = X.astype(np.float64) * (1 + 2.0 ** -22 * jr.choice([-1, 1], X.shape))
            _, gj, _ = run(vj, Xj)
            moved = np.abs(gj - want) > 1e-4 * scale + 1e-9
            stable &= ~np.any(np.where(np.isfinite(want) & np.isfinite(scale), moved | ~np.isfinite(gj), False), axis=1)
    return want_loss, want, scale, stable


def comparable_grad(oracle, value, type_, size, X, y, w, kind, param):
    """-> (want_loss, want, gabs, stable)"""
    return _comparable(oracle, lambda v, Xv: forest_wgrad(v, type_, size, Xv, y, w, kind, param), value, type_, size, X, y, w,
                       kind != "mae")


def comparable_normal(oracle, value, type_, size, X, y, w):
    """-> (want_loss, want, nabs, stable)"""
    return _comparable(oracle, lambda v, Xv: forest_wnormal_eq(v, type_, size, Xv, y, w), value, type_, size, X, y, w, True)
