"""TEST-ONLY: a float64 numpy restatement of the Levenberg-Marquardt constant optimiser (csrc/sr_lm.hip) on top of the forward
semantics and adjoint table of tests/sr_grad_ref.py.  Single-output trees, MSE.

``tree_jacobian(value, type, size, X)`` -> ``(pred[D], J[D][K], cidx[K])``: the prediction, its derivative in the tree's OPTIMISED
constants (the first min(nc, K) CONST nodes of the live prefix in prefix order; absent ones have a zero column and index -1), or
``None`` for a malformed tree.
``forest_normal_eq(value, type, size, X, y)`` -> ``(loss, normal, nabs)``: loss[t] = mean r^2, normal[t] = the 36 upper-triangle
entries of A = J^T J / D row-major then the 8 entries of b = J^T r / D (r = pred - y), nabs[t] the same sums over absolute values
(the scale of the per-entry tolerance of the GPU tests).  Malformed trees: NaN loss, zero rows.
``lm_step(...)`` restates evogp_hip_sr_lm_step on numpy arrays in place; ``lm_optimize`` is the whole loop."""
import numpy as np

import sr_grad_ref as R

K = 8
TRI = [(i, j) for i in range(K) for j in range(i, K)]   # the packed order of A's upper triangle
WORDS = len(TRI) + K
DAMP_MIN, DAMP_MAX = np.float32(1e-10), np.float32(1e10)


def optimised_consts(type_, size):
    """node indices of the first K CONST nodes of the live prefix of one single-output row, padded with -1"""
    L = len(type_)
    n = min(max(int(size[0]), 0), L)
    idx = [i for i in range(n) if int(type_[i]) == R.T_CONST][:K]
    return np.array(idx + [-1] * (K - len(idx)), np.int64)


def tree_jacobian(value, type_, size, X):
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
    cidx = optimised_consts(type_, size)
    J = np.zeros((D, K))
    for j, c in enumerate(cidx):
        if c >= 0:
            J[:, j] = adj[c]
    return val[0], J, cidx


def tree_normal_eq(value, type_, size, X, y):
    """one tree: (loss, normal[44], nabs[44]) in float64"""
    out = tree_jacobian(value, type_, size, X)
    if out is None:
        return np.nan, np.zeros(WORDS), np.zeros(WORDS)
    pred, J, cidx = out
    D = X.shape[0]
    with np.errstate(all="ignore"):
        r = pred - y.astype(np.float64).reshape(-1)
        loss = float(np.sum(r * r) / D)
        normal, nabs = np.zeros(WORDS), np.zeros(WORDS)
        for k, (i, j) in enumerate(TRI):
            if cidx[j] >= 0:
                normal[k] = np.sum(J[:, i] * J[:, j]) / D
                nabs[k] = np.sum(np.abs(J[:, i] * J[:, j])) / D
        for i in range(K):
            if cidx[i] >= 0:
                normal[len(TRI) + i] = np.sum(J[:, i] * r) / D
                nabs[len(TRI) + i] = np.sum(np.abs(J[:, i] * r)) / D
    return loss, normal, nabs


def forest_normal_eq(value, type_, size, X, y):
    value, type_, size, X, y = (np.asarray(a) for a in (value, type_, size, X, y))
    pop = value.shape[0]
    loss, normal, nabs = np.zeros(pop), np.zeros((pop, WORDS)), np.zeros((pop, WORDS))
    for t in range(pop):
        loss[t], normal[t], nabs[t] = tree_normal_eq(value[t], type_[t], size[t], X, y)
    return loss, normal, nabs


def unpack(normal_row):
    """(A[K][K] symmetric, b[K]) of one packed row"""
    A = np.zeros((K, K))
    for k, (i, j) in enumerate(TRI):
        A[i, j] = A[j, i] = normal_row[k]
    return A, np.asarray(normal_row[len(TRI):], np.float64)


def solve_step(normal_row, lam, loss, consts):
    """the proposal of one tree: the new float32 values of its optimised constants (``consts``: their current values, one per present
    constant), or None when the tree does not move"""
    nc = len(consts)
    A, b = unpack(np.asarray(normal_row, np.float64))
    with np.errstate(all="ignore"):
        if not np.isfinite(loss) or loss == 0:
            return None
        act = [i for i in range(nc) if A[i, i] != 0]   # (a NaN diagonal is "active" and stops the tree below)
        if not act:
            return None
        As, bs = A[np.ix_(act, act)], b[act]
        if not (np.isfinite(As).all() and np.isfinite(bs).all()):
            return None
        M = As + float(lam) * np.diag(np.diag(As))
        try:
            U = np.linalg.cholesky(M)
        except np.linalg.LinAlgError:
            return None
        if not np.isfinite(U).all() or (np.diag(U) <= 0).any():
            return None
        z = np.linalg.solve(U, -bs)
        delta = np.linalg.solve(U.T, z)
        new = np.array(consts, np.float32)
        new[act] = (np.asarray(consts, np.float64)[act] + delta).astype(np.float32)
        if not np.isfinite(new[act]).all():
            return None
    return new


def lm_step(value, type_, size, cand, loss, normal, loss_cand, normal_cand, damping, phase):
    """float32-state restatement of evogp_hip_sr_lm_step on numpy arrays, in place (the test-only CPU kernel of tree_SR_lm_step)"""
    pop = value.shape[0]
    for t in range(pop):
        cidx = optimised_consts(type_[t], size[t])
        cidx = cidx[cidx >= 0]
        if phase & 1:
            if loss_cand[t] < loss[t]:
                value[t, cidx] = cand[t, cidx]
                normal[t] = normal_cand[t]
                loss[t] = loss_cand[t]
                damping[t] = max(np.float32(damping[t]) / np.float32(10), DAMP_MIN)
            else:
                damping[t] = min(np.float32(10) * np.float32(damping[t]), DAMP_MAX)
        if phase & 2:
            cand[t] = value[t]
            new = solve_step(normal[t], damping[t], loss[t], value[t, cidx])
            if new is not None:
                cand[t, cidx] = new


def lm_optimize(value, type_, size, X, y, steps, damping=1e-3):
    """the whole loop of Forest.optimize_constants(method="lm") with the float64 normal equations rounded to float32 state:
    -> (value, loss, accepted[steps][pop])"""
    value = np.array(value, np.float32)
    pop = value.shape[0]

    def neq(v):
        with np.errstate(all="ignore"):
            l, n, _ = forest_normal_eq(v, type_, size, X, y)
            return l.astype(np.float32), n.astype(np.float32)

    loss, normal = neq(value)
    accepted = np.zeros((steps, pop), bool)
    if steps > 0:
        cand = np.empty_like(value)
        lam = np.full(pop, damping, np.float32)
        lm_step(value, type_, size, cand, loss, normal, loss, normal, lam, 2)
        for k in range(steps):
            loss_c, normal_c = neq(cand)
            accepted[k] = loss_c < loss
            lm_step(value, type_, size, cand, loss, normal, loss_c, normal_c, lam, 3 if k + 1 < steps else 1)
    return value, loss, accepted
