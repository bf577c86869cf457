"""TEST-ONLY: the simulation sensitivities (include/evogp_hip.h, evogp_hip_sr_simulation_sensitivities) restated in numpy: a dual-number
evaluator over the forest arrays, one numpy operation per rounding, under tests/simulate_ref.py's step formulas applied to value and tangent
alike.  float32 is the definition the kernel is held to bit for bit; float64 is the same code, the truth for finite differences.  Node
values and the adjoint table are tests/sr_grad_ref.py's.  ``lm_tune``: evogp_hip_sr_lm_step's rule driven by this restatement."""
import numpy as np

import sr_grad_ref as R

F = np.float32
K = 8


def program(value, type_, size, t, multi, var_len, out_len, override=None):
    """tree t as ``[(kind, payload, out, slot)]`` in execution (reverse prefix) order, slot = which optimised constant a CONST node is
    (-1: none), and the number of optimised constants; ``(None, 0)`` for a malformed tree"""
    n = min(max(int(size[t, 0]), 0), value.shape[1])
    slots = {i: k for k, i in enumerate([i for i in range(n) if type_[t, i] == R.T_CONST][:K])}
    prog, h = [], 0
    for i in range(n - 1, -1, -1):
        kind, pay, out = R.decode(type_[t, i], value[t, i], multi, var_len, out_len)
        h += 1 - R.ARITY[kind]
        if h < 1:
            return None, 0
        prog.append((kind, override.get(i, pay) if override and kind == "C" else pay, out, slots.get(i, -1)))
    return (prog, len(slots)) if h == 1 else (None, 0)


def evaluate(prog, X, TX, multi, out_len):
    """values (B, out_len) and tangents (B, out_len, K) of one tree on rows X (B, V) whose variables carry the tangents TX (B, V, K)"""
    B, dtype = X.shape[0], X.dtype
    zero = np.zeros((B, K), dtype)
    outs, outs_t = np.zeros((B, out_len), dtype), np.zeros((B, out_len, K), dtype)
    st = []
    with np.errstate(all="ignore"):
        for kind, pay, out, slot in prog:
            if kind in "CV":
                seed = zero + (np.arange(K) == slot).astype(dtype)   # (slot -1: no constant's seed)
                st.append((np.full(B, pay, dtype), seed) if kind == "C" else (X[:, pay], TX[:, pay]))
                continue
            if kind == "U":
                a, ta = last = st.pop()
                r = R.unary(pay, a).astype(dtype)
                tr = zero if pay is None else -ta if pay == R.F_NEG else R.unary_adjoint(pay, a, r, np.ones_like(a)).astype(dtype)[:, None] * ta
            elif kind == "B":
                (a, ta), (b, tb) = st.pop(), st.pop()
                r, last = R.binary(pay, a, b).astype(dtype), (b, tb)
                if pay is None or pay >= R.F_LT:
                    tr = zero
                elif pay in (R.F_ADD, R.F_SUB):
                    tr = ta + tb if pay == R.F_ADD else ta - tb
                else:
                    pa, pb = R.binary_adjoint(pay, a, b, r, np.ones_like(a))
                    tr = pa.astype(dtype)[:, None] * ta + pb.astype(dtype)[:, None] * tb
            else:
                (a, _), (b, tb), last = st.pop(), st.pop(), st.pop()
                r, tr = np.where(a > 0, b, last[0]), np.where((a > 0)[:, None], tb, last[1])
            if multi:
                if out is not None:
                    outs[:, out] = outs[:, out] + r
                    outs_t[:, out] = outs_t[:, out] + tr
                st.append(last)
            else:
                st.append((r, tr))
    return (outs, outs_t) if multi else (st[-1][0][:, None], st[-1][1][:, None])


def step(f, x, s, u, scheme, dt, dtype):
    """simulate_ref.step on the pair (x (B, S), s (B, S, K)): the same formula, in the same association, on values and tangents"""
    dt = F(dt)
    h2, h6 = dtype(F(dt * F(0.5))), dtype(F(dt / F(6)))
    dt, two = dtype(dt), dtype(2)
    zu = np.zeros(u.shape + (K,), dtype)
    call = lambda x, s: f(np.concatenate([x, u], 1), np.concatenate([s, zu], 1))  # noqa: E731
    pair = lambda g, *ps: tuple(g(*q) for q in zip(*ps))  # noqa: E731
    with np.errstate(all="ignore"):
        if scheme == "map":
            return call(x, s)
        if scheme == "euler":
            return pair(lambda x, k: x + dt * k, (x, s), call(x, s))
        if scheme == "narx":
            return pair(lambda x, k: np.concatenate([k[:, :1], x[:, :-1]], 1), (x, s), call(x, s))
        k1 = call(x, s)
        k2 = call(*pair(lambda x, k: x + h2 * k, (x, s), k1))
        k3 = call(*pair(lambda x, k: x + h2 * k, (x, s), k2))
        k4 = call(*pair(lambda x, k: x + dt * k, (x, s), k3))
        return pair(lambda x, a, b, c, d: x + h6 * (((a + two * b) + two * c) + d), (x, s), k1, k2, k3, k4)


def simulate(forest, var_len, x0, u, scheme, dt, dtype=F, trees=None, override=None):
    """``(states (pop, B, T, S), sens (pop, B, T, S, K), nc (pop,))`` in ``dtype``: NaN from the step a trajectory dies and for a malformed
    tree, slots k >= nc exactly 0.  ``override`` {node: value}: constants that replace the (float32) node words, for finite differences"""
    value, type_, size = forest
    pop, (B, S), T = value.shape[0], x0.shape, u.shape[1]
    multi = scheme != "narx" and S > 1
    out_len = S if multi else 1
    states, sens, ncs = np.full((pop, B, T, S), np.nan, dtype), np.full((pop, B, T, S, K), np.nan, dtype), np.zeros(pop, int)
    for t in range(pop) if trees is None else trees:
        prog, nc = program(value, type_, size, t, multi, var_len, out_len, override)
        ncs[t] = nc
        if prog is None:
            continue
        x, s, alive = x0.astype(dtype), np.zeros((B, S, K), dtype), np.ones(B, bool)
        for ts in range(T):
            x, s = step(lambda X, TX: evaluate(prog, X, TX, multi, out_len), x, s, u[:, ts].astype(dtype), scheme, dt, dtype)
            alive &= np.isfinite(x).all(1)
            states[t, alive, ts], sens[t, alive, ts] = x[alive], s[alive]
            sens[t, alive, ts, :, nc:] = 0
    return states, sens, ncs


def finite_differences(forest, var_len, x0, u, scheme, dt, t, h=1e-6):
    """central differences of the float64 restatement of tree t's states in each optimised constant: (B, T, S, nc)"""
    value, type_, size = forest
    run = lambda i, c: simulate(forest, var_len, x0, u, scheme, dt, np.float64, [t], {i: c})[0][t]  # noqa: E731
    where = [i for i in range(int(size[t, 0])) if type_[t, i] == R.T_CONST][:K]
    return np.stack([(run(i, float(value[t, i]) + h) - run(i, float(value[t, i]) - h)) / (2 * h) for i in where], -1)


def normal_equations(states, sens, target, weight):
    """longdouble ``(A (K, K), b (K,), sum|terms| of each)`` of one tree from its states (B, T, SC) and sens (B, T, SC, K): every product
    rounded to float32 as the kernel rounds it, the sums exact"""
    L = np.longdouble
    r32 = lambda a: a.astype(F).astype(L)  # noqa: E731
    J, r, w = sens.astype(L), (states - target).astype(L), np.asarray(weight, F).astype(L)
    wJ = r32(w[None, None, :, None] * J)
    tA, tb = r32(wJ[..., :, None] * J[..., None, :]), r32(wJ * r[..., None])
    return tuple(a.sum((0, 1, 2)) / L(r.shape[0] * r.shape[1]) for a in (tA, tb, np.abs(tA), np.abs(tb)))


def lm_tune(forest, var_len, x0, u, target, scheme, dt, steps, damping=1e-3):
    """evogp_hip_sr_lm_step's rule on tree 0 (unit state weights), driven by the float32 restatement: the loss before every step and after the last"""
    value, type_, size = (np.array(a) for a in forest)
    where = [i for i in range(int(size[0, 0])) if type_[0, i] == R.T_CONST][:K]
    n, lam = len(where), damping

    def model(v):
        states, sens, _ = simulate((v, type_, size), var_len, x0, u, scheme, dt)
        A, b = normal_equations(states[0], sens[0], target, np.ones(target.shape[-1]))[:2]
        d = states[0].astype(np.float64) - target
        return float((d * d).mean((0, 1)).sum()), A[:n, :n].astype(np.float64), b[:n].astype(np.float64)

    cur = model(value)
    history = [cur[0]]
    for _ in range(steps):
        cand = value.copy()
        cand[0, where] = (value[0, where] + np.linalg.solve(cur[1] + lam * np.diag(np.diag(cur[1])), -cur[2])).astype(F)
        new = model(cand)
        if new[0] < cur[0]:
            value, cur, lam = cand, new, max(lam / 10, 1e-10)
        else:
            lam = min(lam * 10, 1e10)
        history.append(cur[0])
    return history
