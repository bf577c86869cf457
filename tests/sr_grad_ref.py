"""TEST-ONLY: a float64 numpy restatement of the constant-gradient pass (csrc/sr_grad.hip): the forward semantics of the
stack interpreter (csrc/interp.hpp run_general, both output modes) and the adjoint table of DESIGN.md "Constant gradients".

``forest_grad(value, type, size, X, y, use_mse)`` -> ``(loss, grad, gabs)``:
    loss[t]     (1/D) sum_d sum_o err(y[d][o] - tree_t(X[d])_o)
    grad[t][i]  d loss[t] / d value[t][i] at CONST nodes, 0 elsewhere
    gabs[t][i]  (1/D) sum_d |d err_d / d value[t][i]|: the scale of the per-entry tolerance of the GPU tests
Malformed trees: NaN loss, zero rows."""
import numpy as np

DELTA = float(np.float32(1e-9))
MAXVAL = float(np.float32(1e9))
T_VAR, T_CONST, T_UFUNC, T_BFUNC = 0, 1, 2, 3
(F_IF, F_ADD, F_SUB, F_MUL, F_DIV, F_LOOSE_DIV, F_POW, F_LOOSE_POW, F_MAX, F_MIN, F_LT, F_GT, F_LE, F_GE, F_SIN, F_COS, F_TAN,
 F_SINH, F_COSH, F_TANH, F_LOG, F_LOOSE_LOG, F_EXP, F_INV, F_LOOSE_INV, F_NEG, F_ABS, F_SQRT, F_LOOSE_SQRT) = range(29)


def decode(t, v, multi, var_len, out_len):
    """-> (kind, payload, out): kind 'C' (value), 'V' (variable index), 'U' / 'B' (function id or None = unknown id), 'T'."""
    t = int(t)
    out = None
    is_out = False
    if multi:
        is_out = (t & 0x80) != 0
        t &= 0x7F
    if t == T_CONST:
        return "C", float(np.float32(v)), None
    if t == T_VAR:
        k = int(np.float32(v))
        return "V", min(max(k, 0), var_len - 1), None
    f = int(np.float32(v)) & 0xFFFFFFFF
    if multi and is_out:
        bits = int(np.float32(v).view(np.uint32))
        f = int(np.int16(np.uint16(bits & 0xFFFF)))
        oi = int(np.int16(np.uint16(bits >> 16)))
        if 0 <= oi < out_len:
            out = oi
    if t == T_UFUNC:
        return "U", (f if F_SIN <= f <= F_LOOSE_SQRT else None), out
    if t == T_BFUNC:
        return "B", (f if F_ADD <= f <= F_GE else None), out
    return "T", None, out


ARITY = {"C": 0, "V": 0, "U": 1, "B": 2, "T": 3}


def _where(c, x, y):
    return np.where(c, x, y)


def unary(f, a):
    with np.errstate(all="ignore"):
        if f is None:
            return np.zeros_like(a)
        return {
            F_SIN: np.sin, F_COS: np.cos, F_TAN: np.tan, F_SINH: np.sinh, F_COSH: np.cosh, F_TANH: np.tanh, F_LOG: np.log,
            F_LOOSE_LOG: lambda a: _where(a == 0, -MAXVAL, np.log(np.abs(a))), F_EXP: np.exp,
            F_INV: lambda a: _where(a == 0, np.nan, 1.0 / a),
            F_LOOSE_INV: lambda a: 1.0 / _where(np.abs(a) <= DELTA, np.copysign(DELTA, a), a),
            F_NEG: np.negative, F_ABS: np.abs, F_SQRT: np.sqrt, F_LOOSE_SQRT: lambda a: np.sqrt(np.abs(a)),
        }[f](a)


def binary(f, a, b):
    with np.errstate(all="ignore"):
        if f is None:
            return np.zeros_like(a)
        if f == F_ADD: return a + b
        if f == F_SUB: return a - b
        if f == F_MUL: return a * b
        if f == F_DIV: return _where(b == 0, np.nan, a / b)
        if f == F_LOOSE_DIV: return a / _where(np.abs(b) <= DELTA, np.copysign(DELTA, b), b)
        if f == F_POW: return np.power(a, b)
        if f == F_LOOSE_POW: return _where((a == 0) & (b == 0), 0.0, np.power(np.abs(a), b))
        if f == F_MAX: return _where(a >= b, a, b)
        if f == F_MIN: return _where(a <= b, a, b)
        if f == F_LT: return _where(a < b, 1.0, -1.0)
        if f == F_GT: return _where(a > b, 1.0, -1.0)
        if f == F_LE: return _where(a <= b, 1.0, -1.0)
        if f == F_GE: return _where(a >= b, 1.0, -1.0)


def unary_adjoint(f, a, r, g):
    with np.errstate(all="ignore"):
        if f is None: return np.zeros_like(a)
        if f == F_SIN: return g * np.cos(a)
        if f == F_COS: return -g * np.sin(a)
        if f == F_TAN: return g * (1 + r * r)
        if f == F_SINH: return g * np.cosh(a)
        if f == F_COSH: return g * np.sinh(a)
        if f == F_TANH: return g * (1 - r * r)
        if f == F_LOG: return g / a
        if f == F_LOOSE_LOG: return _where(a == 0, 0.0, g / a)
        if f == F_EXP: return g * r
        if f == F_INV: return _where(a == 0, np.nan, -g * r * r)
        if f == F_LOOSE_INV: return _where(np.abs(a) <= DELTA, 0.0, -g * r * r)
        if f == F_NEG: return -g
        if f == F_ABS: return g * np.sign(a)
        if f == F_SQRT: return g * 0.5 / r
        if f == F_LOOSE_SQRT: return _where(a == 0, 0.0, g * 0.5 / r * np.sign(a))


def binary_adjoint(f, a, b, r, g):
    z = np.zeros_like(a)
    with np.errstate(all="ignore"):
        if f is None or f in (F_LT, F_GT, F_LE, F_GE): return z, z
        if f == F_ADD: return g, g
        if f == F_SUB: return g, -g
        if f == F_MUL: return g * b, g * a
        if f == F_DIV: return g / b, -g * r / b
        if f == F_LOOSE_DIV:
            tiny = np.abs(b) <= DELTA
            d = _where(tiny, np.copysign(DELTA, b), b)
            return g / d, _where(tiny, 0.0, -g * r / d)
        if f == F_POW:
            return g * b * np.power(a, b - 1), _where(a > 0, g * r * np.log(_where(a > 0, a, 1.0)), 0.0)
        if f == F_LOOSE_POW:
            m = np.abs(a)
            da = _where((a == 0) & (b == 0), 0.0, g * b * np.power(m, b - 1) * np.sign(a))
            return da, _where(m > 0, g * r * np.log(_where(m > 0, m, 1.0)), 0.0)
        if f == F_MAX: c = a >= b; return _where(c, g, 0.0), _where(c, 0.0, g)
        if f == F_MIN: c = a <= b; return _where(c, g, 0.0), _where(c, 0.0, g)


def tree_grad(value, type_, size, X, y, use_mse=True):
    """one tree: (loss, grad[L], gabs[L]) in float64"""
    L = len(value)
    D, var_len = X.shape
    out_len = y.shape[1]
    multi = out_len > 1
    n = min(max(int(size[0]), 0), L)
    grad = np.zeros(L)
    gabs = np.zeros(L)
    nodes = [decode(type_[i], value[i], multi, var_len, out_len) for i in range(n)]
    h = 0
    for i in reversed(range(n)):
        h += 1 - ARITY[nodes[i][0]]
        if h < 1:
            return np.nan, grad, gabs
    if n <= 0 or h != 1:
        return np.nan, grad, gabs
    X = X.astype(np.float64)
    y = y.astype(np.float64)
    val, res, kids = [None] * n, [None] * n, [None] * n
    outs = np.zeros((out_len, D))
    stack = []
    for i in reversed(range(n)):
        kind, f, out = nodes[i]
        if kind == "C":
            val[i] = np.full(D, f)
        elif kind == "V":
            val[i] = X[:, f]
        else:
            k = [stack.pop() for _ in range(ARITY[kind])]   # top of stack first: a, b, c
            kids[i] = k
            ops = [val[j] for j in k]
            if kind == "U":
                r = unary(f, ops[0])
            elif kind == "B":
                r = binary(f, ops[0], ops[1])
            else:
                r = _where(ops[0] > 0, ops[1], ops[2])
            res[i] = r
            if multi:
                if out is not None:
                    outs[out] += r
                val[i] = ops[-1]
            else:
                val[i] = r
        stack.append(i)
    pred = outs if multi else val[0][None, :]
    with np.errstate(all="ignore"):
        diff = pred - y.T
        loss = float(np.sum(diff * diff if use_mse else np.abs(diff)) / D)
        gout = (2.0 * diff if use_mse else np.sign(diff)) / D
    adj = [None] * n
    adj[0] = np.zeros(D) if multi else gout[0]
    for i in range(n):
        kind, f, out = nodes[i]
        if kind == "C":
            grad[i] += np.sum(adj[i])
            with np.errstate(all="ignore"):
                gabs[i] += np.sum(np.abs(adj[i]))
            continue
        if kind == "V":
            continue
        g = adj[i]
        k = kids[i]
        ops = [val[j] for j in k]
        through = (not multi) or out is not None
        gr = (gout[out] if multi else g) if through else np.zeros(D)
        zero = np.zeros(D)
        with np.errstate(all="ignore"):
            if kind == "U":
                d = [unary_adjoint(f, ops[0], res[i], gr) if through else zero]
            elif kind == "B":
                d = list(binary_adjoint(f, ops[0], ops[1], res[i], gr)) if through else [zero, zero]
            else:
                take_b = ops[0] > 0
                d = [zero, _where(take_b, gr, 0.0) if through else zero, _where(take_b, 0.0, gr) if through else zero]
            if multi:
                d[-1] = d[-1] + g
        for j, dj in zip(k, d):
            adj[j] = dj
    return loss, grad, gabs


def forest_grad(value, type_, size, X, y, use_mse=True):
    value, type_, size = np.asarray(value), np.asarray(type_), np.asarray(size)
    X, y = np.asarray(X), np.asarray(y)
    if y.ndim == 1:
        y = y[:, None]
    pop, L = value.shape
    loss = np.zeros(pop)
    grad = np.zeros((pop, L))
    gabs = np.zeros((pop, L))
    for t in range(pop):
        loss[t], grad[t], gabs[t] = tree_grad(value[t], type_[t], size[t], X, y, use_mse)
    return loss, grad, gabs


def const_step(value, type_, size, cand, loss, grad, loss_cand, grad_cand, step, out_len, phase):
    """float32 restatement of evogp_hip_sr_const_step on numpy arrays, in place (the test-only CPU kernel of tree_SR_const_step)"""
    multi = out_len > 1
    pop, L = value.shape
    for t in range(pop):
        n = min(max(int(size[t, 0]), 0), L)
        ty = type_[t].astype(np.int32)
        is_c = ((ty & 0x7F) if multi else ty) == T_CONST
        is_c[n:] = False
        if phase & 1:
            if loss_cand[t] < loss[t]:
                value[t, is_c] = cand[t, is_c]
                grad[t] = grad_cand[t]
                loss[t] = loss_cand[t]
                step[t] = np.float32(2) * step[t]
            else:
                step[t] = np.float32(0.5) * step[t]
        if phase & 2:
            with np.errstate(all="ignore"):
                norm = np.sqrt(np.sum(grad[t].astype(np.float32) ** 2, dtype=np.float32), dtype=np.float32)
                move = np.isfinite(loss[t]) and loss[t] != 0 and np.isfinite(norm) and norm != 0
                cand[t] = value[t]
                if move:
                    cand[t, is_c] = (value[t, is_c] - step[t] * grad[t, is_c] / norm).astype(np.float32)
