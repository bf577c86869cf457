"""TEST-ONLY: a numpy restatement of the second input derivatives (csrc/sr_hessian.hip, rules of csrc/sr_hyperdual.hpp): a tree interpreted
on hyper-dual numbers (v, t_a, t_b, t_ab).  Decoding, the forward semantics and the first partials are those of tests/sr_grad_ref.py and
tests/input_grad_ref.py (imported, not copied); what is new are the second partials and the way the four words combine.

``forest_hessian(value, type, size, X, pairs, dtype)`` -> ``(pred (pop, D), h (P, pop, D))``: h[k][t][r] = d^2 tree_t / dx_a dx_b at X[r]
for pairs[k] = (a, b).  At float64 it is the reference; at float32 the reference's own rounding yardstick.  Malformed trees: NaN
everywhere.  A pair whose variables the tree does not both hold: +0.0.
``curvature_loss(pred32, h32, y, ...)``: the fused epilogue on float32 arrays (input_grad_ref.loss_columns: the same definition)."""
import numpy as np

from input_grad_ref import loss_columns as curvature_loss  # noqa: F401
from input_grad_ref import well_formed
from sr_grad_ref import (ARITY, DELTA, F_ABS, F_ADD, F_COS, F_COSH, F_DIV, F_EXP, F_GE, F_INV, F_LOG, F_LOOSE_DIV, F_LOOSE_INV,
                         F_LOOSE_LOG, F_LOOSE_POW, F_LOOSE_SQRT, F_LT, F_MAX, F_MIN, F_MUL, F_NEG, F_POW, F_SIN, F_SINH, F_SQRT, F_SUB,
                         F_TAN, F_TANH, binary, binary_adjoint, decode, unary, unary_adjoint)

PAIR = 1 << 30


def code(a, b):
    return PAIR | a << 15 | b


def unary_second(f, a, r):
    with np.errstate(all="ignore"):
        z = np.zeros_like(a)
        if f in (F_SIN, F_COS): return -r
        if f == F_TAN: return 2 * r * (1 + r * r)
        if f in (F_SINH, F_COSH, F_EXP): return r
        if f == F_TANH: return -2 * r * (1 - r * r)
        if f == F_LOG: return -1 / (a * a)
        if f == F_LOOSE_LOG: return np.where(a == 0, z, -1 / (a * a))
        if f == F_INV: return np.where(a == 0, np.nan, 2 * r * r * r)
        if f == F_LOOSE_INV: return np.where(np.abs(a) <= DELTA, z, 2 * r * r * r)
        if f == F_SQRT: return -0.25 / (a * r)
        if f == F_LOOSE_SQRT: return np.where(a == 0, z, -0.25 / (np.abs(a) * r))
        return z   # abs, unknown ids


def pow_second(loose, a, b, r, ga, gb):
    with np.errstate(all="ignore"):
        m = np.abs(a) if loose else a
        pos = m > 0
        lm = np.log(np.where(pos, m, 1))
        gaa = b * (b - 1) * np.power(m, b - 2)
        gab = np.power(m, b - 1) * (1 + b * lm)
        if loose:
            gab = gab * np.sign(a)
            gaa = np.where(a == 0, 0, gaa)
        gab = np.where(pos, gab, 0)
        gbb = np.where(pos, r * lm * lm, 0)
        bad = np.isnan(ga) | np.isnan(gb)
        return [np.where(bad, np.nan, g) for g in (gaa, gab, gbb)]


def hd_unary(f, A, one):
    a, aa, ab, aab = A
    r = unary(f, a)
    if f == F_NEG:
        return r, -aa, -ab, -aab
    if f is None:
        return r, 0 * one, 0 * one, 0 * one
    f1, f2 = unary_adjoint(f, a, r, one), unary_second(f, a, r)
    return r, f1 * aa, f1 * ab, f2 * aa * ab + f1 * aab


def hd_binary(f, A, B, one):
    (a, aa, ab, aab), (b, ba, bb, bab) = A, B
    r = binary(f, a, b)
    zero = 0 * one
    if f == F_ADD: return r, aa + ba, ab + bb, aab + bab
    if f == F_SUB: return r, aa - ba, ab - bb, aab - bab
    if f == F_MUL: return r, aa * b + a * ba, ab * b + a * bb, aab * b + a * bab + aa * bb + ab * ba
    if f in (F_DIV, F_LOOSE_DIV):
        tiny = (np.abs(b) <= DELTA) if f == F_LOOSE_DIV else np.zeros(b.shape, bool)
        d = np.where(tiny, np.copysign(one * DELTA, b), b)
        ra, rb = (aa - r * ba) / d, (ab - r * bb) / d
        rab = (aab - ra * bb - rb * ba - r * bab) / d
        return r, np.where(tiny, aa / d, ra), np.where(tiny, ab / d, rb), np.where(tiny, aab / d, rab)
    if f in (F_MAX, F_MIN):
        c = a >= b if f == F_MAX else a <= b
        return tuple(np.where(c, x, y) for x, y in zip(A, B))
    if f is None or F_LT <= f <= F_GE:
        return r, zero, zero, zero
    ga, gb = binary_adjoint(f, a, b, r, one)
    gaa, gab, gbb = pow_second(f == F_LOOSE_POW, a, b, r, ga, gb)
    return (r, ga * aa + gb * ba, ga * ab + gb * bb,
            ga * aab + gb * bab + gaa * aa * ab + gab * (aa * bb + ab * ba) + gbb * ba * bb)


def tree_hessian(value, type_, size, X, pairs, dtype=np.float64):
    L, (D, var_len) = len(value), X.shape
    n = min(max(int(size[0]), 0), L)
    nodes = [decode(type_[i], value[i], False, var_len, 1) for i in range(n)]
    if not well_formed(nodes):
        return np.full(D, np.nan, dtype), np.full((len(pairs), D), np.nan, dtype)
    X = X.astype(dtype)
    one, zero = np.ones(D, dtype), np.zeros(D, dtype)
    held = {f for kind, f, _ in nodes if kind == "V"}
    pred, h = None, np.zeros((len(pairs), D), dtype)
    with np.errstate(all="ignore"):
        for k, (va, vb) in enumerate(list(pairs) + [(-1, -1)]):   # the last run is the plain one: the prediction
            if k < len(pairs) and not (va in held and vb in held):
                continue
            stack = []
            for kind, f, _ in reversed(nodes):
                if kind == "C":
                    e = (np.full(D, f, dtype), zero, zero, zero)
                elif kind == "V":
                    e = (X[:, f], one if f == va else zero, one if f == vb else zero, zero)
                else:
                    ops = [stack.pop() for _ in range(ARITY[kind])]   # top of stack first: a, b, c
                    if kind == "U":
                        e = hd_unary(f, ops[0], one)
                    elif kind == "B":
                        e = hd_binary(f, ops[0], ops[1], one)
                    else:
                        e = tuple(np.where(ops[0][0] > 0, x, y) for x, y in zip(ops[1], ops[2]))
                    e = tuple(np.asarray(x, dtype) + zero for x in e)
                stack.append(e)
            if k < len(pairs):
                h[k] = stack[0][3]
            else:
                pred = stack[0][0]
    return pred, h


def forest_hessian(value, type_, size, X, pairs, dtype=np.float64):
    value, type_, size, X = np.asarray(value), np.asarray(type_), np.asarray(size), np.asarray(X)
    pop, D, P = value.shape[0], X.shape[0], len(pairs)
    pred, h = np.zeros((pop, D), dtype), np.zeros((P, pop, D), dtype)
    for t in range(pop):
        pred[t], h[:, t] = tree_hessian(value[t], type_[t], size[t], X, pairs, dtype)
    return pred, h
