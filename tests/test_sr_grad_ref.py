"""CPU: the float64 numpy reference of the constant-gradient pass (tests/sr_grad_ref.py) -- the yardstick of the GPU tests --
agrees with torch float64 autograd on trees away from the edge points, and implements the edge cases of the adjoint table."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sr_grad_ref as R  # noqa: E402
from grad_trees import ALL_FUNCS, ARITH, out_word, random_forest  # noqa: E402


def torch_tree(value, type_, size, X, y, use_mse):
    """(loss, {node: grad}) by torch autograd over an independent restatement of the forward pass (float64)"""
    D, var_len = X.shape
    out_len = y.shape[1]
    multi = out_len > 1
    n = int(size[0])
    Xt, yt = torch.from_numpy(X.astype(np.float64)), torch.from_numpy(y.astype(np.float64))
    leaves, stack = {}, []
    outs = [torch.zeros(D, dtype=torch.float64) for _ in range(out_len)]
    un = {R.F_SIN: torch.sin, R.F_COS: torch.cos, R.F_TAN: torch.tan, R.F_SINH: torch.sinh, R.F_COSH: torch.cosh, R.F_TANH: torch.tanh,
          R.F_LOG: torch.log, R.F_LOOSE_LOG: lambda a: torch.log(torch.abs(a)), R.F_EXP: torch.exp, R.F_INV: lambda a: 1 / a,
          R.F_LOOSE_INV: lambda a: 1 / a, R.F_NEG: torch.neg, R.F_ABS: torch.abs, R.F_SQRT: torch.sqrt,
          R.F_LOOSE_SQRT: lambda a: torch.sqrt(torch.abs(a))}
    one = torch.ones(D, dtype=torch.float64)
    bi = {R.F_ADD: torch.add, R.F_SUB: torch.sub, R.F_MUL: torch.mul, R.F_DIV: torch.div, R.F_LOOSE_DIV: torch.div, R.F_POW: torch.pow,
          R.F_LOOSE_POW: lambda a, b: torch.pow(torch.abs(a), b), R.F_MAX: lambda a, b: torch.where(a >= b, a, b),
          R.F_MIN: lambda a, b: torch.where(a <= b, a, b), R.F_LT: lambda a, b: torch.where(a < b, one, -one),
          R.F_GT: lambda a, b: torch.where(a > b, one, -one), R.F_LE: lambda a, b: torch.where(a <= b, one, -one),
          R.F_GE: lambda a, b: torch.where(a >= b, one, -one)}
    for i in reversed(range(n)):
        kind, f, out = R.decode(type_[i], value[i], multi, var_len, out_len)
        if kind == "C":
            c = torch.tensor(f, dtype=torch.float64, requires_grad=True)
            leaves[i] = c
            stack.append(c.expand(D))
        elif kind == "V":
            stack.append(Xt[:, f])
        else:
            ops = [stack.pop() for _ in range(R.ARITY[kind])]
            r = un[f](ops[0]) if kind == "U" else bi[f](ops[0], ops[1]) if kind == "B" else torch.where(ops[0] > 0, ops[1], ops[2])
            if multi:
                if out is not None:
                    outs[out] = outs[out] + r
                stack.append(ops[-1])
            else:
                stack.append(r)
    pred = torch.stack(outs) if multi else stack[-1][None, :]
    diff = pred - yt.T
    loss = (diff * diff if use_mse else torch.abs(diff)).sum() / D
    if not loss.requires_grad:   # (no constant reaches the loss)
        return float(loss), {i: 0.0 for i in leaves}
    gs = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)
    return float(loss.detach()), {i: (0.0 if g is None else float(g)) for i, g in zip(leaves, gs)}


@pytest.mark.parametrize("out_len", [1, 3])
@pytest.mark.parametrize("funcs", ["arith", "all"])
@pytest.mark.parametrize("use_mse", [True, False])
def test_reference_matches_torch_autograd(rng, out_len, funcs, use_mse):
    fs = ARITH if funcs == "arith" else ALL_FUNCS
    var_len, D = 3, 17
    value, type_, size = random_forest(rng, 60, 64, fs, var_len, out_len, max_depth=5)
    X = rng.uniform(0.5, 1.5, (D, var_len)).astype(np.float32)
    y = rng.uniform(-1, 1, (D, out_len)).astype(np.float32)
    loss, grad, _ = R.forest_grad(value, type_, size, X, y, use_mse)
    compared, seen = 0, set()
    for t in range(value.shape[0]):
        want_loss, want = torch_tree(value[t], type_[t], size[t], X, y, use_mse)
        n = int(size[t, 0])
        assert np.all(grad[t][n:] == 0)
        consts = {i for i in range(n) if type_[t, i] & 0x7F == R.T_CONST}
        assert set(want) == consts and np.all(grad[t][[i for i in range(n) if i not in consts]] == 0)
        if not np.isfinite(want_loss):
            continue   # rule: trees whose loss is not finite are outside "away from the edge points"
        assert loss[t] == pytest.approx(want_loss, rel=1e-12, abs=1e-300)
        for i, g in want.items():
            if np.isfinite(g):
                assert grad[t, i] == pytest.approx(g, rel=1e-9, abs=1e-12), (t, i)
                compared += 1
        seen |= {int(np.float32(v).view(np.uint32) & 0xFFFF) if ty & 0x80 else int(v) for v, ty in zip(value[t, :n], type_[t, :n])
                 if ty & 0x7F >= R.T_UFUNC}
    assert compared >= 40
    if funcs == "all" and out_len == 1:
        assert len(seen) >= 20   # the forests reach most of the 29 functions


def test_reference_covers_every_function_against_autograd(rng):
    """one small tree per function, on operands away from its edge points"""
    X = rng.uniform(0.6, 1.4, (9, 2)).astype(np.float32)
    y = rng.uniform(-1, 1, (9, 1)).astype(np.float32)
    for f in ALL_FUNCS:
        if f == R.F_IF:
            rows = [(0, 4, 4), (0.7, 1, 1), (1.3, 1, 1), (0, 0, 1)]          # IF(0.7, 1.3, x0)
        elif f >= R.F_SIN:
            rows = [(f, 2, 4), (R.F_MUL, 3, 3), (0.8, 1, 1), (1, 0, 1)]      # f(0.8 * x1)
        else:
            rows = [(f, 3, 3), (1.2, 1, 1), (0, 0, 1)]                      # f(1.2, x0)
        value = np.array([[r[0] for r in rows]], np.float32)
        type_ = np.array([[r[1] for r in rows]], np.int16)
        size = np.array([[r[2] for r in rows]], np.int16)
        loss, grad, _ = R.forest_grad(value, type_, size, X, y, True)
        want_loss, want = torch_tree(value[0], type_[0], size[0], X, y, True)
        assert loss[0] == pytest.approx(want_loss, rel=1e-12), f
        for i, g in want.items():
            assert grad[0, i] == pytest.approx(g, rel=1e-9, abs=1e-12), (f, i)


def _one(rows, X, y, use_mse=True):
    value = np.array([[r[0] for r in rows]], np.float32)
    type_ = np.array([[r[1] for r in rows]], np.int16)
    size = np.array([[r[2] for r in rows]], np.int16)
    return R.forest_grad(value, type_, size, X, y, use_mse)


X1 = np.array([[2.0]], np.float32)
Y0 = np.array([[0.0]], np.float32)


def test_edge_div_by_zero():
    # x0 / c with c = 0: the result is NaN and so is the adjoint of the divisor
    loss, grad, _ = _one([(R.F_DIV, 3, 3), (0, 0, 1), (0.0, 1, 1)], X1, Y0)
    assert np.isnan(loss[0]) and np.isnan(grad[0, 2])


def test_edge_loose_div_tiny_divisor():
    # c1 / c2 with |c2| <= delta: the divisor gets no adjoint, the dividend g / copysign(delta, b)
    loss, grad, _ = _one([(R.F_LOOSE_DIV, 3, 3), (1e-12, 1, 1), (0.0, 1, 1)], X1, np.array([[0.0]], np.float32))
    r = float(np.float32(1e-12)) / R.DELTA
    assert grad[0, 2] == 0.0
    assert grad[0, 1] == pytest.approx(2 * r / R.DELTA)


def test_edge_max_min_ties_go_to_a():
    for f in (R.F_MAX, R.F_MIN):
        loss, grad, _ = _one([(f, 3, 3), (1.5, 1, 1), (1.5, 1, 1)], X1, Y0)
        assert grad[0, 1] == pytest.approx(2 * 1.5) and grad[0, 2] == 0.0


def test_edge_if_branches():
    # IF(c0, c1, c2): no adjoint to the condition, all of it to the branch taken
    for cond, taken, other in ((0.5, 2, 3), (0.0, 3, 2), (-1.0, 3, 2)):
        loss, grad, _ = _one([(0, 4, 4), (cond, 1, 1), (3.0, 1, 1), (5.0, 1, 1)], X1, Y0)
        val = 3.0 if taken == 2 else 5.0
        assert grad[0, 1] == 0.0 and grad[0, other] == 0.0 and grad[0, taken] == pytest.approx(2 * val)


def test_edge_abs_and_loose_sqrt_at_zero():
    for f in (R.F_ABS, R.F_LOOSE_SQRT):
        loss, grad, _ = _one([(f, 2, 2), (0.0, 1, 1)], X1, np.array([[1.0]], np.float32))
        assert np.isfinite(loss[0]) and grad[0, 1] == 0.0


def test_edge_pow_non_positive_base():
    # pow(c1, c2) with c1 <= 0: the exponent gets no adjoint; the base g * b * pow(a, b - 1)
    loss, grad, _ = _one([(R.F_POW, 3, 3), (-2.0, 1, 1), (2.0, 1, 1)], X1, Y0)
    assert grad[0, 2] == 0.0 and grad[0, 1] == pytest.approx(2 * 4.0 * 2.0 * -2.0)
    loss, grad, _ = _one([(R.F_POW, 3, 3), (0.0, 1, 1), (2.0, 1, 1)], X1, Y0)
    assert grad[0, 2] == 0.0 and grad[0, 1] == 0.0
    # loose pow at a == b == 0: no adjoint at all
    loss, grad, _ = _one([(R.F_LOOSE_POW, 3, 3), (0.0, 1, 1), (0.0, 1, 1)], X1, Y0)
    assert grad[0, 1] == 0.0 and grad[0, 2] == 0.0


def test_edge_mae_sign_zero_and_malformed():
    loss, grad, _ = _one([(R.F_ADD, 3, 3), (1.0, 1, 1), (1.0, 1, 1)], X1, np.array([[2.0]], np.float32), use_mse=False)
    assert loss[0] == 0.0 and grad[0, 1] == 0.0 and grad[0, 2] == 0.0
    loss, grad, _ = _one([(R.F_ADD, 3, 2), (1.0, 1, 1), (0.0, 0, 0)], X1, Y0)   # one operand short: malformed
    assert np.isnan(loss[0]) and np.all(grad == 0)


def test_multi_output_pass_through():
    # outs[0] += c1 * c2 (OUT node), the node hands c2 on to its parent: a non-OUT ADD whose r is dropped, itself handing on x0
    X = np.array([[3.0], [1.0]], np.float32)
    y = np.array([[1.0, 0.0], [0.5, 0.0]], np.float32)
    rows = [(R.F_ADD, 3, 5), (out_word(R.F_MUL, 0), 3 | 0x80, 3), (2.0, 1, 1), (5.0, 1, 1), (0, 0, 1)]
    loss, grad, _ = _one(rows, X, y)
    # outs[0] = 10 on both rows, outs[1] = 0; d loss / d c1 = (1/2) sum 2 (10 - y0) * c2, d / d c2 = (1/2) sum 2 (10 - y0) * c1
    assert loss[0] == pytest.approx(((10 - 1) ** 2 + (10 - 0.5) ** 2) / 2)
    assert grad[0, 2] == pytest.approx((2 * 9 * 5 + 2 * 9.5 * 5) / 2)
    assert grad[0, 3] == pytest.approx((2 * 9 * 2 + 2 * 9.5 * 2) / 2)
