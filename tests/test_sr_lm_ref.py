"""CPU: the float64 reference of the Levenberg-Marquardt constant optimiser (tests/sr_lm_ref.py) checked on its own: its per-row
Jacobian against torch autograd on hand-written trees, its normal equations against the gradient reference, and its loop against
numpy's least squares on trees that are linear in their constants."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sr_grad_ref as R  # noqa: E402
import sr_lm_ref as LM  # noqa: E402
from grad_trees import ALL_FUNCS, random_forest  # noqa: E402

C, V, U, B, T = R.T_CONST, R.T_VAR, R.T_UFUNC, R.T_BFUNC, 4


def _row(nodes, L=16):
    """nodes: (value, type, size) in prefix order -> one padded row of each array"""
    value, type_, size = np.zeros(L, np.float32), np.zeros(L, np.int16), np.zeros(L, np.int16)
    for i, (v, t, s) in enumerate(nodes):
        value[i], type_[i], size[i] = v, t, s
    return value, type_, size


# (prefix nodes, the same model in torch over the constants c[0..] in prefix order and the columns of X)
HAND_TREES = [
    # c0 * x0 + c1
    ([(R.F_ADD, B, 5), (R.F_MUL, B, 3), (1.5, C, 1), (0, V, 1), (-0.5, C, 1)],
     lambda c, X: c[0] * X[:, 0] + c[1]),
    # c0 * sin(c1 * x0) + c2
    ([(R.F_ADD, B, 8), (R.F_MUL, B, 6), (1.0, C, 1), (R.F_SIN, U, 4), (R.F_MUL, B, 3), (1.5, C, 1), (0, V, 1), (0.25, C, 1)],
     lambda c, X: c[0] * torch.sin(c[1] * X[:, 0]) + c[2]),
    # exp(c0 * x1) / (c1 + x0 * x0)
    ([(R.F_DIV, B, 10), (R.F_EXP, U, 4), (R.F_MUL, B, 3), (0.7, C, 1), (1, V, 1), (R.F_ADD, B, 5), (2.0, C, 1), (R.F_MUL, B, 3), (0, V, 1), (0, V, 1)],
     lambda c, X: torch.exp(c[0] * X[:, 1]) / (c[1] + X[:, 0] * X[:, 0])),
    # if(x0, c0 * x1, tanh(c1)) - sqrt(c2)
    ([(R.F_SUB, B, 10), (R.F_IF, T, 7), (0, V, 1), (R.F_MUL, B, 3), (1.25, C, 1), (1, V, 1), (R.F_TANH, U, 2), (0.5, C, 1), (R.F_SQRT, U, 2), (2.0, C, 1)],
     lambda c, X: torch.where(X[:, 0] > 0, c[0] * X[:, 1], torch.tanh(c[1])) - torch.sqrt(c[2])),
    # a lone constant
    ([(0.3, C, 1)], lambda c, X: c[0] + 0 * X[:, 0]),
    # 0 * c0 + c1: the first constant has no influence
    ([(R.F_ADD, B, 5), (R.F_MUL, B, 3), (0.0, C, 1), (2.0, C, 1), (1.0, C, 1)],
     lambda c, X: c[0] * c[1] + c[2] + 0 * X[:, 0]),
]


@pytest.mark.parametrize("case", range(len(HAND_TREES)))
def test_jacobian_equals_torch_autograd(case):
    nodes, model = HAND_TREES[case]
    value, type_, size = _row(nodes)
    rng = np.random.default_rng(case)
    X = rng.uniform(-1, 1, (37, 2)).astype(np.float32)
    pred, J, cidx = LM.tree_jacobian(value, type_, size, X)
    consts = [i for i, n in enumerate(nodes) if n[1] == C]
    assert list(cidx[:len(consts)]) == consts and np.all(cidx[len(consts):] == -1)
    c = torch.tensor([float(np.float32(nodes[i][0])) for i in consts], dtype=torch.float64, requires_grad=True)
    Xt = torch.from_numpy(X.astype(np.float64))
    want = torch.autograd.functional.jacobian(lambda c: model(c, Xt), c).numpy()
    np.testing.assert_allclose(pred, model(c, Xt).detach().numpy(), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(J[:, :len(consts)], want, rtol=1e-10, atol=1e-13)
    assert np.all(J[:, len(consts):] == 0)


def test_only_the_first_eight_constants_are_optimised():
    # c0 + (c1 + (... + c10)): 11 constants, a right comb of 10 additions
    nodes = []
    for k in range(10):
        nodes += [(R.F_ADD, B, 21 - 2 * k), (float(k + 1), C, 1)]
    nodes.append((11.0, C, 1))
    value, type_, size = _row(nodes, 32)
    X = np.zeros((5, 1), np.float32)
    pred, J, cidx = LM.tree_jacobian(value, type_, size, X)
    assert list(cidx) == [1, 3, 5, 7, 9, 11, 13, 15]
    assert np.all(J == 1.0) and np.all(pred == 66.0)
    size[0] = 7                      # a live prefix that ends inside the row hides the rest: malformed here, no Jacobian
    assert LM.tree_jacobian(value, type_, size, X) is None


def test_normal_equations_agree_with_the_gradient_reference(rng):
    value, type_, size = random_forest(rng, 40, 32, ALL_FUNCS, 2, 1, max_depth=4)
    size[3, 0] = 0
    X = rng.uniform(0.5, 1.5, (50, 2)).astype(np.float32)
    y = rng.uniform(-1, 1, (50, 1)).astype(np.float32)
    with np.errstate(all="ignore"):
        loss, normal, nabs = LM.forest_normal_eq(value, type_, size, X, y)
        gloss, grad, _ = R.forest_grad(value, type_, size, X, y)
    assert np.isnan(loss[3]) and np.all(normal[3] == 0)
    np.testing.assert_allclose(loss, gloss, rtol=1e-12, equal_nan=True)
    checked = 0
    for t in range(40):
        cidx = LM.optimised_consts(type_[t], size[t])
        A, b = LM.unpack(normal[t])
        for j, c in enumerate(cidx):
            if c < 0:
                assert np.all(A[j] == 0) and np.all(A[:, j] == 0) and b[j] == 0
            elif np.isfinite(grad[t, c]) and np.isfinite(b[j]):
                assert abs(b[j] - grad[t, c] / 2) <= 1e-9 * nabs[t, len(LM.TRI) + j] + 1e-300
                checked += 1
    assert checked > 40


def _linear_tree(k, L=64):
    """c0 * x0 + (c1 * x1 + (... + c_{k-1})): linear in its k constants, all started at 1"""
    nodes = []
    for j in range(k - 1):
        nodes += [(R.F_ADD, B, 0), (R.F_MUL, B, 3), (1.0, C, 1), (j, V, 1)]
    nodes.append((1.0, C, 1))
    n = len(nodes)
    nodes = [(v, t, n - i if (t == B and s == 0) else s) for i, (v, t, s) in enumerate(nodes)]
    return _row(nodes, L)


@pytest.mark.parametrize("k", [1, 2, 5, 8])
def test_linear_trees_reach_the_least_squares_loss(k):
    value, type_, size = _linear_tree(k)
    rng = np.random.default_rng(100 + k)
    X = rng.uniform(-1, 1, (200, 8)).astype(np.float32)
    y = (X[:, :3] @ np.array([2.5, -1.0, 0.5]) + 0.7 + 0.1 * rng.standard_normal(200)).astype(np.float32)[:, None]
    design = np.concatenate([X[:, :k - 1].astype(np.float64), np.ones((200, 1))], axis=1)
    coef = np.linalg.lstsq(design, y.astype(np.float64)[:, 0], rcond=None)[0]
    best = float(np.mean((design @ coef - y[:, 0]) ** 2))
    # in float64 state throughout: the reference's own arithmetic, without the float32 rounding of the stored constants
    v = value.astype(np.float64)[None, :]
    lam = 1e-3
    loss, normal, _ = LM.forest_normal_eq(v, type_[None], size[None], X, y)
    cidx = LM.optimised_consts(type_, size)[:k]
    for step in range(4):
        A, b = LM.unpack(normal[0])
        M = A[:k, :k] + lam * np.diag(np.diag(A[:k, :k]))
        cand = v.copy()
        cand[0, cidx] += np.linalg.solve(M, -b[:k])
        loss_c, normal_c, _ = LM.forest_normal_eq(cand, type_[None], size[None], X, y)
        assert loss_c[0] < loss[0] or loss[0] <= best * (1 + 1e-9)
        if loss_c[0] < loss[0]:
            v, loss, normal, lam = cand, loss_c, normal_c, max(lam / 10, 1e-10)
        else:
            lam = min(lam * 10, 1e10)
    assert loss[0] <= best * (1 + 1e-9), (loss[0], best)
    # and the float32-state loop (what the CPU kernels of the host tests run) gets as close as float32 constants allow
    v32, loss32, _ = LM.lm_optimize(value[None], type_[None], size[None], X, y, steps=4)
    assert loss32[0] <= np.float32(best) * (1 + 1e-5)


def test_step_leaves_degenerate_trees_where_they_are():
    normal = np.zeros(LM.WORDS)
    normal[0], normal[len(LM.TRI)] = 2.0, 1.0
    assert LM.solve_step(normal, 1e-3, 1.0, [0.5])[0] == np.float32(0.5 - 1.0 / (2.0 * 1.001))
    assert LM.solve_step(normal, 1e-3, 0.0, [0.5]) is None          # zero loss
    assert LM.solve_step(normal, 1e-3, np.nan, [0.5]) is None       # non-finite loss
    assert LM.solve_step(normal, 1e-3, 1.0, [3e38]) is not None
    big = normal.copy(); big[len(LM.TRI)] = -1e39
    assert LM.solve_step(big, 1e-3, 1.0, [3e38]) is None            # c + delta overflows float32
    bad = normal.copy(); bad[len(LM.TRI)] = np.inf
    assert LM.solve_step(bad, 1e-3, 1.0, [0.5]) is None             # non-finite b
    zero = np.zeros(LM.WORDS)
    assert LM.solve_step(zero, 1e-3, 1.0, [0.5]) is None            # no constant has any influence
    # a dropped constant keeps its value while the other one moves
    two = np.zeros(LM.WORDS); two[8] = 4.0; two[len(LM.TRI) + 1] = 2.0
    new = LM.solve_step(two, 0.0, 1.0, [7.0, 1.0])
    assert new[0] == np.float32(7.0) and new[1] == np.float32(0.5)
    # an indefinite matrix (no such J^T J exists; a rounding artefact at worst) has a pivot <= 0
    ind = np.zeros(LM.WORDS); ind[0], ind[1], ind[8] = 1.0, 2.0, 1.0; ind[len(LM.TRI)] = 1.0
    assert LM.solve_step(ind, 1e-3, 1.0, [0.0, 0.0]) is None


def test_gpu_cases_keep_half_of_their_trees_on_the_reference_alone(oracle):
    """the exclusion rule of tests/test_gpu_sr_lm.py's comparison, applied to its own cases without a GPU"""
    import lm_cases

    for funcs, gp_len, D, pop in [c + (lm_cases.POP,) for c in lm_cases.CASES] + [lm_cases.FILL_CASE + (lm_cases.FILL_DISTINCT,)]:
        value, type_, size, X, y = lm_cases.make_case(funcs, gp_len, D, pop)
        stable = lm_cases.comparable(oracle, value, type_, size, X, y)[3]
        assert stable.mean() >= 0.5, (funcs, gp_len, D, pop, int(stable.sum()))


# ---- the edge cells of the adjoint table, as the normal equations state them ---------------------------------------------------------
D9 = float(np.float32(1e-9))
NAN, INF = np.nan, np.inf
# (prefix nodes of f over CONST operands, loss, J per constant): one row, label 0, so A_ij = J_i J_j and b_i = J_i pred
EDGE_TREES = [
    ([(R.F_LOOSE_DIV, B, 3), (3.0, C, 1), (5e-10, C, 1)], (3 / D9) ** 2, [1 / D9, 0.0]),       # |b| <= delta: d = delta, db = 0
    ([(R.F_LOOSE_DIV, B, 3), (3.0, C, 1), (-0.0, C, 1)], (3 / D9) ** 2, [-1 / D9, 0.0]),       # the sign of the zero
    ([(R.F_LOOSE_DIV, B, 3), (3.0, C, 1), (D9, C, 1)], (3 / D9) ** 2, [1 / D9, 0.0]),          # <=, not <
    ([(R.F_DIV, B, 3), (1.0, C, 1), (0.0, C, 1)], NAN, [INF, NAN]),
    ([(R.F_MAX, B, 3), (1.0, C, 1), (1.0, C, 1)], 1.0, [1.0, 0.0]),                            # ties go to a
    ([(R.F_MIN, B, 3), (0.0, C, 1), (-0.0, C, 1)], 0.0, [1.0, 0.0]),
    ([(R.F_IF, T, 4), (0.0, C, 1), (2.0, C, 1), (3.0, C, 1)], 9.0, [0.0, 0.0, 1.0]),           # the condition gets nothing
    ([(R.F_IF, T, 4), (1e-45, C, 1), (2.0, C, 1), (3.0, C, 1)], 4.0, [0.0, 1.0, 0.0]),
    ([(R.F_LT, B, 3), (1.0, C, 1), (2.0, C, 1)], 1.0, [0.0, 0.0]),
    ([(40.0, B, 3), (1.0, C, 1), (2.0, C, 1)], 0.0, [0.0, 0.0]),                               # an unknown binary id
    ([(99.0, U, 2), (1.0, C, 1)], 0.0, [0.0]),                                                 # an unknown unary id
    ([(R.F_INV, U, 2), (0.0, C, 1)], NAN, [NAN]),
    ([(R.F_LOOSE_INV, U, 2), (1e-10, C, 1)], (1 / D9) ** 2, [0.0]),
    ([(R.F_LOG, U, 2), (-2.0, C, 1)], NAN, [-0.5]),
    ([(R.F_LOOSE_LOG, U, 2), (0.0, C, 1)], 1e18, [0.0]),
    ([(R.F_LOOSE_LOG, U, 2), (-2.0, C, 1)], np.log(2.0) ** 2, [-0.5]),
    ([(R.F_POW, B, 3), (-2.0, C, 1), (3.0, C, 1)], 64.0, [12.0, 0.0]),                         # a < 0: nothing to the exponent
    ([(R.F_POW, B, 3), (0.0, C, 1), (0.0, C, 1)], 1.0, [NAN, 0.0]),                            # 0 * pow(0, -1): the formula as written
    ([(R.F_LOOSE_POW, B, 3), (0.0, C, 1), (0.0, C, 1)], 0.0, [0.0, 0.0]),
    ([(R.F_LOOSE_POW, B, 3), (-2.0, C, 1), (3.0, C, 1)], 64.0, [-12.0, 8 * np.log(2.0)]),      # sign a; db is 0 only at |a| = 0
    ([(R.F_ABS, U, 2), (0.0, C, 1)], 0.0, [0.0]),
    ([(R.F_ABS, U, 2), (-3.0, C, 1)], 9.0, [-1.0]),
    ([(R.F_SQRT, U, 2), (0.0, C, 1)], 0.0, [INF]),
    ([(R.F_SQRT, U, 2), (-4.0, C, 1)], NAN, [NAN]),
    ([(R.F_LOOSE_SQRT, U, 2), (0.0, C, 1)], 0.0, [0.0]),
    ([(R.F_LOOSE_SQRT, U, 2), (-4.0, C, 1)], 4.0, [-0.25]),
]


@pytest.mark.parametrize("case", range(len(EDGE_TREES)))
def test_normal_equations_at_the_edge_cells_of_the_adjoint_table(case):
    nodes, want_loss, J = EDGE_TREES[case]
    value, type_, size = _row(nodes)
    with np.errstate(all="ignore"):
        loss, normal, _ = LM.tree_normal_eq(value, type_, size, np.zeros((1, 1), np.float32), np.zeros((1, 1), np.float32))
        pred, Jg, cidx = LM.tree_jacobian(value, type_, size, np.zeros((1, 1), np.float32))
        A, b = LM.unpack(normal)
        nc = len(J)
        J = np.array(J)
        np.testing.assert_allclose(loss, want_loss, rtol=1e-12)
        np.testing.assert_allclose(Jg[0, :nc], J, rtol=1e-12)
        np.testing.assert_allclose(A[:nc, :nc], np.outer(J, J), rtol=1e-12)   # a 0 of the table is a zero row and column, a NaN a NaN one
        np.testing.assert_allclose(b[:nc], J * pred[0], rtol=1e-12)
    assert np.all(A[nc:] == 0) and np.all(A[:, nc:] == 0) and np.all(b[nc:] == 0) and np.all(Jg[0, nc:] == 0)   # absent constants
    for j in range(nc):
        if J[j] == 0 and np.isfinite(J).all() and np.isfinite(pred[0]):
            assert np.all(A[j] == 0) and np.all(A[:, j] == 0) and b[j] == 0


def test_step_at_the_edge_cells():
    """a constant the table gives 0 is dropped and keeps its value while the other moves; a NaN cell stops the tree"""
    z = np.zeros((1, 1), np.float32)
    value, type_, size = _row([(R.F_LOOSE_DIV, B, 3), (3.0, C, 1), (5e-10, C, 1)])
    _, normal, _ = LM.tree_normal_eq(value, type_, size, z, z)
    new = LM.solve_step(normal, 1e-3, 1.0, [3.0, 5e-10])
    assert new is not None and new[1] == np.float32(5e-10) and new[0] != np.float32(3.0)
    for nodes, consts in (([(R.F_DIV, B, 3), (1.0, C, 1), (0.0, C, 1)], [1.0, 0.0]), ([(R.F_INV, U, 2), (0.0, C, 1)], [0.0]),
                          ([(R.F_POW, B, 3), (0.0, C, 1), (0.0, C, 1)], [0.0, 0.0])):
        value, type_, size = _row(nodes)
        with np.errstate(all="ignore"):
            _, normal, _ = LM.tree_normal_eq(value, type_, size, z, z)
        assert LM.solve_step(normal, 1e-3, 1.0, consts) is None
