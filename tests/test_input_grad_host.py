"""CPU: the input gradients on the data (csrc/sr_xgrad.hip) above the kernel -- the float64 restatement (tests/input_grad_ref.py) on
hand-written trees with known derivatives, the host logic of Forest.SR_input_gradients / SR_derivative_loss and of
SymbolicRegression(derivative_labels=, derivative_wrt=, derivative_weight=, sampled_monotonic=) with the restatement registered as a
test-only CPU kernel (tests/cpu_xgrad_ops.py), and the forest invariants (dead words, row order, slices) of the two ops on it.
Importing this module also puts the two ops into the invariance and binding tables (tests/xgrad_tables.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cpu_interval_ops  # noqa: E402
import cpu_derivative_ops  # noqa: E402
import cpu_ops  # noqa: E402
import cpu_xgrad_ops  # noqa: E402
import forest_invariance as FI  # noqa: E402
import input_grad_ref as XR  # noqa: E402
import sr_grad_ref as R  # noqa: E402
import xgrad_tables as XT  # noqa: E402
from interval_cases import B, C, IF, U, V, rows  # noqa: E402

cpu_ops.register()
cpu_interval_ops.register()
cpu_derivative_ops.register()
cpu_xgrad_ops.register()

from evogp_amd.problem import SymbolicRegression  # noqa: E402
from evogp_amd.tree import Forest, set_default_device  # noqa: E402
from evogp_amd.tree import utils as _tree_utils  # noqa: E402

POP, D = 40, 50   # as tests/test_forest_invariance_host.py: the per-tree numpy loops stay within seconds per op


@pytest.fixture(autouse=True)
def _cpu_default_device():
    saved = _tree_utils._DEVICE
    set_default_device("cpu")
    yield
    _tree_utils._DEVICE = saved


# ---- the invariants of the two ops on the CPU stand-ins ------------------------------------------------------------------------------
@pytest.mark.parametrize("op,case", [(op, c) for op in (XT.GRAD, XT.LOSS) for c in FI.cases_for(op)])
def test_cpu_stand_in_keeps_the_invariants(op, case):
    FI.check(op, FI.TABLE[op], FI.build_case(case, min(POP, FI.CASES[case]["pop"]), D), "cpu")


def test_the_ops_are_in_both_tables():
    assert FI.cases_for(XT.GRAD) == FI.cases_for(XT.LOSS) == ["arith_L64", "all_L64_v13", "all_L1024_v40"]
    assert XT.GRAD in XT.BC.TABLE and XT.LOSS in XT.BC.TABLE


# ---- hand-written trees with known derivatives ---------------------------------------------------------------------------------------
def _x(rng, n=33, var_len=2):
    return rng.uniform(0.5, 1.5, (n, var_len))


def _xg(expr, X, wrt, L=16):
    value, type_, size = rows([expr], L)
    pred, d, scale = XR.forest_xgrad(value, type_, size, X, wrt)
    return pred[0], d[:, 0], scale[:, 0]


def test_known_derivatives(rng):
    X = _x(rng)
    x0, x1 = X[:, 0], X[:, 1]
    pred, d, scale = _xg(B(R.F_MUL, V(0), V(0)), X, [0, 1])
    assert np.array_equal(pred, x0 * x0) and np.array_equal(d[0], 2 * x0) and np.array_equal(scale[0], 2 * x0)
    assert np.array_equal(d[1], np.zeros_like(x0)) and not np.signbit(d[1]).any() and np.array_equal(scale[1], np.zeros_like(x0))
    pred, d, _ = _xg(B(R.F_DIV, V(0), V(1)), X, [1, 0])   # (wrt not in order: column 0 is x1)
    np.testing.assert_allclose(d[1], 1 / x1, rtol=1e-15)
    np.testing.assert_allclose(d[0], -x0 / x1 ** 2, rtol=1e-15)
    pred, d, _ = _xg(U(R.F_SIN, B(R.F_MUL, V(0), V(1))), X, [0, 1])
    np.testing.assert_allclose(d[0], np.cos(x0 * x1) * x1, rtol=1e-15)
    np.testing.assert_allclose(d[1], np.cos(x0 * x1) * x0, rtol=1e-15)
    pred, d, scale = _xg(V(1), X, [0, 1])   # a VAR root
    assert np.array_equal(pred, x1) and np.array_equal(d[0], 0 * x0) and np.array_equal(d[1], np.ones_like(x0)) and np.array_equal(scale[1], d[1])
    pred, d, scale = _xg(C(2.5), X, [0, 1])   # a CONST-only tree: +0.0
    assert np.array_equal(pred, np.full(len(X), 2.5)) and not d.any() and not np.signbit(d).any() and not scale.any()


def test_if_max_and_a_variable_that_occurs_five_times(rng):
    X = _x(rng) - 1.0   # x0 - 1 in (-0.5, 0.5): both branches are taken
    x0, x1 = X[:, 0], X[:, 1]
    pred, d, _ = _xg(IF(V(0), B(R.F_MUL, V(0), V(1)), U(R.F_NEG, V(1))), X, [0, 1])   # x0 > 0 ? x0 x1 : -x1
    take = x0 > 0
    assert np.array_equal(pred, np.where(take, x0 * x1, -x1))
    assert np.array_equal(d[0], np.where(take, x1, 0.0)) and np.array_equal(d[1], np.where(take, x0, -1.0))   # nothing through the condition
    pred, d, _ = _xg(B(R.F_MAX, V(0), B(R.F_MUL, C(2.0), V(1))), X, [0, 1])
    first = x0 >= 2 * x1
    assert np.array_equal(d[0], np.where(first, 1.0, 0.0)) and np.array_equal(d[1], np.where(first, 0.0, 2.0))
    # x0 * x0 + x0 * x1 - x0 / (x1 + 2) + x0: five occurrences of x0
    e = B(R.F_ADD, B(R.F_SUB, B(R.F_ADD, B(R.F_MUL, V(0), V(0)), B(R.F_MUL, V(0), V(1))), B(R.F_DIV, V(0), B(R.F_ADD, V(1), C(2.0)))), V(0))
    pred, d, scale = _xg(e, X, [0], L=32)
    np.testing.assert_allclose(d[0], 2 * x0 + x1 - 1 / (x1 + 2) + 1, rtol=1e-14, atol=1e-15)
    np.testing.assert_allclose(scale[0], 2 * np.abs(x0) + np.abs(x1) + 1 / (x1 + 2) + 1, rtol=1e-14)


def test_nan_rules_of_the_restatement(rng):
    X = _x(rng, 8)
    X[0, 0] = 0.0
    # sqrt(x0) at x0 == 0: the prediction is 0, the derivative inf
    pred, d, _ = _xg(U(R.F_SQRT, V(0)), X, [0])
    assert pred[0] == 0.0 and np.isposinf(d[0, 0]) and np.isfinite(d[0, 1:]).all()
    # x0 / (x1 - x1): a NaN prediction; the adjoint rule of / gives g / b = inf to the numerator and -g r / b = NaN to the divisor
    pred, d, _ = _xg(B(R.F_DIV, V(0), B(R.F_SUB, V(1), V(1))), X, [0, 1])
    assert np.isnan(pred).all() and np.isposinf(d[0]).all() and np.isnan(d[1]).all()
    # IF(1, x0, log(-1) * x1): the untaken branch holds a NaN value; its 0 adjoint times a NaN partial is NaN in x1, finite in x0
    e = IF(C(1.0), V(0), B(R.F_MUL, U(R.F_LOG, C(-1.0)), V(1)))
    pred, d, _ = _xg(e, X, [0, 1])
    assert np.array_equal(pred, X[:, 0]) and np.array_equal(d[0], np.ones(8)) and np.isnan(d[1]).all()
    # malformed rows: NaN everywhere
    value, type_, size = rows([B(R.F_ADD, V(0), V(1))], 8)
    size[0, 0] = 2
    pred, d, scale = XR.forest_xgrad(value, type_, size, X, [0])
    assert np.isnan(pred).all() and np.isnan(d).all() and np.isnan(scale).all()
    loss, viol = XR.derivative_loss(value, type_, size, X, X[:, :1], None, [0])
    assert np.isnan(loss).all() and (viol == len(X)).all()


def test_the_jitter_rule_keeps_well_conditioned_entries_and_drops_a_pole(rng):
    X = _x(rng, 64).astype(np.float32).astype(np.float64)
    good = B(R.F_ADD, B(R.F_MUL, V(0), V(1)), U(R.F_EXP, V(0)))
    # tan(1.5707963 + 1e-7 x0) is within 1e-7 of its pole: three ulps on the sum move the argument by 2.8e-7, so the rule drops d / d x0;
    # x1 does not occur: its derivative is 0 under every draw and stays
    value, type_, size = rows([good, U(R.F_TAN, B(R.F_ADD, C(1.5707963), B(R.F_MUL, C(1e-7), V(0))))], 16)
    ok = XR.comparable(value, type_, size, X, [0, 1])
    assert ok[:, 0].all() and not ok[0, 1].any() and ok[1, 1].all()


# ---- Forest --------------------------------------------------------------------------------------------------------------------------
EXPRS = [B(R.F_MUL, V(0), V(0)), B(R.F_DIV, V(0), V(1)), B(R.F_MUL, V(0), V(1)), V(1), C(2.5), B(R.F_SUB, V(1), B(R.F_MUL, C(2.0), V(0))),
         U(R.F_SQRT, V(0))]


def _forest(exprs=EXPRS, L=16, var_len=2):
    return Forest(var_len, 1, *(torch.from_numpy(a) for a in rows(exprs, L)))


def _data(rng, n=40, var_len=2):
    X = rng.uniform(0.5, 1.5, (n, var_len)).astype(np.float32)
    y = (X[:, :1] ** 2 + np.sin(X[:, 1:2])).astype(np.float32)
    dy = np.stack([2 * X[:, 0], np.cos(X[:, 1])], 1).astype(np.float32)
    return torch.from_numpy(X), torch.from_numpy(y), torch.from_numpy(dy)


def test_forest_input_gradients_shapes_wrt_and_errors(rng):
    forest = _forest()
    X, y, dy = _data(rng)
    pred, grad = forest.SR_input_gradients(X)
    assert pred.shape == (7, 40) and grad.shape == (7, 40, 2) and pred.dtype == grad.dtype == torch.float32
    assert grad.stride() == (40, 1, 7 * 40)   # a permuted view of the kernel's (V, pop, D) array
    x0 = X[:, 0].numpy()
    np.testing.assert_allclose(grad[0, :, 0].numpy(), 2 * x0, rtol=1e-6)
    assert not grad[0, :, 1].numpy().any() and torch.equal(grad[3, :, 1], torch.ones(40)) and not grad[4].numpy().any()
    swapped = forest.SR_input_gradients(X, wrt=[1, 0])[1]
    assert torch.equal(swapped[:, :, 0], grad[:, :, 1]) and torch.equal(swapped[:, :, 1], grad[:, :, 0])
    assert torch.equal(forest.SR_input_gradients(X, wrt=1)[1][:, :, 0], grad[:, :, 1])
    assert torch.equal(forest.SR_input_gradients(X, wrt=torch.tensor([0]))[1][:, :, 0], grad[:, :, 0])
    for wrt in ([2], [-1], [], [0, 0]):
        with pytest.raises(ValueError, match="wrt"):
            forest.SR_input_gradients(X, wrt=wrt)
    wide = Forest(9, 1, *forest._tensors())
    X9 = torch.from_numpy(rng.uniform(0.5, 1.5, (40, 9)).astype(np.float32))
    with pytest.raises(ValueError, match="at most 8"):
        wide.SR_input_gradients(X9)
    with pytest.raises(ValueError, match="at most 8"):
        wide.SR_input_gradients(X9, wrt=list(range(9)))
    assert wide.SR_input_gradients(X9, wrt=[8, 0, 3])[1].shape == (7, 40, 3)
    multi = Forest(2, 2, *forest._tensors())
    with pytest.raises(ValueError, match="single-output"):
        multi.SR_input_gradients(X)
    with pytest.raises(ValueError, match="single-output"):
        multi.SR_derivative_loss(X, torch.cat([y, y], 1))


def test_forest_derivative_loss_bounds_and_labels(rng):
    forest = _forest()
    X, y, dy = _data(rng)
    n0 = cpu_xgrad_ops.calls["derivative_loss"]
    loss, viol = forest.SR_derivative_loss(X, y, dy)
    assert cpu_xgrad_ops.calls["derivative_loss"] == n0 + 1   # one call of the op
    assert loss.shape == (7, 3) and loss.dtype == torch.float32 and viol.shape == (7, 2) and viol.dtype == torch.int32
    pred, grad = forest.SR_input_gradients(X)
    want = ((grad.double() - dy.double()[None]) ** 2).mean(1)
    np.testing.assert_allclose(loss[:, 1:].numpy(), want.numpy(), rtol=1e-6)
    np.testing.assert_allclose(loss[:, 0].numpy(), ((pred.double() - y.double()[:, 0][None]) ** 2).mean(1).numpy(), rtol=1e-6)
    assert not viol.numpy().any()   # no bounds: only NaN rows count, and there are none
    # dlabels=None is labels of zero: the mean squared sensitivity
    a, b = forest.SR_derivative_loss(X, y), forest.SR_derivative_loss(X, y, torch.zeros_like(dy))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    np.testing.assert_allclose(a[0][:, 1:].numpy(), (grad.double() ** 2).mean(1).numpy(), rtol=1e-6)
    # bounds: +1 | -1 | (dmin, dmax); x1 - 2 x0 (tree 5) falls in x0 with slope -2
    loss, viol = forest.SR_derivative_loss(X, y, wrt=[0], bounds={0: +1})
    assert viol.shape == (7, 1) and viol[:, 0].tolist() == [0, 0, 0, 0, 0, 40, 0]
    loss, viol = forest.SR_derivative_loss(X, y, wrt=[0], bounds={0: -1})
    assert viol[:, 0].tolist() == [40, 40, 40, 0, 0, 0, 40]
    loss, viol = forest.SR_derivative_loss(X, y, wrt=[0], bounds={0: (-2.0, 0.0)})
    assert viol[5, 0] == 0 and viol[3, 0] == 0 and viol[0, 0] == 40
    # a variable of bounds that wrt lacks is appended; the columns follow wrt, then the appended ones
    loss, viol = forest.SR_derivative_loss(X, y, wrt=[1], bounds={0: +1})
    assert loss.shape == (7, 3) and viol.shape == (7, 2) and viol[:, 1].tolist() == [0, 0, 0, 0, 0, 40, 0] and not viol[:, 0].numpy().any()
    with pytest.raises(ValueError, match="dlabels"):
        forest.SR_derivative_loss(X, y, dy, wrt=[1])   # two label columns for one variable
    with pytest.raises(ValueError, match="monotonic constraint"):
        forest.SR_derivative_loss(X, y, bounds={0: 2})
    with pytest.raises(ValueError, match="wrt"):
        forest.SR_derivative_loss(X, y, bounds={5: +1})
    # sqrt(x0) with a row at x0 == 0: the derivative is inf there -- its column is NaN, column 0 stays finite, and inf violates every bound but +1's
    X0 = X.clone()
    X0[3, 0] = 0.0
    loss, viol = forest.SR_derivative_loss(X0, y, wrt=[0], bounds={0: (0.0, 100.0)})
    assert torch.isfinite(loss[6, 0]) and torch.isnan(loss[6, 1]) and viol[6, 0] == 1


# ---- SymbolicRegression --------------------------------------------------------------------------------------------------------------
def _problem(rng, **kw):
    X, y, dy = _data(rng)
    return SymbolicRegression(datapoints=X, labels=y, **kw), X, y, dy


def test_scores_compose_the_weights_and_the_mask(rng):
    forest = _forest()
    X, y, dy = _data(rng)
    prob = SymbolicRegression(datapoints=X, labels=y, derivative_labels=dy, derivative_weight=[0.5, 2.0])
    loss, viol = prob.derivative_loss(forest)
    assert loss.shape == (7, 3) and viol.shape == (7, 2)
    want = -(loss[:, 0] + (0.5 * loss[:, 1] + 2.0 * loss[:, 2]))
    assert torch.equal(prob.scores(forest), want) and torch.equal(prob.evaluate(forest), want)
    one = SymbolicRegression(datapoints=X, labels=y, derivative_labels=dy[:, 1:], derivative_wrt=1, derivative_weight=3.0)
    l1, _ = one.derivative_loss(forest)
    assert torch.equal(l1[:, 1], loss[:, 2]) and torch.equal(one.scores(forest), -(l1[:, 0] + 3.0 * l1[:, 1]))
    with pytest.raises(ValueError, match="use_MSE"):
        prob.scores(forest, use_MSE=False)
    # with a sampled constraint: the trees with a violating row are at -inf / NaN, the others keep their bits; x0 is appended behind x1
    n0 = cpu_xgrad_ops.calls["derivative_loss"]
    both = SymbolicRegression(datapoints=X, labels=y, derivative_labels=dy[:, 1:], derivative_wrt=[1], derivative_weight=3.0,
                              sampled_monotonic={0: +1})
    s = both.scores(forest)
    assert cpu_xgrad_ops.calls["derivative_loss"] == n0 + 1   # the loss and the mask come from ONE pass
    lb, vb = both.derivative_loss(forest)
    assert lb.shape == (7, 3) and vb[:, 1].tolist() == [0, 0, 0, 0, 0, 40, 0]
    assert s[5] == float("-inf") and torch.equal(s[[0, 1, 2, 3, 4, 6]], one.scores(forest)[[0, 1, 2, 3, 4, 6]])
    e = both.evaluate(forest)
    assert torch.isnan(e[5]) and torch.equal(e[[0, 1, 2, 3, 4, 6]], s[[0, 1, 2, 3, 4, 6]])


def test_sampled_monotonic_alone_only_masks(rng):
    forest = _forest()
    X, y, dy = _data(rng)
    plain = SymbolicRegression(datapoints=X, labels=y)
    prob = SymbolicRegression(datapoints=X, labels=y, sampled_monotonic={0: -1})
    s, p = prob.scores(forest), plain.scores(forest)
    falls = [3, 4, 5]   # x1, 2.5 and x1 - 2 x0 do not rise in x0
    assert torch.equal(s[falls], p[falls]) and (s[[0, 1, 2, 6]] == float("-inf")).all()
    assert prob.derivative_loss(forest)[1].shape == (7, 1) and prob.sampled_monotonic == {0: -1}
    rng2 = SymbolicRegression(datapoints=X, labels=y, sampled_monotonic={0: (-2.5, 0.5), 1: +1})
    assert rng2.sampled_monotonic == {0: (-2.5, 0.5), 1: 1} and rng2._deriv_wrt == [0, 1]
    # composes with the interval proof: both masks apply
    boxed = SymbolicRegression(datapoints=X, labels=y, sampled_monotonic={0: -1}, monotonic={1: +1})
    sb = boxed.scores(forest)
    assert (sb[[0, 1, 2, 6]] == float("-inf")).all() and sb[3] == p[3]
    with pytest.raises(ValueError, match="neither"):
        plain.derivative_loss(forest)


def test_constructor_errors(rng):
    X, y, dy = _data(rng)
    kw = dict(datapoints=X, labels=y, derivative_labels=dy)
    w = torch.ones(40)
    for extra, text in ((dict(linear_scaling=True), "linear_scaling"), (dict(loss="huber", loss_param=1.0), "loss"),
                        (dict(sample_weights=w), "sample_weights"), (dict(validation_mask=torch.arange(40) < 10), "validation_mask"),
                        (dict(const_opt_steps=2), "const_opt_steps"), (dict(simplify_every=2), "simplify_every")):
        with pytest.raises(ValueError, match="derivative_labels cannot be combined with.*" + text):
            SymbolicRegression(**kw, **extra)
    with pytest.raises(ValueError, match="derivative_labels cannot be combined with multigene"):
        SymbolicRegression(datapoints=X, labels=y, derivative_labels=dy, multigene=True)
    with pytest.raises(ValueError, match="multigene cannot be combined with sampled_monotonic"):
        SymbolicRegression(datapoints=X, labels=y, multigene=True, sampled_monotonic={0: +1})
    two = torch.cat([y, y], 1)
    with pytest.raises(ValueError, match="derivative_labels works on one label column"):
        SymbolicRegression(datapoints=X, labels=two, derivative_labels=dy)
    with pytest.raises(ValueError, match="sampled_monotonic works on single-output"):
        SymbolicRegression(datapoints=X, labels=two, sampled_monotonic={0: +1})
    for bad in (dy[:, :1], dy[:10], dy.long(), dy.numpy()):
        with pytest.raises(ValueError, match="derivative_labels should be"):
            SymbolicRegression(datapoints=X, labels=y, derivative_labels=bad)
    for wrt in ([0, 0], [2], [], [-1]):
        with pytest.raises(ValueError, match="derivative_wrt should name distinct"):
            SymbolicRegression(datapoints=X, labels=y, derivative_labels=dy[:, :len(wrt) or 1], derivative_wrt=wrt)
    with pytest.raises(ValueError, match="derivative_wrt needs derivative_labels"):
        SymbolicRegression(datapoints=X, labels=y, derivative_wrt=[0])
    for lam in (-1.0, float("nan"), [1.0, 2.0, 3.0], float("inf")):
        with pytest.raises(ValueError, match="derivative_weight should be"):
            SymbolicRegression(datapoints=X, labels=y, derivative_labels=dy, derivative_weight=lam)
    for c in ({0: 2}, {0: (1.0, 0.0)}, {2: +1}, {}):
        with pytest.raises(ValueError, match="monotonic"):
            SymbolicRegression(datapoints=X, labels=y, sampled_monotonic=c)
    X9 = torch.from_numpy(rng.uniform(0.5, 1.5, (40, 9)).astype(np.float32))
    with pytest.raises(ValueError, match="at most 8"):
        SymbolicRegression(datapoints=X9, labels=y, derivative_labels=torch.zeros(40, 9))
    with pytest.raises(ValueError, match="at most 8"):
        SymbolicRegression(datapoints=X9, labels=y, derivative_labels=torch.zeros(40, 8), derivative_wrt=list(range(8)), sampled_monotonic={8: +1})
    ok = SymbolicRegression(datapoints=X9, labels=y, sampled_monotonic={8: +1})   # alone: only its own variables are asked for
    assert ok._deriv_wrt == [8]


def test_c_abi_argument_checks_return_before_any_launch():
    """bad sizes and wrt entries: EVOGP_E_BADARG (-1); null pointers: -2; out_len != 1: -3 -- nothing is dereferenced, so the stale pointers
    of this test are never read"""
    import ctypes as C
    from evogp_amd import _lib
    L = _lib.lib
    p = C.c_void_p(64)   # (never dereferenced: every call below fails its checks)

    def wrt(*v):
        return (C.c_int * max(len(v), 1))(*v)

    def grad(pop=4, D=8, gp_len=8, var_len=2, out_len=1, n=1, w=wrt(0), value=p, pred=p):
        return L.evogp_hip_sr_input_gradient(pop, D, gp_len, var_len, out_len, value, p, p, p, n, w, pred, p, None)

    def loss(pop=4, D=8, gp_len=8, var_len=2, out_len=1, n=1, w=wrt(0), labels=p, viol=p):
        return L.evogp_hip_sr_derivative_loss(pop, D, gp_len, var_len, out_len, p, p, p, p, labels, None, n, w, None, None, p, viol, None)

    for f in (grad, loss):
        for bad in (dict(pop=0), dict(D=0), dict(gp_len=0), dict(gp_len=1025), dict(var_len=0), dict(out_len=0), dict(n=0), dict(n=9, w=wrt(*range(9))),
                    dict(w=wrt(2)), dict(w=wrt(-1)), dict(n=2, w=wrt(1, 1))):
            assert f(**bad) == -1, (f.__name__, bad)
        assert f(w=None) == -2
        assert f(out_len=2) == -3
    assert grad(value=None) == -2 and grad(pred=None) == -2 and loss(labels=None) == -2 and loss(viol=None) == -2
    assert grad(out_len=2, value=None) == -2   # (the order of evogp_hip_sr_gradient: bad argument, null pointer, out_len)
