"""CPU: the host logic of Levenberg-Marquardt constant optimisation (Forest.optimize_constants(method="lm"),
Forest.SR_normal_equations, SymbolicRegression(const_opt_method="lm"), StandardPipeline) with the float64 reference registered as a
test-only CPU kernel (tests/cpu_lm_ops.py), and the argument checks of the two C entry points, which return before any launch."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cpu_grad_ops  # noqa: E402
import cpu_lm_ops  # noqa: E402
import cpu_ops  # noqa: E402
import sr_grad_ref as R  # noqa: E402
import sr_lm_ref as LM  # noqa: E402
from grad_trees import ALL_FUNCS, ARITH, random_forest  # noqa: E402

cpu_ops.register()
cpu_grad_ops.register()
cpu_lm_ops.register()

from evogp_amd.tree import Forest, GenerateDescriptor, set_default_device  # noqa: E402
from evogp_amd.tree import utils as _tree_utils  # noqa: E402


@pytest.fixture(autouse=True)
def _cpu_default_device():
    saved = _tree_utils._DEVICE
    set_default_device("cpu")
    yield
    _tree_utils._DEVICE = saved


def _forest(rng, funcs, pop=60, out_len=1):
    value, type_, size = random_forest(rng, pop, 32, funcs, 2, out_len, max_depth=4)
    X = rng.uniform(-1, 1, (40, 2)).astype(np.float32)
    y = rng.uniform(-1, 1, (40, out_len)).astype(np.float32)
    return value, type_, size, X, y


def _comb(n_consts, L=32):
    """c0 + (c1 + (... + c_{n-1})) with constants 1, 2, ..."""
    value, type_, size = np.zeros(L, np.float32), np.zeros(L, np.int16), np.zeros(L, np.int16)
    n = 2 * n_consts - 1
    for k in range(n_consts - 1):
        value[2 * k], type_[2 * k], size[2 * k] = R.F_ADD, R.T_BFUNC, n - 2 * k
        value[2 * k + 1], type_[2 * k + 1], size[2 * k + 1] = k + 1, R.T_CONST, 1
    value[n - 1], type_[n - 1], size[n - 1] = n_consts, R.T_CONST, 1
    return value, type_, size


@pytest.mark.parametrize("funcs", ["arith", "all"])
def test_optimize_constants_lm_invariants(rng, funcs):
    value, type_, size, X, y = _forest(rng, ARITH if funcs == "arith" else ALL_FUNCS)
    size[3, 0] = 0                                   # malformed: NaN loss
    value[4, :3] = [R.F_ADD, 0, 1]                   # no constants: x0 + x1
    type_[4, :3] = [R.T_BFUNC, R.T_VAR, R.T_VAR]
    size[4, :3] = [3, 1, 1]
    value[5], type_[5], size[5] = _comb(11)          # 11 constants: the last three are held fixed
    f0 = Forest(2, 1, *(torch.from_numpy(a) for a in (value, type_, size)))
    keep = [a.clone() for a in f0._tensors()]
    Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
    before_calls = dict(cpu_lm_ops.calls)
    f1, loss = f0.optimize_constants(Xt, yt, steps=6, method="lm")
    assert cpu_lm_ops.calls["normal_eq"] - before_calls["normal_eq"] == 7 and cpu_lm_ops.calls["lm_step"] - before_calls["lm_step"] == 7
    for a, b in zip(keep, f0._tensors()):
        assert torch.equal(a, b)                     # the input forest is untouched
    with np.errstate(all="ignore"):
        before = R.forest_grad(value, type_, size, X, y)[0]
    after = loss.numpy()
    fin = np.isfinite(before)
    assert np.all(after[fin] <= before[fin].astype(np.float32))
    assert (after[fin] < before[fin].astype(np.float32)).mean() > 0.3
    v1, t1, s1 = (a.numpy() for a in f1._tensors())
    assert np.array_equal(t1, type_) and np.array_equal(s1, size)
    opt = np.zeros(value.shape, bool)                # the optimised constants: the first 8 of every live prefix
    for t in range(len(value)):
        c = LM.optimised_consts(type_[t], size[t])
        opt[t, c[c >= 0]] = True
    assert np.array_equal(v1.view(np.uint32)[~opt], value.view(np.uint32)[~opt])
    assert np.array_equal(v1[5, [17, 19, 20]], value[5, [17, 19, 20]]) and not np.array_equal(v1[5, :16], value[5, :16])
    for t in (3, 4):
        assert np.array_equal(v1[t].view(np.uint32), value[t].view(np.uint32))
    assert np.isnan(after[3])
    assert np.array_equal(v1.view(np.uint32)[~fin], value.view(np.uint32)[~fin])
    # the returned loss is the returned forest's loss
    with np.errstate(all="ignore"):
        again = R.forest_grad(v1, type_, size, X, y)[0].astype(np.float32)
    np.testing.assert_array_equal(after, again)
    assert f1.func_mask == f0.func_mask


def test_zero_steps_and_planted_problem_on_cpu_kernel():
    rng = np.random.default_rng(7)
    X = rng.uniform(-1, 1, (64, 1)).astype(np.float32)
    y = (2.5 * X + 0.7).astype(np.float32)
    value = np.array([[R.F_ADD, R.F_MUL, 1.0, 0, 1.0]], np.float32)
    type_ = np.array([[R.T_BFUNC, R.T_BFUNC, R.T_CONST, R.T_VAR, R.T_CONST]], np.int16)
    size = np.array([[5, 3, 1, 1, 1]], np.int16)
    f0 = Forest(1, 1, *(torch.from_numpy(a) for a in (value, type_, size)))
    Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
    f2, loss2 = f0.optimize_constants(Xt, yt, steps=0, method="lm")
    assert torch.equal(f2.batch_node_value, f0.batch_node_value)
    np.testing.assert_allclose(loss2.numpy(), R.forest_grad(value, type_, size, X, y)[0].astype(np.float32), rtol=1e-6)
    f1, loss = f0.optimize_constants(Xt, yt, steps=3, method="lm")
    c = f1.batch_node_value.numpy()[0]
    assert abs(c[2] - 2.5) <= 1e-3 and abs(c[4] - 0.7) <= 1e-3 and float(loss[0]) < 1e-5, (c, loss)
    # the descent is nowhere near after as many steps: the two methods are different paths
    fd, _ = f0.optimize_constants(Xt, yt, steps=3)
    assert abs(fd.batch_node_value.numpy()[0][2] - 2.5) > 0.1


def test_sr_normal_equations(rng):
    value, type_, size, X, y = _forest(rng, ARITH, pop=12)
    value[0], type_[0], size[0] = _comb(11)
    value[1, :3], type_[1, :3], size[1, :3] = [R.F_ADD, 0, 1], [R.T_BFUNC, R.T_VAR, R.T_VAR], [3, 1, 1]
    size[2, 0] = 0
    f = Forest(2, 1, *(torch.from_numpy(a) for a in (value, type_, size)))
    loss, A, b, cidx = f.SR_normal_equations(torch.from_numpy(X), torch.from_numpy(y))
    assert A.shape == (12, 8, 8) and b.shape == (12, 8) and cidx.shape == (12, 8) and cidx.dtype == torch.int64
    assert torch.equal(A, A.transpose(1, 2))
    want_loss, want, _ = LM.forest_normal_eq(value, type_, size, X, y)
    for t in range(12):
        np.testing.assert_array_equal(cidx[t].numpy(), LM.optimised_consts(type_[t], size[t]))
        Aw, bw = LM.unpack(want[t].astype(np.float32))
        np.testing.assert_array_equal(A[t].numpy(), Aw.astype(np.float32))
        np.testing.assert_array_equal(b[t].numpy(), bw.astype(np.float32))
    np.testing.assert_array_equal(loss.numpy(), want_loss.astype(np.float32))
    assert list(cidx[0]) == [1, 3, 5, 7, 9, 11, 13, 15] and torch.all(A[0] == 1) and torch.all(cidx[1] == -1) and torch.all(A[1] == 0)
    assert torch.isnan(loss[2]) and torch.all(A[2] == 0) and torch.all(b[2] == 0)
    multi = Forest(2, 3, *(torch.from_numpy(a) for a in (value, type_, size)))
    with pytest.raises(AssertionError):
        multi.SR_normal_equations(torch.from_numpy(X), torch.zeros(40, 3))


def test_value_errors(rng):
    value, type_, size, X, y = _forest(rng, ARITH, pop=8)
    f = Forest(2, 1, *(torch.from_numpy(a) for a in (value, type_, size)))
    Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
    with pytest.raises(ValueError):
        f.optimize_constants(Xt, yt, steps=2, use_MSE=False, method="lm")
    with pytest.raises(ValueError):
        f.optimize_constants(Xt, yt, steps=2, method="newton")
    value3, type3, size3, X3, y3 = _forest(rng, ARITH, pop=8, out_len=3)
    f3 = Forest(2, 3, *(torch.from_numpy(a) for a in (value3, type3, size3)))
    with pytest.raises(ValueError):
        f3.optimize_constants(torch.from_numpy(X3), torch.from_numpy(y3), steps=2, method="lm")
    f3.optimize_constants(torch.from_numpy(X3), torch.from_numpy(y3), steps=1)   # (the descent takes multi-output forests)


def test_default_method_takes_the_descent_path(rng):
    value, type_, size, X, y = _forest(rng, ALL_FUNCS, pop=30)
    f = Forest(2, 1, *(torch.from_numpy(a) for a in (value, type_, size)))
    Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
    lm_calls = dict(cpu_lm_ops.calls)
    f1, l1 = f.optimize_constants(Xt, yt, 4, 0.2)
    f2, l2 = f.optimize_constants(Xt, yt, 4, 0.2, True, method="descent", damping=5.0)
    assert cpu_lm_ops.calls == lm_calls             # no LM kernel ran
    assert torch.equal(f1.batch_node_value.view(torch.int32), f2.batch_node_value.view(torch.int32))
    assert torch.equal(l1.view(torch.int32), l2.view(torch.int32))
    # ... and it is the descent of the reference loop: gradient, propose, then {gradient, accept + propose}
    v = value.copy()
    with np.errstate(all="ignore"):
        g = lambda a: tuple(x.astype(np.float32) for x in R.forest_grad(a, type_, size, X, y)[:2])  # noqa: E731
        loss, grad = g(v)
        cand, step = np.empty_like(v), np.full(30, 0.2, np.float32)
        R.const_step(v, type_, size, cand, loss, grad, loss, grad, step, 1, 2)
        for k in range(4):
            lc, gc = g(cand)
            R.const_step(v, type_, size, cand, loss, grad, lc, gc, step, 1, 3 if k < 3 else 1)
    assert np.array_equal(f1.batch_node_value.numpy().view(np.uint32), v.view(np.uint32))


def test_pipeline_with_lm_constant_optimisation(rng):
    from evogp_amd.algorithm import DefaultCrossover, DefaultMutation, DefaultSelection, GeneticProgramming
    from evogp_amd.pipeline import StandardPipeline
    from evogp_amd.problem import SymbolicRegression

    d = GenerateDescriptor(max_tree_len=32, input_len=1, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=3,
                           const_samples=[-1, 0.5, 1])
    X = torch.from_numpy(rng.uniform(-1, 1, (32, 1)).astype(np.float32))
    y = 2.5 * X + 0.7
    prob = SymbolicRegression(datapoints=X, labels=y, execute_mode="auto", const_opt_steps=3, const_opt_method="lm")
    assert SymbolicRegression(datapoints=X, labels=y).const_opt_method == "descent"
    with pytest.raises(AssertionError):
        SymbolicRegression(datapoints=X, labels=y, const_opt_method="newton")
    algo = GeneticProgramming(Forest.random_generate(60, d, keys=torch.tensor([1, 2])), DefaultCrossover(),
                              DefaultMutation(0.2, d), DefaultSelection(0.3, 2))
    start = algo.forest
    pipe = StandardPipeline(algo, prob, generation_limit=2, is_show_details=False)
    lm_calls = dict(cpu_lm_ops.calls)
    optimised = prob.optimize(start)
    assert cpu_lm_ops.calls["normal_eq"] - lm_calls["normal_eq"] == 4
    want_forest, _ = start.optimize_constants(X, y, steps=3, method="lm")
    assert torch.equal(optimised.batch_node_value, want_forest.batch_node_value)
    host = pipe.step()
    # the first generation scored the optimised forest (the same deterministic tuning of the same trees)
    want = -optimised.SR_fitness(X, y)
    np.testing.assert_allclose(host.numpy(), torch.where(torch.isnan(want), torch.full_like(want, float("-inf")), want).numpy(), rtol=1e-5)
    best = int(torch.argmax(host))
    assert torch.equal(pipe.best_tree.node_value, optimised[best].node_value)
    pipe.step()


def test_argument_errors_without_gpu_and_abi():
    from evogp_amd import _lib

    L = _lib.lib
    assert L.evogp_hip_abi_version() == 9 == _lib.ABI_VERSION
    p = 8  # (never dereferenced: the host checks come first)
    ne = L.evogp_hip_sr_normal_eq
    assert ne(0, 8, 32, 3, 1, p, p, p, p, p, p, p, None) == -1
    assert ne(4, 0, 32, 3, 1, p, p, p, p, p, p, p, None) == -1
    assert ne(4, 8, 0, 3, 1, p, p, p, p, p, p, p, None) == -1
    assert ne(4, 8, 1025, 3, 1, p, p, p, p, p, p, p, None) == -1
    assert ne(4, 8, 32, 0, 1, p, p, p, p, p, p, p, None) == -1
    assert ne(4, 8, 32, 3, 2, p, p, p, p, p, p, p, None) == -1      # single-output only
    assert ne(4, 8, 32, 3, 0, p, p, p, p, p, p, p, None) == -1
    for k in range(7):
        ptrs = [p] * 7
        ptrs[k] = None
        assert ne(4, 8, 32, 3, 1, *ptrs, None) == -2
    st = L.evogp_hip_sr_lm_step
    assert st(0, 32, 1, 3, p, p, p, p, p, p, p, p, p, None) == -1
    assert st(4, 0, 1, 3, p, p, p, p, p, p, p, p, p, None) == -1
    assert st(4, 1025, 1, 3, p, p, p, p, p, p, p, p, p, None) == -1
    assert st(4, 32, 2, 3, p, p, p, p, p, p, p, p, p, None) == -1   # single-output only
    assert st(4, 32, 1, 0, p, p, p, p, p, p, p, p, p, None) == -1
    assert st(4, 32, 1, 4, p, p, p, p, p, p, p, p, p, None) == -1
    for k in (0, 1, 2, 3, 4, 5, 8):
        ptrs = [p] * 9
        ptrs[k] = None
        assert st(4, 32, 1, 3, *ptrs, None) == -2
    assert st(4, 32, 1, 1, p, p, p, p, p, p, None, p, p, None) == -2
    assert st(4, 32, 1, 3, p, p, p, p, p, p, p, None, p, None) == -2
    # (phase 2 with NULL candidates passes the checks and would launch: not called here)
