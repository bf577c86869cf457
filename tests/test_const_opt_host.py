"""CPU: the host logic of gradient-based constant optimisation (Forest.optimize_constants, SymbolicRegression.optimize,
StandardPipeline with const_opt_steps > 0) with the float64 reference registered as a test-only CPU kernel (tests/cpu_grad_ops.py),
and the argument checks of the two new C entry points, which return before any launch."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cpu_grad_ops  # noqa: E402
import cpu_ops  # noqa: E402
import sr_grad_ref as R  # noqa: E402
from grad_trees import ALL_FUNCS, ARITH, random_forest  # noqa: E402

cpu_ops.register()
cpu_grad_ops.register()

from evogp_amd.tree import Forest, GenerateDescriptor, set_default_device  # noqa: E402
from evogp_amd.tree import utils as _tree_utils  # noqa: E402


@pytest.fixture(autouse=True)
def _cpu_default_device():
    saved = _tree_utils._DEVICE
    set_default_device("cpu")
    yield
    _tree_utils._DEVICE = saved


def _forest(rng, funcs, out_len, pop=60):
    value, type_, size = random_forest(rng, pop, 32, funcs, 2, out_len, max_depth=4)
    X = rng.uniform(-1, 1, (40, 2)).astype(np.float32)
    y = rng.uniform(-1, 1, (40, out_len)).astype(np.float32)
    return value, type_, size, X, y


@pytest.mark.parametrize("funcs,out_len", [("arith", 1), ("all", 1), ("all", 3)])
def test_optimize_constants_invariants(rng, funcs, out_len):
    value, type_, size, X, y = _forest(rng, ARITH if funcs == "arith" else ALL_FUNCS, out_len)
    size[3, 0] = 0                                   # malformed: NaN loss
    value[4, :3] = [R.F_ADD, 0, 1]                   # no constants: x0 + x1
    type_[4, :3] = [R.T_BFUNC, R.T_VAR, R.T_VAR]
    size[4, :3] = [3, 1, 1]
    f0 = Forest(2, out_len, *(torch.from_numpy(a) for a in (value, type_, size)))
    keep = [a.clone() for a in f0._tensors()]
    Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
    f1, loss = f0.optimize_constants(Xt, yt, steps=6, step_size=0.2)
    for a, b in zip(keep, f0._tensors()):
        assert torch.equal(a, b)
    before = R.forest_grad(value, type_, size, X, y)[0]
    after = loss.numpy()
    fin = np.isfinite(before)
    assert np.all(after[fin] <= before[fin].astype(np.float32))
    assert (after[fin] < before[fin].astype(np.float32)).any()
    v1, t1, s1 = (a.numpy() for a in f1._tensors())
    assert np.array_equal(t1, type_) and np.array_equal(s1, size)
    multi = out_len > 1
    is_c = (((type_.astype(np.int32) & 0x7F) if multi else type_) == R.T_CONST) & (np.arange(32)[None, :] < np.clip(size[:, :1], 0, 32))
    assert np.array_equal(v1.view(np.uint32)[~is_c], value.view(np.uint32)[~is_c])
    for t in (3, 4):
        assert np.array_equal(v1[t].view(np.uint32), value[t].view(np.uint32))
    assert np.isnan(after[3])
    assert np.array_equal(v1.view(np.uint32)[~fin], value.view(np.uint32)[~fin])


def test_optimize_constants_planted_problem_on_cpu_kernel():
    rng = np.random.default_rng(7)
    X = rng.uniform(-1, 1, (64, 1)).astype(np.float32)
    y = (2.5 * X + 0.7).astype(np.float32)
    value = np.array([[R.F_ADD, R.F_MUL, 1.0, 0, 1.0]], np.float32)
    type_ = np.array([[R.T_BFUNC, R.T_BFUNC, R.T_CONST, R.T_VAR, R.T_CONST]], np.int16)
    size = np.array([[5, 3, 1, 1, 1]], np.int16)
    f1, loss = Forest(1, 1, *(torch.from_numpy(a) for a in (value, type_, size))).optimize_constants(
        torch.from_numpy(X), torch.from_numpy(y), steps=200, step_size=0.1)
    c = f1.batch_node_value.numpy()[0]
    assert abs(c[2] - 2.5) <= 1e-3 and abs(c[4] - 0.7) <= 1e-3, c


def test_func_mask_carried_and_zero_steps(rng):
    d = GenerateDescriptor(max_tree_len=32, input_len=2, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=4,
                           const_samples=[-1, 0.5, 1])
    f0 = Forest.random_generate(50, d, keys=torch.tensor([3, 4]))
    X = torch.from_numpy(rng.uniform(-1, 1, (30, 2)).astype(np.float32))
    y = X[:, :1] * 1.7 - 0.3
    f1, loss = f0.optimize_constants(X, y, steps=3)
    assert f1.func_mask == f0.func_mask != 0
    f2, loss2 = f0.optimize_constants(X, y, steps=0)
    assert torch.equal(f2.batch_node_value, f0.batch_node_value)
    want = R.forest_grad(*(a.numpy() for a in f0._tensors()), X.numpy(), y.numpy())[0]
    np.testing.assert_allclose(loss2.numpy(), want.astype(np.float32), rtol=1e-6, equal_nan=True)


def test_pipeline_with_constant_optimisation_reports_optimised_best_tree(rng):
    from evogp_amd.algorithm import DefaultCrossover, DefaultMutation, DefaultSelection, GeneticProgramming
    from evogp_amd.pipeline import StandardPipeline
    from evogp_amd.problem import SymbolicRegression

    d = GenerateDescriptor(max_tree_len=32, input_len=1, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=3,
                           const_samples=[-1, 0.5, 1])
    X = torch.from_numpy(rng.uniform(-1, 1, (32, 1)).astype(np.float32))
    y = 2.5 * X + 0.7
    prob = SymbolicRegression(datapoints=X, labels=y, execute_mode="auto", const_opt_steps=4, const_step_size=0.1)
    assert SymbolicRegression(datapoints=X, labels=y).const_opt_steps == 0
    algo = GeneticProgramming(Forest.random_generate(60, d, keys=torch.tensor([1, 2])), DefaultCrossover(),
                              DefaultMutation(0.2, d), DefaultSelection(0.3, 2))
    start = algo.forest
    pipe = StandardPipeline(algo, prob, generation_limit=2, is_show_details=False)
    optimised = prob.optimize(start)
    host = pipe.step()
    # the first generation scored the optimised forest (the same deterministic tuning of the same trees)
    want = -optimised.SR_fitness(X, y)
    np.testing.assert_allclose(host.numpy(), torch.where(torch.isnan(want), torch.full_like(want, float("-inf")), want).numpy(), rtol=1e-5)
    best = int(torch.argmax(host))
    assert torch.equal(pipe.best_tree.node_value, optimised[best].node_value)
    pipe.step()


def test_argument_errors_without_gpu():
    from evogp_amd import _lib

    L = _lib.lib
    p = 8  # (never dereferenced: the host checks come first)
    assert L.evogp_hip_sr_gradient(0, 8, 32, 3, 1, 1, p, p, p, p, p, p, p, None) == -1
    assert L.evogp_hip_sr_gradient(4, 0, 32, 3, 1, 1, p, p, p, p, p, p, p, None) == -1
    assert L.evogp_hip_sr_gradient(4, 8, 1025, 3, 1, 1, p, p, p, p, p, p, p, None) == -1
    assert L.evogp_hip_sr_gradient(4, 8, 32, 3, 1, 1, p, p, p, p, p, p, None, None) == -2
    assert L.evogp_hip_sr_gradient(4, 8, 32, 3, 17, 1, p, p, p, p, p, p, p, None) == -3
    assert L.evogp_hip_sr_const_step(4, 32, 1, 4, p, p, p, p, p, p, p, p, p, None) == -1
    assert L.evogp_hip_sr_const_step(4, 32, 1, 1, p, p, p, p, p, p, None, p, p, None) == -2
