"""GPU: the constant-gradient kernel (csrc/sr_grad.hip) against the float64 reference (tests/sr_grad_ref.py), its loss against
tree_SR_fitness's tolerances, its output layout and determinism, and Forest.optimize_constants on the device."""
import os
import sys

import numpy as np
import pytest
import torch

import evogp_amd  # noqa: F401  (registers the ops)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sr_grad_ref as R  # noqa: E402
from grad_trees import ALL_FUNCS, ARITH, random_forest  # noqa: E402
from helpers import assert_within_sensitivity, per_tree_tolerance  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _grad(value, type_, size, X, y, use_mse=True):
    v, t, s, Xd, yd = _dev(value, type_, size, X, y)
    pop, L = value.shape
    loss, grad = torch.ops.evogp_hip.tree_SR_gradient(pop, X.shape[0], L, X.shape[1], y.shape[1], use_mse, v, t, s, Xd, yd)
    return loss.cpu().numpy(), grad.cpu().numpy()


def _case(rng, funcs, out_len, gp_len, D, pop=24, var_len=3):
    value, type_, size = random_forest(rng, pop, gp_len, ARITH if funcs == "arith" else ALL_FUNCS, var_len, out_len, max_depth=5)
    X = rng.uniform(0.5, 1.5, (D, var_len)).astype(np.float32)
    y = rng.uniform(-1, 1, (D, out_len)).astype(np.float32)
    return value, type_, size, X, y


@pytest.mark.parametrize("D", [1, 63, 1024, 5000])
@pytest.mark.parametrize("gp_len", [64, 1024])
@pytest.mark.parametrize("out_len", [1, 3])
@pytest.mark.parametrize("funcs", ["arith", "all"])
def test_gradient_matches_float64_reference(rng, oracle, funcs, out_len, gp_len, D):
    value, type_, size, X, y = _case(rng, funcs, out_len, gp_len, D)
    for use_mse in (True, False):
        loss, grad = _grad(value, type_, size, X, y, use_mse)
        want_loss, want, gabs = R.forest_grad(value, type_, size, X, y, use_mse)
        # Exclusion rule: a tree is compared when its float64 loss is finite, its fp32 loss is ulp-stable -- a 3-ulp nudge of every
        # library result (the oracle's sensitivity probe) moves it by at most 1e-4 relative -- and its float64 gradient is well
        # conditioned at fp32 resolution: nudging every constant and input by a relative 2^-22 (two draws of random signs) moves no
        # entry by more than 1e-4 of its scale.  Within it, every entry whose float64 gradient and scale are finite.
        _, tol, unstable = per_tree_tolerance(oracle, (value, type_, size), X, y, use_mse=use_mse)
        with np.errstate(all="ignore"):
            stable = np.isfinite(want_loss) & ~unstable & (tol <= 1e-4 * np.abs(want_loss) + 1e-6)
            is_c = (type_.astype(np.int32) & 0x7F) == R.T_CONST
            for k in range(2):
                jr = np.random.default_rng(k)
                vj = np.where(is_c, value * (1 + 2.0 ** -22 * jr.choice([-1, 1], value.shape)), value).astype(np.float32)
                Xj = X.astype(np.float64) * (1 + 2.0 ** -22 * jr.choice([-1, 1], X.shape))
                _, gj, _ = R.forest_grad(vj, type_, size, Xj, y, use_mse)
                moved = np.abs(gj - want) > 1e-4 * gabs + 1e-9
                stable &= ~np.any(np.where(np.isfinite(want) & np.isfinite(gabs), moved | ~np.isfinite(gj), False), axis=1)
        assert stable.mean() >= 0.5, f"only {stable.sum()} of {len(stable)} trees are comparable"
        for t in np.flatnonzero(stable):
            ok = np.isfinite(want[t]) & np.isfinite(gabs[t])
            err = np.abs(grad[t][ok].astype(np.float64) - want[t][ok])
            bound = 1e-3 * gabs[t][ok] + 1e-7
            assert (err <= bound).all(), (t, np.flatnonzero(ok)[np.argmax(err - bound)], grad[t][ok][np.argmax(err - bound)],
                                          want[t][ok][np.argmax(err - bound)])
            assert np.isfinite(loss[t]) and abs(loss[t] - want_loss[t]) <= 1e-4 * abs(want_loss[t]) + 1e-6


@pytest.mark.parametrize("funcs,out_len", [("arith", 1), ("all", 1), ("all", 4)])
def test_loss_agrees_with_sr_fitness(rng, oracle, funcs, out_len):
    value, type_, size, X, y = _case(rng, funcs, out_len, 64, 300, pop=200)
    loss, _ = _grad(value, type_, size, X, y)
    want, tol, unstable = per_tree_tolerance(oracle, (value, type_, size), X, y)
    assert_within_sensitivity(loss, want, tol, unstable, "tree_SR_gradient loss")
    v, t, s, Xd, yd = _dev(value, type_, size, X, y)
    fit = torch.ops.evogp_cuda.tree_SR_fitness(200, 300, 64, 3, out_len, True, v, t, s, Xd, yd, 4).cpu().numpy()
    assert_within_sensitivity(loss, fit.astype(np.float64), tol, unstable, "loss vs tree_SR_fitness")


@pytest.mark.parametrize("gp_len,out_len", [(64, 1), (1024, 1), (64, 5)])
def test_layout_determinism_and_malformed_trees(rng, gp_len, out_len):
    value, type_, size, X, y = _case(rng, "all", out_len, gp_len, 777, pop=300)
    type_[7, :] = R.T_CONST          # 64 leaves, size says 1..: not one value on the stack at the end
    size[7, 0] = 5
    size[9, 0] = 0                   # empty tree
    value[11, 0], type_[11, 0] = R.F_ADD, R.T_BFUNC   # the root now pops a missing operand
    size[11, 0] = 1
    loss, grad = _grad(value, type_, size, X, y)
    loss2, grad2 = _grad(value, type_, size, X, y)
    assert np.array_equal(loss.view(np.uint32), loss2.view(np.uint32)) and np.array_equal(grad.view(np.uint32), grad2.view(np.uint32))
    multi = out_len > 1
    for t in range(300):
        n = min(max(int(size[t, 0]), 0), gp_len)
        ty = type_[t].astype(np.int32)
        is_c = ((ty & 0x7F) if multi else ty) == R.T_CONST
        is_c[n:] = False
        assert np.all(grad[t][~is_c].view(np.uint32) == 0)
    for t in (7, 9, 11):
        assert np.isnan(loss[t]) and np.all(grad[t].view(np.uint32) == 0)


def test_argument_errors_without_launch():
    from evogp_amd import _lib

    L = _lib.lib
    p = 8  # (never dereferenced: the checks come first)
    assert L.evogp_hip_sr_gradient(0, 8, 32, 3, 1, 1, p, p, p, p, p, p, p, None) == -1
    assert L.evogp_hip_sr_gradient(4, 8, 2000, 3, 1, 1, p, p, p, p, p, p, p, None) == -1
    assert L.evogp_hip_sr_gradient(4, 8, 32, 3, 1, 1, None, p, p, p, p, p, p, None) == -2
    assert L.evogp_hip_sr_gradient(4, 8, 32, 3, 17, 1, p, p, p, p, p, p, p, None) == -3
    assert L.evogp_hip_sr_const_step(4, 32, 1, 0, p, p, p, p, p, p, p, p, p, None) == -1
    assert L.evogp_hip_sr_const_step(4, 32, 1, 3, p, p, p, p, p, p, None, None, p, None) == -2
    with pytest.raises(RuntimeError):
        torch.ops.evogp_hip.tree_SR_gradient(4, 8, 32, 3, 17, True, *_dev(np.zeros((4, 32), np.float32), np.zeros((4, 32), np.int16),
                                             np.zeros((4, 32), np.int16), np.zeros((8, 3), np.float32), np.zeros((8, 17), np.float32)))


def _check_optimised(f0, f1, loss1, X, y):
    v0, t0, s0 = (a.cpu().numpy() for a in f0._tensors())
    v1, t1, s1 = (a.cpu().numpy() for a in f1._tensors())
    assert np.array_equal(t0, t1) and np.array_equal(s0, s1)
    multi = f0.output_len > 1
    L = v0.shape[1]
    is_c = (((t0.astype(np.int32) & 0x7F) if multi else t0) == R.T_CONST) & (np.arange(L)[None, :] < np.clip(s0[:, :1], 0, L))
    assert np.array_equal(v0.view(np.uint32)[~is_c], v1.view(np.uint32)[~is_c])
    before = f0.SR_gradient(X, y)[0].cpu().numpy()
    after = loss1.cpu().numpy()
    fin = np.isfinite(before)
    assert np.all(after[fin] <= before[fin])
    assert np.array_equal(v0.view(np.uint32)[~fin], v1.view(np.uint32)[~fin])
    no_c = ~is_c.any(1)
    assert np.array_equal(v0.view(np.uint32)[no_c], v1.view(np.uint32)[no_c])
    # the returned loss is the returned forest's loss
    assert np.array_equal(np.isnan(after), np.isnan(f1.SR_gradient(X, y)[0].cpu().numpy()))
    return before, after


@pytest.mark.parametrize("out_len", [1, 3])
def test_optimize_constants_invariants(rng, out_len):
    from evogp_amd.tree import Forest

    value, type_, size, X, y = _case(rng, "all", out_len, 64, 500, pop=400)
    size[5, 0] = 0
    v, t, s, Xd, yd = _dev(value, type_, size, X, y)
    f0 = Forest(3, out_len, v, t, s)
    keep = [a.clone() for a in (v, t, s)]
    f1, loss1 = f0.optimize_constants(Xd, yd, steps=8, step_size=0.1)
    for a, b in zip(keep, (f0.batch_node_value, f0.batch_node_type, f0.batch_subtree_size)):
        assert torch.equal(a, b)   # the input forest is untouched
    before, after = _check_optimised(f0, f1, loss1, Xd, yd)
    assert np.isnan(after[5])
    fin = np.isfinite(before) & np.isfinite(after)
    # (a few trees near a pole carry losses of 1e16 that no constant step moves in fp32: the median, not the mean, shows the trend)
    assert np.median(after[fin]) < np.median(before[fin]) and (after[fin] < before[fin]).mean() > 0.2


def test_optimize_constants_planted_problem():
    from evogp_amd.tree import Forest

    rng = np.random.default_rng(7)
    X = rng.uniform(-1, 1, (256, 1)).astype(np.float32)
    y = (2.5 * X[:, :1] + 0.7).astype(np.float32)
    # c1 * x0 + c2 in prefix order, started at (1, 1)
    value = np.array([[R.F_ADD, R.F_MUL, 1.0, 0, 1.0]], np.float32)
    type_ = np.array([[R.T_BFUNC, R.T_BFUNC, R.T_CONST, R.T_VAR, R.T_CONST]], np.int16)
    size = np.array([[5, 3, 1, 1, 1]], np.int16)
    v, t, s, Xd, yd = _dev(value, type_, size, X, y)
    f1, loss = Forest(1, 1, v, t, s).optimize_constants(Xd, yd, steps=200, step_size=0.1)
    c = f1.batch_node_value.cpu().numpy()[0]
    assert abs(c[2] - 2.5) <= 1e-3 and abs(c[4] - 0.7) <= 1e-3, c
    assert float(loss[0]) < 1e-5


def test_optimize_constants_configs1_forest():
    from evogp_amd.tree import Forest, GenerateDescriptor

    desc = GenerateDescriptor(max_tree_len=64, input_len=10, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=6,
                              const_samples=[-1, 0, 1])
    f0 = Forest.random_generate(100_000, desc, keys=torch.tensor([42, 0], dtype=torch.uint32, device="cuda"))
    rng = np.random.default_rng(1234)
    X = rng.uniform(-5, 5, (1024, 10)).astype(np.float32)
    y = (X[:, 0] * X[:, 1] + X[:, 2] * X[:, 3] - X[:, 4] + 0.5 * X[:, 5] ** 2).astype(np.float32)[:, None]
    Xd, yd = _dev(X, y)
    f1, loss1 = f0.optimize_constants(Xd, yd, steps=5)
    assert f1.func_mask == f0.func_mask != 0
    before, after = _check_optimised(f0, f1, loss1, Xd, yd)
    fin = np.isfinite(before) & np.isfinite(after)
    # (a few trees near a pole carry losses of 1e16 that no constant step moves in fp32: the median, not the mean, shows the trend)
    assert np.median(after[fin]) < np.median(before[fin]) and (after[fin] < before[fin]).mean() > 0.2
    assert (after[fin] < before[fin]).mean() > 0.1
