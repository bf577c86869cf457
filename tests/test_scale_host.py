"""CPU: the host logic of linear scaling (Forest.SR_scaled_fitness / apply_scaling, SymbolicRegression(linear_scaling=),
StandardPipeline) with the numpy restatement registered as test-only CPU kernels (tests/cpu_scale_ops.py), and the argument checks
of the two new C entry points, which return before any launch."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cpu_dedup_ops  # noqa: E402
import cpu_grad_ops  # noqa: E402
import cpu_ops  # noqa: E402
import cpu_scale_ops  # noqa: E402
import linear_scaling_ref as LS  # noqa: E402
from grad_trees import ALL_FUNCS, ARITH, random_forest  # noqa: E402

cpu_ops.register()
cpu_grad_ops.register()
cpu_dedup_ops.register()
cpu_scale_ops.register()

from evogp_amd.problem import SymbolicRegression  # noqa: E402
from evogp_amd.tree import Forest, GenerateDescriptor, set_default_device  # noqa: E402
from evogp_amd.tree import utils as _tree_utils  # noqa: E402


@pytest.fixture(autouse=True)
def _cpu_default_device():
    saved = _tree_utils._DEVICE
    set_default_device("cpu")
    yield
    _tree_utils._DEVICE = saved


def _data(rng, D=40, var_len=2):
    X = rng.uniform(0.5, 1.5, (D, var_len)).astype(np.float32)
    y = (2.0 * X[:, :1] * X[:, 1:2] - 0.5).astype(np.float32)
    return torch.from_numpy(X), torch.from_numpy(y)


def _forest(rng, pop=30, funcs=ARITH, mask=0):
    value, type_, size = random_forest(rng, pop, 32, funcs, 2, 1, max_depth=4)
    return Forest(2, 1, *(torch.from_numpy(a) for a in (value, type_, size)), func_mask=mask)


def _bits(t):
    return t.contiguous().numpy().view(np.uint32)


def test_default_problem_calls_none_of_the_new_ops(rng):
    forest = _forest(rng)
    X, y = _data(rng)
    before = dict(cpu_scale_ops.calls)
    prob = SymbolicRegression(datapoints=X, labels=y)
    assert prob.linear_scaling is False
    fit = forest.SR_fitness(X, y)
    assert np.array_equal(_bits(prob.evaluate(forest)), _bits(-fit))
    want = torch.where(torch.isnan(fit), torch.full_like(fit, float("-inf")), -fit)
    assert np.array_equal(_bits(prob.scores(forest)), _bits(want))
    assert prob.optimize(forest) is forest
    assert cpu_scale_ops.calls == before


def test_value_errors(rng):
    X, y = _data(rng)
    with pytest.raises(ValueError):
        SymbolicRegression(datapoints=X, labels=torch.cat([y, y], dim=1), linear_scaling=True)
    prob = SymbolicRegression(datapoints=X, labels=y, linear_scaling=True)
    forest = _forest(rng, 4)
    with pytest.raises(ValueError):
        prob.evaluate(forest, use_MSE=False)
    with pytest.raises(ValueError):
        prob.scores(forest, use_MSE=False)
    multi = Forest(2, 3, *(torch.from_numpy(a) for a in random_forest(rng, 4, 32, ALL_FUNCS, 2, 3, max_depth=3)))
    with pytest.raises(AssertionError):
        multi.SR_scaled_fitness(X, torch.zeros(40, 3))
    with pytest.raises(AssertionError):
        multi.apply_scaling(torch.ones(4), torch.zeros(4))


def test_scaled_fitness_scores_and_torch_mode(rng):
    forest = _forest(rng, 40, ALL_FUNCS)
    X, y = _data(rng)
    # execute_mode="torch": the same definition from batch_forward in float64 torch, no kernel of the new file
    # (on well-formed trees here: the CPU oracle behind batch_forward has no NaN row for a malformed tree, the device has)
    n1 = cpu_scale_ops.calls["linear_scaling"]
    tprob = SymbolicRegression(datapoints=X, labels=y, linear_scaling=True, execute_mode="torch")
    tl, tb, ta = tprob.scaled_fitness(forest)
    assert cpu_scale_ops.calls["linear_scaling"] == n1
    clean = LS.scaling(cpu_scale_ops.predictions(*(a.numpy() for a in forest._tensors()), X.numpy()), y.numpy())
    assert LS.check_against(clean, tl.numpy(), ta.numpy(), tb.numpy(), 40, what="torch mode") <= 0.10   # float64 torch against float64 numpy
    assert np.array_equal(_bits(tprob.evaluate(forest)), _bits(-tl))
    assert np.array_equal(_bits(tprob.scores(forest)), _bits(torch.where(torch.isnan(tl), torch.full_like(tl, float("-inf")), -tl)))
    forest.batch_subtree_size[3, 0] = 0   # malformed
    P = cpu_scale_ops.predictions(*(a.numpy() for a in forest._tensors()), X.numpy())
    ref = LS.scaling(P, y.numpy())
    n0 = cpu_scale_ops.calls["linear_scaling"]
    prob = SymbolicRegression(datapoints=X, labels=y, linear_scaling=True)
    loss, slope, intercept = prob.scaled_fitness(forest)
    assert cpu_scale_ops.calls["linear_scaling"] == n0 + 1
    assert loss.shape == slope.shape == intercept.shape == (40,) and loss.dtype == torch.float32
    # (the CPU stand-in IS the restatement: this checks the plumbing -- argument order, the (intercept, slope) columns, float32 outputs --
    # not the arithmetic, which tests/test_gpu_linear_scaling.py checks on the device)
    LS.check_against(ref, loss.numpy(), intercept.numpy(), slope.numpy(), 40, what="CPU op (plumbing)")
    assert np.isnan(float(loss[3])) and np.isfinite(loss.numpy()).sum() > 20
    ev, sc = prob.evaluate(forest), prob.scores(forest)
    assert np.array_equal(_bits(ev), _bits(-loss))
    assert np.array_equal(_bits(sc), _bits(torch.where(torch.isnan(loss), torch.full_like(loss, float("-inf")), -loss)))
    # dedup: the same bits
    twice = forest + forest[:10]
    l1, b1, a1 = twice.SR_scaled_fitness(X, y)
    l2, b2, a2 = twice.SR_scaled_fitness(X, y, dedup=True)
    assert np.array_equal(_bits(l1), _bits(l2)) and np.array_equal(_bits(b1), _bits(b2)) and np.array_equal(_bits(a1), _bits(a2))
    assert np.array_equal(_bits(l1[40:]), _bits(l1[:10]))


def test_apply_scaling_and_func_mask(rng):
    sub_div = (1 << 2) | (1 << 4)
    forest = _forest(rng, 12, [2, 4], mask=sub_div)
    X, y = _data(rng)
    loss, slope, intercept = forest.SR_scaled_fitness(X, y)
    keep = [a.clone() for a in forest._tensors()]
    same, applied = forest.apply_scaling(slope, intercept)
    grown, applied_g = forest.apply_scaling(slope, intercept, grow=True)
    for a, b in zip(keep, forest._tensors()):
        assert torch.equal(a, b)
    assert same.max_tree_len == 32 and grown.max_tree_len == 36 and applied.dtype == torch.bool
    assert same.func_mask == grown.func_mask == sub_div | (1 << 1) | (1 << 3)
    unknown = Forest(2, 1, *forest._tensors())
    assert unknown.func_mask == 0 and unknown.apply_scaling(slope, intercept)[0].func_mask == 0
    finite = torch.isfinite(slope) & torch.isfinite(intercept)
    assert torch.equal(applied_g, finite) and finite.any()
    coef = torch.stack([intercept, slope], 1).numpy()
    want = LS.wrap_rows(*(a.numpy() for a in forest._tensors()), coef, 36)
    for got, w in zip(grown._tensors(), want[:3]):
        assert np.array_equal(got.numpy().view(np.uint16 if w.dtype == np.int16 else np.uint32), w.view(np.uint16 if w.dtype == np.int16 else np.uint32))
    # the wrapped tree is the scaled model: its plain MSE is the scaled loss up to the float32 evaluation of b p + a
    P = cpu_scale_ops.predictions(*(a.numpy() for a in forest._tensors()), X.numpy())
    mse = grown.SR_fitness(X, y).numpy().astype(np.float64)
    ok = finite.numpy()
    bound = LS.refit_bound(P, intercept.numpy(), slope.numpy(), loss.numpy()) + 1e-6 * np.abs(loss.numpy())   # + the float32 loss itself
    assert np.all(np.abs(mse - loss.numpy())[ok] <= bound[ok])
    # SymbolicRegression.scaled is apply_scaling of the forest's own coefficients with grow=True
    prob = SymbolicRegression(datapoints=X, labels=y, linear_scaling=True)
    for a, b in zip(prob.scaled(forest)._tensors(), grown._tensors()):
        assert torch.equal(a, b)


def test_pipeline_reports_the_wrapped_best_tree(rng):
    from evogp_amd.algorithm import DefaultCrossover, DefaultMutation, DefaultSelection, GeneticProgramming
    from evogp_amd.pipeline import StandardPipeline

    d = GenerateDescriptor(max_tree_len=32, input_len=2, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=4,
                           const_samples=[-1, 0, 1])
    X, y = _data(rng)

    def pipeline(**kw):
        algo = GeneticProgramming(Forest.random_generate(60, d, keys=torch.tensor([1, 2])), DefaultCrossover(), DefaultMutation(0.2, d),
                                  DefaultSelection(0.3, 2))
        return algo, StandardPipeline(algo, SymbolicRegression(datapoints=X, labels=y, **kw), generation_limit=2, is_show_details=False)

    algo, pipe = pipeline(linear_scaling=True)
    start = algo.forest
    loss, slope, intercept = start.SR_scaled_fitness(X, y)
    n0 = dict(cpu_scale_ops.calls)
    host = pipe.step()
    assert cpu_scale_ops.calls["linear_scaling"] == n0["linear_scaling"] + 2 and cpu_scale_ops.calls["wrap_linear"] == n0["wrap_linear"] + 1
    want = torch.where(torch.isnan(loss), torch.full_like(loss, float("-inf")), -loss)
    assert np.array_equal(_bits(host), _bits(want))
    best = int(torch.argmax(host))
    wrapped = start[best:best + 1].apply_scaling(slope[best:best + 1], intercept[best:best + 1], grow=True)[0][0]
    assert pipe.best_tree.node_value.shape == (36,) and torch.equal(pipe.best_tree.node_value, wrapped.node_value)
    assert torch.equal(pipe.best_tree.subtree_size, wrapped.subtree_size) and float(pipe.best_fitness) == float(host[best])
    # dedup=True deduplicates the population's pass, once, not the one-tree slice the best tree is wrapped from
    algo, pipe = pipeline(linear_scaling=True, dedup=True)
    h0 = cpu_dedup_ops.calls["tree_classes"]
    host_dedup = pipe.step()
    assert cpu_dedup_ops.calls["tree_classes"] == h0 + 1 and np.array_equal(_bits(host_dedup), _bits(host))
    assert torch.equal(pipe.best_tree.node_value, wrapped.node_value)
    # without the option: the tree as it stands in the forest, and none of the new ops
    algo, pipe = pipeline()
    start = algo.forest
    n0 = dict(cpu_scale_ops.calls)
    host = pipe.step()
    assert cpu_scale_ops.calls == n0
    assert torch.equal(pipe.best_tree.node_value, start[int(torch.argmax(host))].node_value)


def test_argument_errors_without_gpu():
    from evogp_amd import _lib

    L = _lib.lib
    p, q = 8, 16  # (never dereferenced: the host checks come first)
    assert L.evogp_hip_sr_linear_scaling(0, 8, 32, 3, 1, p, p, p, p, p, q, q, None) == -1
    assert L.evogp_hip_sr_linear_scaling(4, 0, 32, 3, 1, p, p, p, p, p, q, q, None) == -1
    assert L.evogp_hip_sr_linear_scaling(4, 8, 1025, 3, 1, p, p, p, p, p, q, q, None) == -1
    assert L.evogp_hip_sr_linear_scaling(4, 8, 32, 0, 1, p, p, p, p, p, q, q, None) == -1
    assert L.evogp_hip_sr_linear_scaling(4, 8, 32, 3, 0, p, p, p, p, p, q, q, None) == -1
    assert L.evogp_hip_sr_linear_scaling(4, 8, 32, 3, 2, p, p, p, p, p, q, q, None) == -3      # multi-output: unsupported
    assert L.evogp_hip_sr_linear_scaling(4, 8, 32, 3, 1, p, p, p, p, p, None, q, None) == -2
    assert L.evogp_hip_sr_linear_scaling(4, 8, 32, 3, 1, p, p, p, p, None, q, q, None) == -2
    assert L.evogp_hip_wrap_linear(0, 32, 32, p, p, p, p, q, q, q, q, None) == -1
    assert L.evogp_hip_wrap_linear(4, 32, 31, p, p, p, p, q, q, q, q, None) == -1               # the output rows may not shrink
    assert L.evogp_hip_wrap_linear(4, 1024, 1028, p, p, p, p, q, q, q, q, None) == -1
    assert L.evogp_hip_wrap_linear(4, 32, 36, p, p, p, p, p, q, q, q, None) == -1               # in place
    assert L.evogp_hip_wrap_linear(4, 32, 36, p, p, p, None, q, q, q, q, None) == -2
    assert L.evogp_hip_wrap_linear(4, 32, 36, p, p, p, p, q, q, q, None, None) == -2
    assert L.evogp_hip_abi_version() == _lib.ABI_VERSION
