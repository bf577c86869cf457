"""CPU: the host logic of the interval pass (Forest.SR_intervals / safe_mask, SymbolicRegression(interval_check=), StandardPipeline)
with the numpy restatement registered as a test-only CPU kernel (tests/cpu_interval_ops.py), and the argument checks of the new C
entry point, which return before any launch."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cpu_dedup_ops  # noqa: E402
import cpu_grad_ops  # noqa: E402
import cpu_interval_ops  # noqa: E402
import cpu_ops  # noqa: E402
import cpu_scale_ops  # noqa: E402
import interval_cases as IC  # noqa: E402
import interval_ref as IR  # noqa: E402
import sr_grad_ref as R  # noqa: E402
from grad_trees import ALL_FUNCS, random_forest  # noqa: E402
from interval_cases import B, C, U, V  # noqa: E402

cpu_ops.register()
cpu_grad_ops.register()
cpu_dedup_ops.register()
cpu_scale_ops.register()
cpu_interval_ops.register()

from evogp_amd.problem import SymbolicRegression  # noqa: E402
from evogp_amd.tree import Forest, GenerateDescriptor, set_default_device  # noqa: E402
from evogp_amd.tree import utils as _tree_utils  # noqa: E402


@pytest.fixture(autouse=True)
def _cpu_default_device():
    saved = _tree_utils._DEVICE
    set_default_device("cpu")
    yield
    _tree_utils._DEVICE = saved


def _bits(t):
    return t.contiguous().numpy().view(np.uint32)


# x0 + 1 (safe), 1 / x1 (unsafe where the box holds 0), sqrt(x0) (unsafe where it reaches below 0), x0 * x1 (safe), x0 * 1e30 * 1e30
EXPRS = [B(R.F_ADD, V(0), C(1.0)), B(R.F_DIV, C(1.0), V(1)), U(R.F_SQRT, V(0)), B(R.F_MUL, V(0), V(1)),
         B(R.F_MUL, B(R.F_MUL, V(0), C(1e30)), C(1e30))]


def _forest(exprs=EXPRS, L=16, var_len=2):
    return Forest(var_len, 1, *(torch.from_numpy(a) for a in IC.rows(exprs, L)))


def _data(rng, D=40):
    X = rng.uniform(0.5, 1.5, (D, 2)).astype(np.float32)
    y = (2.0 * X[:, :1] * X[:, 1:2] - 0.5).astype(np.float32)
    return torch.from_numpy(X), torch.from_numpy(y)


def test_argument_checks(rng):
    forest = _forest()
    lo, hi, fl = forest.SR_intervals(-1.0, 1.0)
    assert lo.shape == hi.shape == fl.shape == (5, 16) and lo.dtype == torch.float32 and fl.dtype == torch.uint8
    same = forest.SR_intervals(torch.tensor([-1.0, -1.0]), torch.tensor([1.0, 1.0], dtype=torch.float64))
    for a, b in zip((lo, hi, fl), same):
        assert torch.equal(a, b)
    for lower, upper in ((1.0, -1.0), (torch.tensor([0.0, 2.0]), torch.tensor([1.0, 1.0])), (float("-inf"), 1.0), (0.0, float("nan")),
                         (torch.zeros(3), torch.ones(3)), (torch.zeros(1), 1.0)):
        with pytest.raises(ValueError):
            forest.SR_intervals(lower, upper)
        with pytest.raises(ValueError):
            forest.safe_mask(lower, upper)
    multi = Forest(2, 3, *(torch.from_numpy(a) for a in random_forest(rng, 4, 32, ALL_FUNCS, 2, 3, max_depth=3)))
    with pytest.raises(ValueError):
        multi.SR_intervals(-1.0, 1.0)
    with pytest.raises(ValueError):
        multi.safe_mask(-1.0, 1.0)


def test_safe_mask_against_flags_and_bounds():
    forest = _forest()
    lower, upper = torch.tensor([-1.0, 0.5]), torch.tensor([3.0, 2.0])
    lo, hi, fl = forest.SR_intervals(lower, upper)
    want = IR.forest_intervals(*(a.numpy() for a in forest._tensors()), lower.numpy(), upper.numpy())
    for got, w in zip((lo, hi, fl), want):
        assert np.array_equal(got.numpy().view(np.uint8), w.view(np.uint8))
    assert forest.safe_mask(lower, upper).tolist() == [True, True, False, True, False]          # sqrt reaches below 0; 3e60 overflows
    assert forest.safe_mask(lower, upper, max_abs=4.0).tolist() == [True, True, False, False, False]   # x0 * x1 reaches 6
    assert forest.safe_mask(lower, upper, max_abs=3.9).tolist() == [False, True, False, False, False]  # x0 + 1 reaches 4
    assert forest.safe_mask(-1.0, 1.0).tolist() == [True, False, False, True, False]            # 1 / x1 over a box that holds 0
    assert forest.safe_mask(lower, upper).dtype == torch.bool
    for mx in (float("inf"), 4.0):
        assert forest.safe_mask(lower, upper, mx).tolist() == IR.safe(*want, max_abs=mx).tolist()


def test_data_box_and_margin(rng):
    X, y = _data(rng)
    prob = SymbolicRegression(datapoints=X, labels=y, interval_check=True)
    assert torch.equal(prob.input_lower, X.min(0).values) and torch.equal(prob.input_upper, X.max(0).values)
    wide = SymbolicRegression(datapoints=X, labels=y, interval_check=True, input_margin=0.5)
    span = X.max(0).values - X.min(0).values
    assert torch.equal(wide.input_lower, X.min(0).values - 0.5 * span) and torch.equal(wide.input_upper, X.max(0).values + 0.5 * span)
    pair = SymbolicRegression(datapoints=X, labels=y, interval_check=True, input_bounds=(-1.0, torch.tensor([2.0, 3.0])), input_margin=1.0)
    assert pair.input_lower.tolist() == [-4.0, -5.0] and pair.input_upper.tolist() == [5.0, 7.0]
    with pytest.raises(ValueError):
        SymbolicRegression(datapoints=X, labels=y, interval_check=True, input_bounds="rows")
    with pytest.raises(ValueError):
        SymbolicRegression(datapoints=X, labels=torch.cat([y, y], dim=1), interval_check=True)
    # the data box holds no 0 in x1: 1 / x1 is safe on it, and unsafe once the margin takes the box across 0
    forest = _forest()
    assert prob.safe_mask(forest).tolist() == [True, True, True, True, False]
    assert SymbolicRegression(datapoints=X, labels=y, interval_check=True, input_margin=2.0).safe_mask(forest).tolist() == [
        True, False, False, True, False]


@pytest.mark.parametrize("mode", ["auto", "torch"])
@pytest.mark.parametrize("scaling", [False, True])
def test_evaluate_and_scores_are_masked(mode, scaling, rng):
    X, y = _data(rng)
    forest = _forest()
    kw = dict(datapoints=X, labels=y, execute_mode=mode, linear_scaling=scaling)
    plain = SymbolicRegression(**kw)
    prob = SymbolicRegression(interval_check=True, input_bounds=(-1.0, 2.0), **kw)
    mask = forest.safe_mask(-1.0, 2.0)
    assert mask.tolist() == [True, False, False, True, False]
    ev0, sc0 = plain.evaluate(forest), plain.scores(forest)
    assert torch.isfinite(ev0[:4]).all()            # every tree but the overflowing one scores on the rows: the mask is what removes them
    n0 = cpu_interval_ops.calls["tree_intervals"]
    ev, sc = prob.evaluate(forest), prob.scores(forest)
    assert cpu_interval_ops.calls["tree_intervals"] == n0 + 2
    assert np.array_equal(_bits(ev[mask]), _bits(ev0[mask])) and np.array_equal(_bits(sc[mask]), _bits(sc0[mask]))
    assert torch.isnan(ev[~mask]).all() and (sc[~mask] == float("-inf")).all()


def test_mask_with_dedup_and_optimize(rng):
    X, y = _data(rng)
    forest = _forest(EXPRS + EXPRS[:2])
    prob = SymbolicRegression(datapoints=X, labels=y, interval_check=True, input_bounds=(-1.0, 2.0), dedup=True, linear_scaling=True)
    plain = SymbolicRegression(datapoints=X, labels=y, dedup=True, linear_scaling=True)
    mask = forest.safe_mask(-1.0, 2.0)
    assert mask.tolist() == [True, False, False, True, False, True, False]
    assert np.array_equal(_bits(prob.scores(forest)[mask]), _bits(plain.scores(forest)[mask]))
    assert prob.optimize(forest) is forest


def test_default_problem_calls_none_of_the_new_code(rng):
    X, y = _data(rng)
    forest = _forest()
    before = dict(cpu_interval_ops.calls)
    prob = SymbolicRegression(datapoints=X, labels=y)
    assert prob.interval_check is False and not hasattr(prob, "input_lower")
    fit = forest.SR_fitness(X, y)
    assert np.array_equal(_bits(prob.evaluate(forest)), _bits(-fit))
    assert np.array_equal(_bits(prob.scores(forest)), _bits(torch.where(torch.isnan(fit), torch.full_like(fit, float("-inf")), -fit)))
    assert prob.optimize(forest) is forest
    SymbolicRegression(datapoints=X, labels=y, linear_scaling=True).scores(forest)
    assert cpu_interval_ops.calls == before


def test_pipeline_best_tree_is_safe(rng):
    from evogp_amd.algorithm import DefaultCrossover, DefaultMutation, DefaultSelection, GeneticProgramming
    from evogp_amd.pipeline import StandardPipeline

    d = GenerateDescriptor(max_tree_len=32, input_len=2, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=4,
                           const_samples=[-1, 0, 1])
    X, y = _data(rng)
    algo = GeneticProgramming(Forest.random_generate(60, d, keys=torch.tensor([1, 2])), DefaultCrossover(), DefaultMutation(0.2, d),
                              DefaultSelection(0.3, 2))
    prob = SymbolicRegression(datapoints=X, labels=y, interval_check=True, input_margin=1.0)
    pipe = StandardPipeline(algo, prob, generation_limit=3, is_show_details=False)
    n0 = cpu_interval_ops.calls["tree_intervals"]
    start = algo.forest
    host = pipe.step()
    assert cpu_interval_ops.calls["tree_intervals"] == n0 + 1
    mask = prob.safe_mask(start)
    assert 0 < int(mask.sum()) < 60 and (host[~mask] == float("-inf")).all() and torch.isfinite(host[mask]).any()
    for _ in range(2):
        pipe.step()
    best = pipe.best_tree
    one = Forest(2, 1, best.node_value[None, :], best.node_type[None, :], best.subtree_size[None, :])
    assert bool(prob.safe_mask(one)[0]) and np.isfinite(float(pipe.best_fitness))


def test_argument_errors_without_gpu():
    from evogp_amd import _lib

    L = _lib.lib
    p, q = 8, 16  # (never dereferenced: the host checks come first)
    assert L.evogp_hip_tree_intervals(0, 32, 3, p, p, p, p, p, q, q, q, None) == -1
    assert L.evogp_hip_tree_intervals(4, 0, 3, p, p, p, p, p, q, q, q, None) == -1
    assert L.evogp_hip_tree_intervals(4, 1025, 3, p, p, p, p, p, q, q, q, None) == -1
    assert L.evogp_hip_tree_intervals(4, 32, 0, p, p, p, p, p, q, q, q, None) == -1
    assert L.evogp_hip_tree_intervals(4, 32, 3, p, p, p, None, p, q, q, q, None) == -2
    assert L.evogp_hip_tree_intervals(4, 32, 3, p, p, p, p, p, q, q, None, None) == -2
    assert L.evogp_hip_abi_version() == _lib.ABI_VERSION
