"""CPU: the host logic of the derivative bounds (Forest.SR_derivative_intervals / monotone_mask, SymbolicRegression(monotonic=),
StandardPipeline) with the numpy restatement registered as a test-only CPU kernel (tests/cpu_derivative_ops.py), and the argument
checks of the new C entry point, which return before any launch."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cpu_dedup_ops  # noqa: E402
import cpu_derivative_ops  # noqa: E402
import cpu_grad_ops  # noqa: E402
import cpu_interval_ops  # noqa: E402
import cpu_ops  # noqa: E402
import cpu_scale_ops  # noqa: E402
import derivative_ref as DR  # noqa: E402
import interval_cases as IC  # noqa: E402
import sr_grad_ref as R  # noqa: E402
from grad_trees import ALL_FUNCS, random_forest  # noqa: E402
from interval_cases import B, C, U, V  # noqa: E402

cpu_ops.register()
cpu_grad_ops.register()
cpu_dedup_ops.register()
cpu_scale_ops.register()
cpu_interval_ops.register()
cpu_derivative_ops.register()

from evogp_amd.problem import SymbolicRegression  # noqa: E402
from evogp_amd.tree import Forest, GenerateDescriptor, set_default_device  # noqa: E402
from evogp_amd.tree import utils as _tree_utils  # noqa: E402

INF = float("inf")


@pytest.fixture(autouse=True)
def _cpu_default_device():
    saved = _tree_utils._DEVICE
    set_default_device("cpu")
    yield
    _tree_utils._DEVICE = saved


def _bits(t):
    return t.contiguous().numpy().view(np.uint32)


# x0 + x1 (up in both), x1 - 2 x0 (down in x0), x0 * x0 (up only where the box is >= 0), x0 / x1 (unsafe where x1 reaches 0),
# (x0 < 0.5) (a jump), 3 x0 (slope 3), -x0 * 1e30 * 1e30 (overflows: unsafe)
EXPRS = [B(R.F_ADD, V(0), V(1)), B(R.F_SUB, V(1), B(R.F_MUL, C(2.0), V(0))), B(R.F_MUL, V(0), V(0)), B(R.F_DIV, V(0), V(1)),
         B(R.F_LT, V(0), C(0.5)), B(R.F_MUL, V(0), C(3.0)), B(R.F_MUL, B(R.F_MUL, U(R.F_NEG, V(0)), C(1e30)), C(1e30))]


def _forest(exprs=EXPRS, L=16, var_len=2):
    return Forest(var_len, 1, *(torch.from_numpy(a) for a in IC.rows(exprs, L)))


def _data(rng, D=40):
    X = rng.uniform(0.5, 1.5, (D, 2)).astype(np.float32)
    y = (2.0 * X[:, :1] + X[:, 1:2] - 0.5).astype(np.float32)
    return torch.from_numpy(X), torch.from_numpy(y)


def test_argument_checks(rng):
    forest = _forest()
    dlo, dhi, dfl = forest.SR_derivative_intervals(-1.0, 1.0)
    assert dlo.shape == dhi.shape == dfl.shape == (2, 7, 16) and dlo.dtype == torch.float32 and dfl.dtype == torch.uint8
    want = DR.forest_derivative_intervals(*(a.numpy() for a in forest._tensors()), [-1.0, -1.0], [1.0, 1.0], [0, 1])[3:]
    for got, w in zip((dlo, dhi, dfl), want):
        assert np.array_equal(got.numpy().view(np.uint8), w.view(np.uint8))
    twice = forest.SR_derivative_intervals(-1.0, 1.0, wrt=[1, 1, 0])          # a repeated index: equal slices
    assert twice[0].shape == (3, 7, 16)
    for a, b in zip((dlo, dhi, dfl), twice):
        assert torch.equal(a[1], b[0]) and torch.equal(b[0], b[1]) and torch.equal(a[0], b[2])
    assert torch.equal(forest.SR_derivative_intervals(-1.0, 1.0, wrt=1)[0], dlo[1:2])
    assert torch.equal(forest.SR_derivative_intervals(-1.0, 1.0, wrt=torch.tensor([1]))[0], dlo[1:2])
    for wrt in ([], [2], [-1], [0, 5], torch.tensor([], dtype=torch.int64)):
        with pytest.raises(ValueError):
            forest.SR_derivative_intervals(-1.0, 1.0, wrt=wrt)
    for lower, upper in ((1.0, -1.0), (float("-inf"), 1.0), (0.0, float("nan")), (torch.zeros(3), torch.ones(3))):
        with pytest.raises(ValueError):
            forest.SR_derivative_intervals(lower, upper)
        with pytest.raises(ValueError):
            forest.monotone_mask(lower, upper, {0: 1})
    for bad in ({2: 1}, {-1: 1}, {0: 2}, {0: 0}, {0: (1.0, -1.0)}, {0: "up"}, {}):
        with pytest.raises(ValueError):
            forest.monotone_mask(-1.0, 1.0, bad)
    multi = Forest(2, 3, *(torch.from_numpy(a) for a in random_forest(rng, 4, 32, ALL_FUNCS, 2, 3, max_depth=3)))
    with pytest.raises(ValueError):
        multi.SR_derivative_intervals(-1.0, 1.0)
    with pytest.raises(ValueError):
        multi.monotone_mask(-1.0, 1.0, {0: 1})


def test_monotone_mask():
    forest = _forest()
    lower, upper = torch.tensor([-1.0, 0.5]), torch.tensor([1.0, 2.0])
    n0 = cpu_derivative_ops.calls["tree_derivative_intervals"]
    assert forest.monotone_mask(lower, upper, {0: 1}).tolist() == [True, False, False, True, False, True, False]
    assert cpu_derivative_ops.calls["tree_derivative_intervals"] == n0 + 1          # one call of the op
    assert forest.monotone_mask(lower, upper, {0: -1}).tolist() == [False, True, False, False, False, False, False]
    assert forest.monotone_mask(lower, upper, {0: 1, 1: 1}).tolist() == [True, False, False, False, False, True, False]
    assert forest.monotone_mask(lower, upper, {0: (-2.5, 2.5)}).tolist() == [True, True, True, True, False, False, False]
    assert forest.monotone_mask(lower, upper, {0: (0.0, INF)}).tolist() == forest.monotone_mask(lower, upper, {0: 1}).tolist()
    assert forest.monotone_mask(lower, upper, {1: (0.9, 1.1)}).tolist() == [True, True, False, False, False, False, False]
    assert forest.monotone_mask(lower, upper, {0: 1}, max_abs=2.5).tolist() == [False, False, False, True, False, False, False]
    # x0 * x0 is nondecreasing once the box lies on the positive side; x0 / x1 is unsafe once x1 reaches 0
    assert forest.monotone_mask(0.25, 1.0, {0: 1}).tolist() == [True, False, True, True, False, True, False]
    assert forest.monotone_mask(torch.tensor([0.25, 0.0]), 1.0, {0: 1}).tolist() == [True, False, True, False, False, True, False]
    # ([0, 1] + [0, 1] keeps its exact lower endpoint 0: x0 * x0 is proven on a box that touches 0)
    assert forest.monotone_mask(0.0, 1.0, {0: 1}).tolist() == [True, False, True, False, False, True, False]
    mask = forest.monotone_mask(lower, upper, {0: 1})
    assert mask.dtype == torch.bool and mask.shape == (7,)
    o = DR.forest_derivative_intervals(*(a.numpy() for a in forest._tensors()), lower.numpy(), upper.numpy(), [0, 1])
    assert DR.monotone(*o, [(0.0, INF), (0.0, INF)]).tolist() == forest.monotone_mask(lower, upper, {0: 1, 1: 1}).tolist()
    # the mask holds safe_mask
    assert not (forest.monotone_mask(lower, upper, {0: (-INF, INF)}) & ~forest.safe_mask(lower, upper)).any()


def test_problem_arguments(rng):
    X, y = _data(rng)
    prob = SymbolicRegression(datapoints=X, labels=y, monotonic={0: 1, 1: (-1.0, 4.0)}, input_margin=0.5)
    span = X.max(0).values - X.min(0).values
    assert torch.equal(prob.input_lower, X.min(0).values - 0.5 * span) and torch.equal(prob.input_upper, X.max(0).values + 0.5 * span)
    assert prob.monotonic == {0: 1, 1: (-1.0, 4.0)} and prob.interval_check is False
    both = SymbolicRegression(datapoints=X, labels=y, monotonic={0: -1}, interval_check=True, input_bounds=(-1.0, 2.0))
    assert both.input_lower.tolist() == [-1.0, -1.0] and both.input_upper.tolist() == [2.0, 2.0]
    for bad in ({2: 1}, {-1: 1}, {0: 3}, {0: (2.0, 1.0)}, {"x0": 1}, {}):
        with pytest.raises(ValueError):
            SymbolicRegression(datapoints=X, labels=y, monotonic=bad)
    with pytest.raises(ValueError):
        SymbolicRegression(datapoints=X, labels=torch.cat([y, y], dim=1), monotonic={0: 1})
    with pytest.raises(ValueError):
        SymbolicRegression(datapoints=X, labels=y).monotone_mask(_forest())
    assert prob.monotone_mask(_forest()).tolist() == _forest().monotone_mask(prob.input_lower, prob.input_upper, prob.monotonic).tolist()


@pytest.mark.parametrize("mode", ["auto", "torch"])
@pytest.mark.parametrize("scaling", [False, True])
def test_evaluate_and_scores_are_masked(mode, scaling, rng):
    X, y = _data(rng)
    forest = _forest()
    kw = dict(datapoints=X, labels=y, execute_mode=mode, linear_scaling=scaling)
    plain = SymbolicRegression(**kw)
    prob = SymbolicRegression(monotonic={0: 1}, input_bounds=(torch.tensor([-1.0, 0.5]), torch.tensor([1.0, 2.0])), **kw)
    mask = prob.monotone_mask(forest)
    assert mask.tolist() == [True, False, False, True, False, True, False]
    ev0, sc0 = plain.evaluate(forest), plain.scores(forest)
    assert torch.isfinite(ev0[:6]).all()            # every tree but the overflowing one scores on the rows: the mask is what removes them
    n0, i0 = cpu_derivative_ops.calls["tree_derivative_intervals"], cpu_interval_ops.calls["tree_intervals"]
    ev, sc = prob.evaluate(forest), prob.scores(forest)
    assert cpu_derivative_ops.calls["tree_derivative_intervals"] == n0 + 2 and cpu_interval_ops.calls["tree_intervals"] == i0
    if scaling:      # the slopes of the passing trees on this data are positive: nothing else is removed
        assert (plain.scaled_fitness(forest)[1][mask] > 0).all()
    assert np.array_equal(_bits(ev[mask]), _bits(ev0[mask])) and np.array_equal(_bits(sc[mask]), _bits(sc0[mask]))
    assert torch.isnan(ev[~mask]).all() and (sc[~mask] == float("-inf")).all()


@pytest.mark.parametrize("mode", ["auto", "torch"])
def test_negative_slope_fails_under_a_sign_constraint(mode, rng):
    """linear scaling fits a + b T(x): with b < 0 a tree proven nondecreasing is scored as a nonincreasing model, so it fails"""
    X = torch.from_numpy(rng.uniform(0.5, 1.5, (40, 2)).astype(np.float32))
    y = (-2.0 * X[:, :1] + 0.25).to(torch.float32)           # decreasing in x0: x0 + c fits with slope -2
    forest = _forest([B(R.F_ADD, V(0), C(1.0)), B(R.F_SUB, C(1.0), V(0)), B(R.F_MUL, V(0), C(3.0))])
    kw = dict(datapoints=X, labels=y, execute_mode=mode, linear_scaling=True, input_bounds=(0.0, 2.0))
    plain = SymbolicRegression(**kw)
    loss0, slope0, _ = plain.scaled_fitness(forest)
    assert slope0[0] < 0 and slope0[1] > 0 and slope0[2] < 0 and torch.isfinite(loss0).all()
    up = SymbolicRegression(monotonic={0: 1}, **kw)
    assert up.monotone_mask(forest).tolist() == [True, False, True]
    loss, slope, icpt = up.scaled_fitness(forest)
    assert torch.isnan(loss[0]) and torch.isnan(loss[2]) and np.array_equal(_bits(loss[1:2]), _bits(loss0[1:2]))
    assert np.array_equal(_bits(slope), _bits(slope0))                                  # the coefficients themselves are reported
    assert torch.isnan(up.evaluate(forest)).tolist() == [True, True, True]             # 0, 2: the slope; 1: the mask
    assert (up.scores(forest) == float("-inf")).all()
    # a range constraint bounds the unscaled tree and leaves the slope alone
    ranged = SymbolicRegression(monotonic={0: (0.0, 5.0)}, **kw)
    assert np.array_equal(_bits(ranged.scaled_fitness(forest)[0]), _bits(loss0))
    assert torch.isfinite(ranged.evaluate(forest)).tolist() == [True, False, True]
    # the decreasing constraint keeps x0 - style trees out and 1 - x0 in, whose slope is positive
    down = SymbolicRegression(monotonic={0: -1}, **kw)
    assert torch.isfinite(down.scores(forest)).tolist() == [False, True, False]
    assert np.array_equal(_bits(down.scores(forest)[1:2]), _bits(plain.scores(forest)[1:2]))


def test_mask_with_dedup_and_optimize(rng):
    X, y = _data(rng)
    forest = _forest(EXPRS + EXPRS[:2])
    box = (torch.tensor([-1.0, 0.5]), torch.tensor([1.0, 2.0]))
    prob = SymbolicRegression(datapoints=X, labels=y, monotonic={0: 1}, input_bounds=box, dedup=True, linear_scaling=True)
    plain = SymbolicRegression(datapoints=X, labels=y, dedup=True, linear_scaling=True)
    mask = prob.monotone_mask(forest)
    assert mask.tolist() == [True, False, False, True, False, True, False, True, False]
    assert np.array_equal(_bits(prob.scores(forest)[mask]), _bits(plain.scores(forest)[mask]))
    assert (prob.scores(forest)[~mask] == float("-inf")).all()
    assert prob.optimize(forest) is forest


def test_default_problem_calls_none_of_the_new_code(rng):
    X, y = _data(rng)
    forest = _forest()
    before = dict(cpu_derivative_ops.calls)
    prob = SymbolicRegression(datapoints=X, labels=y)
    assert prob.monotonic is None and not hasattr(prob, "input_lower")
    fit = forest.SR_fitness(X, y)
    assert np.array_equal(_bits(prob.evaluate(forest)), _bits(-fit))
    assert np.array_equal(_bits(prob.scores(forest)), _bits(torch.where(torch.isnan(fit), torch.full_like(fit, float("-inf")), -fit)))
    SymbolicRegression(datapoints=X, labels=y, linear_scaling=True).scores(forest)
    checked = SymbolicRegression(datapoints=X, labels=y, interval_check=True, input_bounds=(-1.0, 2.0))
    checked.scores(forest)
    forest.SR_intervals(-1.0, 1.0)
    forest.safe_mask(-1.0, 1.0)
    assert cpu_derivative_ops.calls == before


def test_pipeline_best_tree_is_monotone(rng):
    from evogp_amd.algorithm import DefaultCrossover, DefaultMutation, DefaultSelection, GeneticProgramming
    from evogp_amd.pipeline import StandardPipeline

    d = GenerateDescriptor(max_tree_len=32, input_len=2, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=4,
                           const_samples=[-1, 0, 1])
    X, y = _data(rng)
    algo = GeneticProgramming(Forest.random_generate(60, d, keys=torch.tensor([1, 2])), DefaultCrossover(), DefaultMutation(0.2, d),
                              DefaultSelection(0.3, 2))
    prob = SymbolicRegression(datapoints=X, labels=y, monotonic={0: 1, 1: 1}, input_margin=0.25)
    pipe = StandardPipeline(algo, prob, generation_limit=3, is_show_details=False)
    n0 = cpu_derivative_ops.calls["tree_derivative_intervals"]
    start = algo.forest
    host = pipe.step()
    assert cpu_derivative_ops.calls["tree_derivative_intervals"] == n0 + 1
    mask = prob.monotone_mask(start)
    assert 0 < int(mask.sum()) < 60 and (host[~mask] == float("-inf")).all() and torch.isfinite(host[mask]).any()
    for _ in range(2):
        pipe.step()
    best = pipe.best_tree
    one = Forest(2, 1, best.node_value[None, :], best.node_type[None, :], best.subtree_size[None, :])
    assert bool(prob.monotone_mask(one)[0]) and np.isfinite(float(pipe.best_fitness))


def test_argument_errors_without_gpu():
    from evogp_amd import _lib

    L = _lib.lib
    p, q = 8, 16  # (never dereferenced: the host checks come first)
    call = L.evogp_hip_tree_derivative_intervals
    assert call(0, 32, 3, p, p, p, p, p, 1, p, q, q, q, q, q, q, None) == -1
    assert call(4, 0, 3, p, p, p, p, p, 1, p, q, q, q, q, q, q, None) == -1
    assert call(4, 1025, 3, p, p, p, p, p, 1, p, q, q, q, q, q, q, None) == -1
    assert call(4, 32, 0, p, p, p, p, p, 1, p, q, q, q, q, q, q, None) == -1
    assert call(4, 32, 3, p, p, p, p, p, 0, p, q, q, q, q, q, q, None) == -1
    assert call(4, 32, 3, p, p, p, p, p, 65536, p, q, q, q, q, q, q, None) == -1
    assert call(4, 32, 3, p, p, p, p, p, 1, None, q, q, q, q, q, q, None) == -2
    assert call(4, 32, 3, p, p, p, None, p, 1, p, q, q, q, q, q, q, None) == -2
    assert call(4, 32, 3, p, p, p, p, p, 1, p, q, q, q, q, q, None, None) == -2
    assert L.evogp_hip_abi_version() == _lib.ABI_VERSION
