"""CPU: the host logic of dimensional analysis (Forest.SR_dimensions / dimension_mask, tree.utils.str_unit, SymbolicRegression(input_units=,
label_units=, dimension_penalty=)) with the integer restatement registered as a test-only CPU kernel (tests/cpu_dimension_ops.py), and
the argument checks of the new C entry point, which return before any launch."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cpu_dedup_ops  # noqa: E402
import cpu_dimension_ops  # noqa: E402
import cpu_grad_ops  # noqa: E402
import cpu_interval_ops  # noqa: E402
import cpu_ops  # noqa: E402
import cpu_scale_ops  # noqa: E402
import dimension_ref as DR  # noqa: E402
import interval_cases as IC  # noqa: E402
import sr_grad_ref as R  # noqa: E402
from grad_trees import ALL_FUNCS, random_forest  # noqa: E402
from interval_cases import B, C, U, V  # noqa: E402

cpu_ops.register()
cpu_grad_ops.register()
cpu_dedup_ops.register()
cpu_scale_ops.register()
cpu_interval_ops.register()
cpu_dimension_ops.register()

from evogp_amd.problem import SymbolicRegression  # noqa: E402
from evogp_amd.tree import Forest, set_default_device, str_unit  # noqa: E402
from evogp_amd.tree import utils as _tree_utils  # noqa: E402

DEN = 25200


@pytest.fixture(autouse=True)
def _cpu_default_device():
    saved = _tree_utils._DEVICE
    set_default_device("cpu")
    yield
    _tree_utils._DEVICE = saved


def _bits(t):
    return t.contiguous().numpy().view(np.uint32)


# x0 in metres, x1 in seconds, the target in metres per second
UNITS, LABEL = [[1, 0], [0, 1]], [1, -1]
# x0 / x1 (consistent); x0 + x1 (the sum, and the root); 2 * (x0 / x1) (consistent, the constant a number); sin(x0) (the sine, and the
# root); x0 (the root alone); x0 / x1 + c (consistent, c in m/s); 1 / x1 (defined only off 0; a frequency: the root alone)
EXPRS = [B(R.F_DIV, V(0), V(1)), B(R.F_ADD, V(0), V(1)), B(R.F_MUL, C(2.0), B(R.F_DIV, V(0), V(1))), U(R.F_SIN, V(0)), V(0),
         B(R.F_ADD, B(R.F_DIV, V(0), V(1)), C(1.0)), U(R.F_INV, V(1))]
VIOL = [0, 2, 0, 2, 1, 0, 1]
VIOL_FREE_ROOT = [0, 1, 0, 1, 0, 0, 0]


def _forest(exprs=EXPRS, L=16, var_len=2):
    return Forest(var_len, 1, *(torch.from_numpy(a) for a in IC.rows(exprs, L)))


def _data(rng, D=40):
    X = rng.uniform(0.5, 1.5, (D, 2)).astype(np.float32)
    y = (2.0 * X[:, :1] / X[:, 1:2] - 0.5).astype(np.float32)
    return torch.from_numpy(X), torch.from_numpy(y)


def test_unit_conversion_and_argument_checks(rng):
    forest = _forest()
    units, flags, viol = forest.SR_dimensions(UNITS, LABEL)
    assert units.shape == (7, 16, 2) and units.dtype == torch.int32 and flags.shape == (7, 16) and flags.dtype == torch.uint8
    assert viol.dtype == torch.int32 and viol.tolist() == VIOL
    assert cpu_dimension_ops.last["var_units"].tolist() == [[DEN, 0], [0, DEN]] and cpu_dimension_ops.last["label_units"].tolist() == [DEN, -DEN]
    assert cpu_dimension_ops.last["check_root"] is True
    want = DR.forest_dimensions(*(a.numpy() for a in forest._tensors()), [[DEN, 0], [0, DEN]], [DEN, -DEN], True)
    for got, w in zip((units, flags, viol), want):
        assert np.array_equal(got.numpy(), w)
    assert forest.SR_dimensions(UNITS)[2].tolist() == VIOL_FREE_ROOT and cpu_dimension_ops.last["check_root"] is False
    # ints, floats, Fractions, tensors and arrays: the same numerators, exactly
    forest.SR_dimensions([[0.5, Fraction(1, 3)], [Fraction(-7, 25200), 2]], np.array([1.5, -0.25]))
    assert cpu_dimension_ops.last["var_units"].tolist() == [[12600, 8400], [-7, 50400]] and cpu_dimension_ops.last["label_units"].tolist() == [37800, -6300]
    forest.SR_dimensions(torch.tensor([[1.0], [2.0]]), torch.tensor([3]))
    assert cpu_dimension_ops.last["var_units"].tolist() == [[DEN], [2 * DEN]] and cpu_dimension_ops.last["label_units"].tolist() == [3 * DEN]
    edge = Fraction(1 << 24, DEN)
    forest.SR_dimensions([[edge, -edge], [0, 0]])
    assert cpu_dimension_ops.last["var_units"].tolist() == [[1 << 24, -(1 << 24)], [0, 0]]
    n0 = cpu_dimension_ops.calls["tree_dimensions"]
    for iu, lu in (([[0.1, 0], [0, 1]], None),                         # 0.1 is no multiple of 1 / 25200 (nor is the float)
                   ([[Fraction(1, 11), 0], [0, 1]], None),
                   ([[1000, 0], [0, 1]], None),                        # 1000 * 25200 > 2^24
                   ([[edge + Fraction(1, DEN), 0], [0, 1]], None),
                   ([[float("nan"), 0], [0, 1]], None), ([[float("inf"), 0], [0, 1]], None),
                   ([["1/2", 0], [0, 1]], None), ([[True, 0], [0, 1]], None), ([[None, 0], [0, 1]], None), (UNITS, ["1", 0]),   # ints, floats, Fractions only
                   ([[1, 0]], None), ([[1, 0], [0, 1], [0, 0]], None), ([[1, 0], [0]], None), ([1, 0], None), ([[], []], None),
                   ([[0] * 9, [0] * 9], None),                         # 9 base dimensions
                   ([[[1, 0]], [[0, 1]]], None),
                   (UNITS, [1]), (UNITS, [1, 0, 0]), (UNITS, [[1, 0]]), (UNITS, [0.1, 0]), (UNITS, 1)):
        with pytest.raises(ValueError):
            forest.SR_dimensions(iu, lu)
        with pytest.raises(ValueError):
            forest.dimension_mask(iu, lu)
    assert cpu_dimension_ops.calls["tree_dimensions"] == n0      # every fault fails on the host, before the op
    multi = Forest(2, 3, *(torch.from_numpy(a) for a in random_forest(rng, 4, 32, ALL_FUNCS, 2, 3, max_depth=3)))
    with pytest.raises(ValueError):
        multi.SR_dimensions(UNITS, LABEL)
    with pytest.raises(ValueError):
        multi.dimension_mask(UNITS)


def test_dimension_mask():
    forest = _forest()
    mask = forest.dimension_mask(UNITS, LABEL)
    assert mask.dtype == torch.bool and mask.tolist() == [v == 0 for v in VIOL]
    assert forest.dimension_mask(UNITS).tolist() == [v == 0 for v in VIOL_FREE_ROOT]
    units = forest.SR_dimensions(UNITS, LABEL)[0]
    assert units[2, 1].tolist() == [0, 0] and units[5, 4].tolist() == [DEN, -DEN]     # the constants of rows 2 and 5


def test_str_unit():
    assert str_unit([DEN, -2 * DEN], ["m", "s"]) == "m s^-2"
    assert str_unit([DEN // 2, 0], ["m", "s"]) == "m^1/2"
    assert str_unit(torch.tensor([0, 0]), ["m", "s"]) == "1"
    assert str_unit(np.array([-8400, 3 * DEN, 1], np.int32)) == "d0^-1/3 d1^3 d2^1/25200"
    assert str_unit([0, DEN], ["kg", "K"]) == "K"
    with pytest.raises(ValueError):
        str_unit([DEN, 0], ["m"])
    forest = _forest()
    units = forest.SR_dimensions(UNITS, LABEL)[0]
    assert str_unit(units[0, 0], ["m", "s"]) == "m s^-1" and str_unit(units[5, 4], ["m", "s"]) == "m s^-1"


@pytest.mark.parametrize("mode", ["auto", "torch"])
def test_hard_constraint(mode, rng):
    X, y = _data(rng)
    forest = _forest()
    plain = SymbolicRegression(datapoints=X, labels=y, execute_mode=mode)
    prob = SymbolicRegression(datapoints=X, labels=y, execute_mode=mode, input_units=UNITS, label_units=LABEL)
    assert prob.dimension_penalty is None and prob.input_units == [[1, 0], [0, 1]] and prob.label_units == [1, -1]
    mask = prob.dimension_mask(forest)
    assert mask.tolist() == [v == 0 for v in VIOL] and prob.dimensions(forest)[2].tolist() == VIOL
    ev0, sc0 = plain.evaluate(forest), plain.scores(forest)
    assert torch.isfinite(ev0).all()                 # every tree scores on the rows: the units are what removes them
    n0 = cpu_dimension_ops.calls["tree_dimensions"]
    ev, sc = prob.evaluate(forest), prob.scores(forest)
    assert cpu_dimension_ops.calls["tree_dimensions"] == n0 + 2
    assert np.array_equal(_bits(ev[mask]), _bits(ev0[mask])) and np.array_equal(_bits(sc[mask]), _bits(sc0[mask]))
    assert torch.isnan(ev[~mask]).all() and (sc[~mask] == float("-inf")).all()


def test_soft_penalty(rng):
    X, y = _data(rng)
    forest = _forest()
    plain = SymbolicRegression(datapoints=X, labels=y)
    prob = SymbolicRegression(datapoints=X, labels=y, input_units=UNITS, label_units=LABEL, dimension_penalty=0.25)
    viol = torch.tensor(VIOL)
    ev0, sc0 = plain.evaluate(forest), plain.scores(forest)
    ev, sc = prob.evaluate(forest), prob.scores(forest)
    ok = viol == 0
    assert np.array_equal(_bits(ev[ok]), _bits(ev0[ok])) and np.array_equal(_bits(sc[ok]), _bits(sc0[ok]))     # bit for bit
    assert torch.equal(ev[~ok], ev0[~ok] - 0.25 * viol[~ok].float()) and torch.equal(sc[~ok], sc0[~ok] - 0.25 * viol[~ok].float())
    zero = SymbolicRegression(datapoints=X, labels=y, input_units=UNITS, label_units=LABEL, dimension_penalty=0)
    assert np.array_equal(_bits(zero.scores(forest)), _bits(sc0))
    # a malformed row (violations = -1) is treated as in the hard case, whatever the penalty
    value, type_, size = (torch.from_numpy(a) for a in IC.rows(EXPRS[:3], 16))
    size[2, 0] = 2
    broken = Forest(2, 1, value, type_, size)
    assert prob.dimensions(broken)[2].tolist() == [0, 2, -1]
    fit = torch.tensor([-1.0, -2.0, -3.0])
    assert prob._masked(broken, fit, float("-inf")).tolist() == [-1.0, -2.5, float("-inf")]
    assert torch.isnan(prob._masked(broken, fit, float("nan"))[2])


@pytest.mark.parametrize("penalty", [None, 0.5])
def test_combined_with_the_interval_check(penalty, rng):
    X, y = _data(rng)
    forest = _forest()
    plain = SymbolicRegression(datapoints=X, labels=y)
    box = SymbolicRegression(datapoints=X, labels=y, interval_check=True, input_bounds=(-1.0, 2.0))
    prob = SymbolicRegression(datapoints=X, labels=y, interval_check=True, input_bounds=(-1.0, 2.0), input_units=UNITS, label_units=LABEL,
                              dimension_penalty=penalty)
    safe = box.safe_mask(forest)
    assert safe.tolist() == [False, True, False, True, True, False, False]     # a division by x1 is undefined on a box that holds 0
    viol = torch.tensor(VIOL)
    n_itv, n_dim = cpu_interval_ops.calls["tree_intervals"], cpu_dimension_ops.calls["tree_dimensions"]
    sc = prob.scores(forest)
    assert cpu_interval_ops.calls["tree_intervals"] == n_itv + 1 and cpu_dimension_ops.calls["tree_dimensions"] == n_dim + 1
    sc0 = plain.scores(forest)
    if penalty is None:
        keep = safe & (viol == 0)
        assert not keep.any() and (sc == float("-inf")).all()       # no tree of this forest passes both
        both = SymbolicRegression(datapoints=X, labels=y, interval_check=True, input_bounds=(0.25, 2.0), input_units=UNITS, label_units=LABEL)
        keep = both.safe_mask(forest) & both.dimension_mask(forest)
        assert keep.tolist() == [True, False, True, False, False, True, False]
        got = both.scores(forest)
        assert np.array_equal(_bits(got[keep]), _bits(sc0[keep])) and (got[~keep] == float("-inf")).all()
        assert torch.isnan(both.evaluate(forest)[~keep]).all()
    else:
        assert (sc[~safe] == float("-inf")).all() and torch.equal(sc[safe], sc0[safe] - penalty * viol[safe].float())


def test_linear_scaling_leaves_the_root_free(rng):
    X, y = _data(rng)
    forest = _forest()
    plain = SymbolicRegression(datapoints=X, labels=y, linear_scaling=True)
    prob = SymbolicRegression(datapoints=X, labels=y, linear_scaling=True, input_units=UNITS, label_units=LABEL)
    assert prob.dimensions(forest)[2].tolist() == VIOL_FREE_ROOT and cpu_dimension_ops.last["check_root"] is False
    mask = prob.dimension_mask(forest)
    assert mask.tolist() == [True, False, True, False, True, True, True]      # x0 and 1 / x1 pass: slope and intercept carry the unit
    sc, sc0 = prob.scores(forest), plain.scores(forest)
    assert np.array_equal(_bits(sc[mask]), _bits(sc0[mask])) and (sc[~mask] == float("-inf")).all()


def test_constructor_refusals(rng):
    X, y = _data(rng)
    for kw in (dict(label_units=LABEL), dict(dimension_penalty=1.0), dict(input_units=UNITS, multigene=True),
               dict(input_units=UNITS, dimension_penalty=-1.0), dict(input_units=UNITS, dimension_penalty=float("nan")),
               dict(input_units=[[1, 0]]), dict(input_units=UNITS, label_units=[1]), dict(input_units=[[0.1, 0], [0, 1]])):
        with pytest.raises(ValueError):
            SymbolicRegression(datapoints=X, labels=y, **kw)
    with pytest.raises(ValueError):
        SymbolicRegression(datapoints=X, labels=torch.cat([y, y], dim=1), input_units=UNITS)
    with pytest.raises(ValueError):
        SymbolicRegression(datapoints=X, labels=y).dimensions(_forest())


def test_default_problem_calls_none_of_the_new_code(rng):
    X, y = _data(rng)
    forest = _forest()
    before = dict(cpu_dimension_ops.calls)
    prob = SymbolicRegression(datapoints=X, labels=y)
    assert prob.input_units is None and prob.label_units is None and prob.dimension_penalty is None
    fit = forest.SR_fitness(X, y)
    assert np.array_equal(_bits(prob.evaluate(forest)), _bits(-fit))
    SymbolicRegression(datapoints=X, labels=y, linear_scaling=True).scores(forest)
    SymbolicRegression(datapoints=X, labels=y, interval_check=True).scores(forest)
    assert cpu_dimension_ops.calls == before


def test_argument_errors_without_gpu():
    from evogp_amd import _lib

    L = _lib.lib
    p, q = 8, 16  # (never dereferenced: the host checks come first)
    call = L.evogp_hip_tree_dimensions
    assert call(0, 32, 3, 2, p, p, p, p, p, 1, q, q, q, None) == -1
    assert call(4, 0, 3, 2, p, p, p, p, p, 1, q, q, q, None) == -1
    assert call(4, 1025, 3, 2, p, p, p, p, p, 1, q, q, q, None) == -1
    assert call(4, 32, 0, 2, p, p, p, p, p, 1, q, q, q, None) == -1
    assert call(4, 32, 3, 0, p, p, p, p, p, 1, q, q, q, None) == -1
    assert call(4, 32, 3, 9, p, p, p, p, p, 1, q, q, q, None) == -1
    for k in range(4, 13):
        if k == 9:
            continue
        args = [4, 32, 3, 2, p, p, p, p, p, 0, q, q, q, None]
        args[k] = None
        assert call(*args) == -2, k
    assert L.evogp_hip_abi_version() == _lib.ABI_VERSION == 9


def test_both_import_roots():
    import evogp
    import evogp.problem
    import evogp.tree
    from evogp.tree.utils import check_units, str_unit as s2, unit_numerators
    import evogp_amd.ops

    assert evogp.tree.Forest is Forest and evogp.problem.SymbolicRegression is SymbolicRegression
    assert hasattr(evogp.tree.Forest, "SR_dimensions") and hasattr(evogp.tree.Forest, "dimension_mask")
    assert s2 is str_unit and evogp.tree.str_unit is str_unit and unit_numerators(Fraction(1, 2)) == 12600
    assert check_units(UNITS, None, 2) == ([[DEN, 0], [0, DEN]], [0, 0], False)
    assert callable(evogp_amd.ops.tree_dimensions)
    assert torch.ops.evogp_hip.tree_dimensions is not None
