"""CPU: the host logic of the structural constraints (tree.utils.parse_structure, Forest.SR_structure / structure_mask / complexity,
SymbolicRegression(max_depth=, max_complexity=, complexity_of=, nested_constraints=, operand_constraints=, structure_penalty=)) with the
integer restatement registered as a test-only CPU kernel (tests/cpu_structure_ops.py), and the argument checks of the new C entry
point, which return before any launch."""
import os
import sys

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
import cpu_structure_ops  # noqa: E402
import interval_cases as IC  # noqa: E402
import sr_grad_ref as R  # noqa: E402
import structure_ref as SR  # noqa: E402
from grad_trees import ALL_FUNCS, random_forest  # noqa: E402
from interval_cases import B, C, U, V  # noqa: E402

cpu_ops.register()
cpu_grad_ops.register()
cpu_dedup_ops.register()
cpu_scale_ops.register()
cpu_interval_ops.register()
cpu_dimension_ops.register()
cpu_structure_ops.register()

from evogp_amd.algorithm import NSGA2Selection  # noqa: E402
from evogp_amd.problem import SymbolicRegression  # noqa: E402
from evogp_amd.tree import Forest, set_default_device  # noqa: E402
from evogp_amd.tree import utils as _tree_utils  # noqa: E402
from evogp_amd.tree.utils import FUNCS_NAMES, parse_structure  # noqa: E402


@pytest.fixture(autouse=True)
def _cpu_default_device():
    saved = _tree_utils._DEVICE
    set_default_device("cpu")
    yield
    _tree_utils._DEVICE = saved


def _bits(t):
    return t.contiguous().numpy().view(np.uint32)


SIN, COS, POW, ADD, SUB, MUL, NEG = R.F_SIN, R.F_COS, R.F_POW, R.F_ADD, R.F_SUB, R.F_MUL, R.F_NEG
# no sine or cosine inside a sine; an exponent of one node; at most four levels; sin and cos cost 3 and a tree at most 9
OPTIONS = dict(nested_constraints={"sin": {"sin": 0, "cos": 0}}, operand_constraints={"pow": (-1, 1)}, max_depth=4,
               complexity_of={"sin": 3, "cos": 3}, max_complexity=9)
EXPRS = [
    B(ADD, V(0), V(1)),                                                    # passes
    U(SIN, U(SIN, V(0))),                                                  # a sine in a sine
    B(POW, V(0), B(ADD, V(1), V(1))),                                      # an exponent of three nodes
    B(MUL, U(SIN, U(COS, V(0))), V(1)),                                    # a cosine in a sine, at node 1; complexity 9, four levels
    B(ADD, V(0), B(MUL, V(1), B(SUB, V(0), U(NEG, V(1))))),                # five levels
    B(ADD, U(COS, V(0)), U(SIN, V(1))),                                    # passes: complexity 9
    B(POW, B(POW, V(0), C(2.0)), C(2.0)),                                  # passes
    B(ADD, U(SIN, V(0)), B(ADD, U(COS, V(1)), U(SIN, V(0)))),              # complexity 14
    U(SIN, U(SIN, B(POW, V(0), B(ADD, V(1), V(1))))),                      # nodes 0 and 2, five levels, complexity 11
]
VIOL = [0, 1, 1, 1, 1, 0, 0, 1, 4]
COMPLEXITY = [3, 7, 5, 9, 8, 9, 5, 14, 11]
SIZE = [3, 3, 5, 5, 8, 5, 5, 8, 7]


def _forest(exprs=EXPRS, L=16, var_len=2):
    return Forest(var_len, 1, *(torch.from_numpy(a) for a in IC.rows(exprs, L)))


def _data(rng, D=40):
    X = rng.uniform(0.5, 1.5, (D, 2)).astype(np.float32)
    y = (2.0 * X[:, :1] / X[:, 1:2] - 0.5).astype(np.float32)
    return torch.from_numpy(X), torch.from_numpy(y)


def test_parse_structure_tables():
    cost, oplim, rules = parse_structure()
    assert cost == [1] * 32 and oplim == [[-1, -1, -1]] * 32 and rules == []
    cost, oplim, rules = parse_structure({"sin": 3, "const": 2, "var": 0, "unknown": 65535, "if": 7},
                                         {"sin": {"sin": 0, "cos": 0}, "pow": {"pow": 1}, "unknown": {"var": 254}},
                                         {"pow": (-1, 1), "sin": 5, "if": (0, -1, 9), "cos": (4,), "unknown": (1, 2), "neg": [3]})
    want = [1] * 32
    want[SIN], want[SR.CONST], want[SR.VAR], want[SR.UNKNOWN], want[R.F_IF] = 3, 2, 0, 65535, 7
    assert cost == want
    assert rules == [(1 << SIN, 1 << SIN, 0), (1 << SIN, 1 << COS, 0), (1 << POW, 1 << POW, 1), (1 << 31, 1 << 29, 254)]
    lim = [[-1, -1, -1] for _ in range(32)]
    lim[POW], lim[SIN], lim[R.F_IF], lim[COS], lim[SR.UNKNOWN], lim[NEG] = [-1, 1, -1], [5, -1, -1], [0, -1, 9], [4, -1, -1], [1, 2, -1], [3, -1, -1]
    assert oplim == lim
    assert parse_structure(operand_constraints={"unknown": 4})[1][31] == [4, -1, -1]
    assert parse_structure(complexity_of={n: i for i, n in enumerate(FUNCS_NAMES)})[0][:29] == list(range(29))
    eight = {"sin": {n: 0 for n in FUNCS_NAMES[:8]}}
    assert len(parse_structure(nested_constraints=eight)[2]) == 8
    assert parse_structure(operand_constraints={"+": (2 ** 31 - 1, 0)})[1][ADD] == [2 ** 31 - 1, 0, -1]


@pytest.mark.parametrize("kw", [
    dict(complexity_of={"sine": 1}), dict(complexity_of={14: 1}), dict(complexity_of={"sin": True}), dict(complexity_of={"sin": 1.0}),
    dict(complexity_of={"sin": -1}), dict(complexity_of={"sin": 65536}), dict(complexity_of={"sin": None}),
    dict(nested_constraints={"sine": {"sin": 0}}), dict(nested_constraints={"sin": {"cosine": 0}}), dict(nested_constraints={"sin": 0}),
    dict(nested_constraints={"sin": {"sin": -1}}), dict(nested_constraints={"sin": {"sin": 255}}), dict(nested_constraints={"sin": {"sin": False}}),
    dict(nested_constraints={"sin": {"sin": 0.0}}),
    dict(nested_constraints={"sin": {n: 0 for n in FUNCS_NAMES[:9]}}),                                     # nine rules
    dict(nested_constraints={"sin": {n: 0 for n in FUNCS_NAMES[:5]}, "cos": {n: 0 for n in FUNCS_NAMES[:4]}}),
    dict(operand_constraints={"power": (-1, 1)}), dict(operand_constraints={"pow": 1}), dict(operand_constraints={"pow": (1,)}),
    dict(operand_constraints={"pow": (1, 1, 1)}), dict(operand_constraints={"sin": (1, 1)}), dict(operand_constraints={"if": (1, 1)}),
    dict(operand_constraints={"pow": (-2, 1)}), dict(operand_constraints={"pow": (True, 1)}), dict(operand_constraints={"pow": (0.5, 1)}),
    dict(operand_constraints={"pow": (2 ** 31, 1)}), dict(operand_constraints={"var": 1}), dict(operand_constraints={"const": ()}),
    dict(operand_constraints={"unknown": (1, 1, 1)}), dict(operand_constraints={"sin": ()}),
])
def test_parse_structure_errors(kw, rng):
    with pytest.raises(ValueError):
        parse_structure(**kw)
    n0 = cpu_structure_ops.calls["tree_structure"]
    with pytest.raises(ValueError):
        _forest().SR_structure(**kw)
    with pytest.raises(ValueError):
        _forest().structure_mask(**kw)
    X, y = _data(rng)
    with pytest.raises(ValueError):
        SymbolicRegression(datapoints=X, labels=y, **kw)
    assert cpu_structure_ops.calls["tree_structure"] == n0      # every fault fails on the host, before the op


def test_forest_argument_passing(rng):
    forest = _forest()
    out = forest.SR_structure(**OPTIONS)
    cx, ht, dp, nest, flags, viol = out
    assert [tuple(o.shape) for o in out] == [(9, 16), (9, 16), (9, 16), (9, 16, 2), (9, 16), (9,)]
    assert [o.dtype for o in out] == [torch.int32, torch.int16, torch.int16, torch.uint8, torch.uint8, torch.int32]
    assert viol.tolist() == VIOL and cx[:, 0].tolist() == COMPLEXITY
    last = cpu_structure_ops.last
    want_cost = np.ones(32, np.int32)
    want_cost[[SIN, COS]] = 3
    assert np.array_equal(last["cost"], want_cost) and last["operand_limit"][POW].tolist() == [-1, 1, -1] and (np.delete(last["operand_limit"], POW, 0) == -1).all()
    assert last["rule_outer"].tolist() == [1 << SIN, 1 << SIN] and last["rule_inner"].tolist() == [1 << SIN, 1 << COS] and last["rule_limit"].tolist() == [0, 0]
    assert last["max_depth"] == 4 and last["max_complexity"] == 9
    want = SR.forest_structure(*(a.numpy() for a in forest._tensors()), last["cost"], last["operand_limit"], last["rule_outer"], last["rule_inner"],
                               last["rule_limit"], 4, 9)
    for got, w in zip(out, want):
        assert np.array_equal(got.numpy(), w)
    # the defaults: unit costs, no rule (empty tensors), no limit
    plain = forest.SR_structure()
    assert cpu_structure_ops.last["rule_outer"].shape == (0,) and cpu_structure_ops.last["max_depth"] == -1 and cpu_structure_ops.last["max_complexity"] == -1
    assert plain[3].shape == (9, 16, 0) and plain[5].tolist() == [0] * 9 and plain[0][:, 0].tolist() == SIZE
    # symbol 31 in a set is bit 31 of an int32 word
    forest.SR_structure(nested_constraints={"unknown": {"unknown": 3}})
    assert cpu_structure_ops.last["rule_outer"].tolist() == [-(1 << 31)] and cpu_structure_ops.last["rule_inner"].tolist() == [-(1 << 31)]
    assert forest.structure_mask(**OPTIONS).tolist() == [v == 0 for v in VIOL] and forest.structure_mask(**OPTIONS).dtype == torch.bool
    assert forest.structure_mask(max_depth=2).tolist() == [True] + [False] * 8
    assert forest.complexity().tolist() == SIZE and forest.complexity({"sin": 3, "cos": 3}).tolist() == COMPLEXITY
    assert forest.complexity().dtype == torch.int32
    assert forest.SR_structure(max_depth=np.int64(4))[5].tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 1]
    n0 = cpu_structure_ops.calls["tree_structure"]
    for kw in (dict(max_depth=-1), dict(max_depth=True), dict(max_depth=2.0), dict(max_complexity=-1), dict(max_complexity="9"),
               dict(max_complexity=2 ** 31)):
        with pytest.raises(ValueError):
            forest.SR_structure(**kw)
        with pytest.raises(ValueError):
            forest.structure_mask(**kw)
    multi = Forest(2, 3, *(torch.from_numpy(a) for a in random_forest(rng, 4, 32, ALL_FUNCS, 2, 3, max_depth=3)))
    for call in (multi.SR_structure, multi.structure_mask, multi.complexity):
        with pytest.raises(ValueError, match="single-output"):
            call()
    assert cpu_structure_ops.calls["tree_structure"] == n0


@pytest.mark.parametrize("mode", ["auto", "torch"])
def test_hard_constraint(mode, rng):
    X, y = _data(rng)
    forest = _forest()
    plain = SymbolicRegression(datapoints=X, labels=y, execute_mode=mode)
    prob = SymbolicRegression(datapoints=X, labels=y, execute_mode=mode, **OPTIONS)
    assert prob.structure_penalty is None and prob.max_depth == 4 and prob.max_complexity == 9
    mask = prob.structure_mask(forest)
    assert mask.tolist() == [v == 0 for v in VIOL] and prob.structure(forest)[5].tolist() == VIOL
    assert prob.complexity(forest).tolist() == COMPLEXITY and plain.complexity(forest).tolist() == SIZE
    ev0, sc0 = plain.evaluate(forest), plain.scores(forest)
    assert torch.isfinite(ev0).all()                 # every tree scores on the rows: the structure is what removes them
    n0 = cpu_structure_ops.calls["tree_structure"]
    ev, sc = prob.evaluate(forest), prob.scores(forest)
    assert cpu_structure_ops.calls["tree_structure"] == n0 + 2
    assert np.array_equal(_bits(ev[mask]), _bits(ev0[mask])) and np.array_equal(_bits(sc[mask]), _bits(sc0[mask]))     # bit for bit
    assert torch.isnan(ev[~mask]).all() and (sc[~mask] == float("-inf")).all()
    # each option alone is a structural option
    for kw, want in ((dict(max_depth=4), [0, 0, 0, 0, 1, 0, 0, 0, 1]), (dict(max_complexity=7), [0, 0, 0, 0, 1, 0, 0, 1, 0]),
                     (dict(nested_constraints={"sin": {"sin": 0}}), [0, 1, 0, 0, 0, 0, 0, 0, 1]),
                     (dict(operand_constraints={"pow": (-1, 1)}), [0, 0, 1, 0, 0, 0, 0, 0, 1])):
        one = SymbolicRegression(datapoints=X, labels=y, execute_mode=mode, **kw)
        assert one.structure(forest)[5].tolist() == want
        assert (one.scores(forest) == float("-inf")).tolist() == [v > 0 for v in want]


def test_soft_penalty(rng):
    X, y = _data(rng)
    forest = _forest()
    plain = SymbolicRegression(datapoints=X, labels=y)
    prob = SymbolicRegression(datapoints=X, labels=y, structure_penalty=0.25, **OPTIONS)
    viol = torch.tensor(VIOL)
    ev0, sc0 = plain.evaluate(forest), plain.scores(forest)
    ev, sc = prob.evaluate(forest), prob.scores(forest)
    ok = viol == 0
    assert np.array_equal(_bits(ev[ok]), _bits(ev0[ok])) and np.array_equal(_bits(sc[ok]), _bits(sc0[ok]))     # bit for bit
    assert torch.equal(ev[~ok], ev0[~ok] - 0.25 * viol[~ok].float()) and torch.equal(sc[~ok], sc0[~ok] - 0.25 * viol[~ok].float())
    zero = SymbolicRegression(datapoints=X, labels=y, structure_penalty=0, **OPTIONS)
    assert np.array_equal(_bits(zero.scores(forest)), _bits(sc0))
    # a malformed row (violations = -1) is treated as in the hard case, whatever the penalty
    value, type_, size = (torch.from_numpy(a) for a in IC.rows(EXPRS[:3], 16))
    size[2, 0] = 2
    broken = Forest(2, 1, value, type_, size)
    assert prob.structure(broken)[5].tolist() == [0, 1, -1]
    fit = torch.tensor([-1.0, -2.0, -3.0])
    assert prob._masked(broken, fit, float("-inf")).tolist() == [-1.0, -2.25, float("-inf")]
    assert torch.isnan(prob._masked(broken, fit, float("nan"))[2])
    hard = SymbolicRegression(datapoints=X, labels=y, **OPTIONS)
    assert hard._masked(broken, fit, float("-inf")).tolist() == [-1.0, float("-inf"), float("-inf")]


@pytest.mark.parametrize("penalty", [None, 0.5])
def test_combined_with_the_interval_check_and_units(penalty, rng):
    X, y = _data(rng)
    forest = _forest()
    plain = SymbolicRegression(datapoints=X, labels=y)
    box = SymbolicRegression(datapoints=X, labels=y, interval_check=True, input_bounds=(-1.0, 2.0))
    units = SymbolicRegression(datapoints=X, labels=y, input_units=[[0], [1]])
    safe, consistent = box.safe_mask(forest), units.dimension_mask(forest)
    assert 0 < safe.sum() < 9 and 0 < consistent.sum() < 9      # (a negative base under a fractional exponent; a number plus seconds)
    viol = torch.tensor(VIOL)
    prob = SymbolicRegression(datapoints=X, labels=y, interval_check=True, input_bounds=(-1.0, 2.0), input_units=[[0], [1]],
                              structure_penalty=penalty, **OPTIONS)
    n = [cpu_interval_ops.calls["tree_intervals"], cpu_dimension_ops.calls["tree_dimensions"], cpu_structure_ops.calls["tree_structure"]]
    sc, sc0 = prob.scores(forest), plain.scores(forest)
    assert [cpu_interval_ops.calls["tree_intervals"], cpu_dimension_ops.calls["tree_dimensions"], cpu_structure_ops.calls["tree_structure"]] == [k + 1 for k in n]
    other = safe & consistent
    if penalty is None:
        keep = other & (viol == 0)
        assert keep.any() and (other & (viol > 0)).any()
        assert np.array_equal(_bits(sc[keep]), _bits(sc0[keep])) and (sc[~keep] == float("-inf")).all()
        assert torch.isnan(prob.evaluate(forest)[~keep]).all()
    else:
        assert (sc[~other] == float("-inf")).all() and torch.equal(sc[other], sc0[other] - penalty * viol[other].float())
    # a soft unit penalty under a hard structure
    soft = SymbolicRegression(datapoints=X, labels=y, input_units=[[0], [1]], dimension_penalty=0.5, **OPTIONS)
    dviol = units.dimensions(forest)[2]
    keep = viol == 0
    got = soft.scores(forest)
    assert (got[~keep] == float("-inf")).all() and torch.equal(got[keep], sc0[keep] - 0.5 * dviol[keep].float())


def test_linear_scaling_and_semantic_dedup_compose(rng):
    X, y = _data(rng)
    forest = _forest()
    plain = SymbolicRegression(datapoints=X, labels=y, linear_scaling=True)
    prob = SymbolicRegression(datapoints=X, labels=y, linear_scaling=True, **OPTIONS)
    mask = torch.tensor(VIOL) == 0
    sc, sc0 = prob.scores(forest), plain.scores(forest)
    assert np.array_equal(_bits(sc[mask]), _bits(sc0[mask])) and (sc[~mask] == float("-inf")).all()


def test_constructor_refusals(rng):
    X, y = _data(rng)
    for kw in (dict(structure_penalty=1.0), dict(structure_penalty=1.0, complexity_of={"sin": 2}), dict(max_depth=4, structure_penalty=-1.0),
               dict(max_depth=4, structure_penalty=float("nan")), dict(max_depth=4, structure_penalty=True), dict(max_depth=4, multigene=True),
               dict(max_complexity=4, multigene=True), dict(nested_constraints={"sin": {"sin": 0}}, multigene=True),
               dict(operand_constraints={"sin": 1}, multigene=True), dict(complexity_of={"sin": 2}, multigene=True),
               dict(max_depth=-1), dict(max_depth=True), dict(max_depth=2.5), dict(max_complexity=-3), dict(max_complexity=2 ** 31)):
        with pytest.raises(ValueError):
            SymbolicRegression(datapoints=X, labels=y, **kw)
    with pytest.raises(ValueError, match="structure_penalty needs"):
        SymbolicRegression(datapoints=X, labels=y, structure_penalty=0.5)
    with pytest.raises(ValueError, match="multigene cannot be combined"):
        SymbolicRegression(datapoints=X, labels=y, multigene=True, max_depth=3)
    with pytest.raises(ValueError):
        SymbolicRegression(datapoints=X, labels=torch.cat([y, y], dim=1), max_depth=3)
    for prob in (SymbolicRegression(datapoints=X, labels=y), SymbolicRegression(datapoints=X, labels=y, complexity_of={"sin": 2})):
        for call in (prob.structure, prob.structure_mask):
            with pytest.raises(ValueError, match="this problem has no"):
                call(_forest())
    multi = Forest(2, 3, *(torch.from_numpy(a) for a in random_forest(rng, 4, 32, ALL_FUNCS, 2, 3, max_depth=3)))
    prob = SymbolicRegression(datapoints=X, labels=y, max_depth=3)
    for call in (prob.structure, prob.structure_mask, prob.complexity):
        with pytest.raises(ValueError, match="single-output"):
            call(multi)


def test_nsga2_takes_the_problem_complexity(rng):
    X, y = _data(rng)
    forest = _forest()
    prob = SymbolicRegression(datapoints=X, labels=y, complexity_of={"sin": 3, "cos": 3})
    sel = NSGA2Selection(complexity=prob.complexity, max_complexity=64)
    err, cx, bound = sel.objectives(forest, prob.scores(forest))
    assert cx.dtype == torch.int32 and cx.is_contiguous() and cx.tolist() == COMPLEXITY and bound == 64
    assert torch.equal(err, -prob.scores(forest))
    err, cx, bound = NSGA2Selection(complexity=Forest.complexity, max_complexity=16).objectives(forest, prob.scores(forest))
    assert cx.tolist() == SIZE     # Forest.complexity itself has the signature too


def test_default_problem_calls_none_of_the_new_code(rng):
    X, y = _data(rng)
    forest = _forest()
    before = dict(cpu_structure_ops.calls)
    prob = SymbolicRegression(datapoints=X, labels=y)
    assert prob.max_depth is None and prob.max_complexity is None and prob.structure_penalty is None
    fit = forest.SR_fitness(X, y)
    assert np.array_equal(_bits(prob.evaluate(forest)), _bits(-fit))
    SymbolicRegression(datapoints=X, labels=y, linear_scaling=True).scores(forest)
    SymbolicRegression(datapoints=X, labels=y, interval_check=True).scores(forest)
    SymbolicRegression(datapoints=X, labels=y, input_units=[[0], [1]]).scores(forest)
    SymbolicRegression(datapoints=X, labels=y, complexity_of={"sin": 2}).scores(forest)      # costs alone constrain nothing
    assert cpu_structure_ops.calls == before


def test_argument_errors_without_gpu():
    from evogp_amd import _lib

    L = _lib.lib
    p, q = 8, 16  # (never dereferenced: the host checks come first)
    call = L.evogp_hip_tree_structure
    good = [4, 32, 2, p, p, p, p, p, p, p, p, -1, -1, q, q, q, q, q, q, None]
    for k, bad in ((0, 0), (1, 0), (1, 1025), (2, 9), (11, -2), (12, -2), (16, 20)):      # (16: nest, not 8-byte aligned)
        args = list(good)
        args[k] = bad
        assert call(*args) == -1, (k, bad)
    for k in list(range(3, 11)) + list(range(13, 19)):
        args = list(good)
        args[k] = None
        assert call(*args) == -2, k
    # no rules: the rule pointers and nest may be null, nothing else
    none = [4, 32, 0, p, p, p, p, p, None, None, None, -1, -1, q, q, q, None, q, q, None]
    for k in (3, 4, 5, 6, 7, 13, 14, 15, 17, 18):
        args = list(none)
        args[k] = None
        assert call(*args) == -2, k
    assert L.evogp_hip_abi_version() == _lib.ABI_VERSION == 9


def test_both_import_roots():
    import evogp
    import evogp.problem
    import evogp.tree
    from evogp.tree.utils import parse_structure as p2
    import evogp_amd.ops

    assert evogp.tree.Forest is Forest and evogp.problem.SymbolicRegression is SymbolicRegression
    assert all(hasattr(evogp.tree.Forest, n) for n in ("SR_structure", "structure_mask", "complexity"))
    assert p2 is parse_structure and callable(evogp_amd.ops.tree_structure)
    assert torch.ops.evogp_hip.tree_structure is not None
