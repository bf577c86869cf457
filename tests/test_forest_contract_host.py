"""CPU: the exception contract of the host layer, as one table.  For every public Forest method that takes a dataset, a box, units or
constraints, and for every check of SymbolicRegression's constructor, one offending input and the exception TYPE it raises: which
methods assert and which raise ValueError is part of the interface, and the per-feature tests cover it only in part.  Every check
fires before the first launch, so the forests are tiny (pop 4, 8 words, 2 inputs, 4 rows) and nothing is computed."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cpu_dedup_ops  # noqa: E402
import cpu_ops  # noqa: E402

cpu_ops.register()
cpu_dedup_ops.register()

from evogp_amd.problem import SymbolicRegression  # noqa: E402
from evogp_amd.tree import Forest, set_default_device  # noqa: E402
from evogp_amd.tree import utils as _tree_utils  # noqa: E402

POP, L, VARS, ROWS = 4, 8, 2, 4


@pytest.fixture(autouse=True)
def _cpu_default_device():
    saved = _tree_utils._DEVICE
    set_default_device("cpu")
    yield
    _tree_utils._DEVICE = saved


def _forest(output_len=1):
    """four copies of the tree ``x0``"""
    size = torch.zeros((POP, L), dtype=torch.int16)
    size[:, 0] = 1
    return Forest(VARS, output_len, torch.zeros((POP, L), dtype=torch.float32), torch.zeros((POP, L), dtype=torch.int16), size)


X = torch.linspace(0.5, 1.5, ROWS * VARS).reshape(ROWS, VARS)
Y = X[:, :1] + X[:, 1:]
Y2 = torch.cat([Y, Y], dim=1)
X3 = torch.ones(ROWS, VARS + 1)          # one column too many
ONES = torch.ones(POP)
UNITS = [[1, 0], [0, 1]]

# (name, output_len of the forest, call, exception type, fragment of the message or None)
FOREST_CASES = [
    # ---- a two-output forest where one output is required: the five that assert ...
    ("normal_eq/multi", 2, lambda f: f.SR_normal_equations(X, Y2), AssertionError, "single-output"),
    ("subtree/multi", 2, lambda f: f.SR_subtree_errors(X, Y2), AssertionError, "single-output"),
    ("simplify/multi", 2, lambda f: f.simplify(X, Y2), AssertionError, "single-output"),
    ("simplify-dedup/multi", 2, lambda f: f.simplify(X, Y2, dedup=True), AssertionError, "single-output"),
    ("scaled/multi", 2, lambda f: f.SR_scaled_fitness(X, Y2), AssertionError, "single-output"),
    ("scaled-dedup/multi", 2, lambda f: f.SR_scaled_fitness(X, Y2, dedup=True), AssertionError, "single-output"),
    ("apply_scaling/multi", 2, lambda f: f.apply_scaling(ONES, ONES), AssertionError, "single-output"),
    # ---- ... and the ones that raise ValueError
    ("semantic_hash/multi", 2, lambda f: f.semantic_hash(X), ValueError, "single-output"),
    ("semantic_classes/multi", 2, lambda f: f.semantic_classes(X), ValueError, "single-output"),
    ("semantic_unique/multi", 2, lambda f: f.semantic_unique(X), ValueError, "single-output"),
    ("intervals/multi", 2, lambda f: f.SR_intervals(-1.0, 1.0), ValueError, "single-output"),
    ("safe_mask/multi", 2, lambda f: f.safe_mask(-1.0, 1.0), ValueError, "single-output"),
    ("derivatives/multi", 2, lambda f: f.SR_derivative_intervals(-1.0, 1.0), ValueError, "single-output"),
    ("monotone_mask/multi", 2, lambda f: f.monotone_mask(-1.0, 1.0, {0: 1}), ValueError, "single-output"),
    ("dimensions/multi", 2, lambda f: f.SR_dimensions(UNITS), ValueError, "single-output"),
    ("dimension_mask/multi", 2, lambda f: f.dimension_mask(UNITS), ValueError, "single-output"),
    ("lm/multi", 2, lambda f: f.optimize_constants(X, Y2, 1, method="lm"), ValueError, "single-output"),
    ("lm-dedup/multi", 2, lambda f: f.optimize_constants(X, Y2, 1, method="lm", dedup=True), ValueError, "single-output"),
    ("genes/nine outputs", 9, lambda f: f.SR_gene_fitness(X, Y), ValueError, "outputs"),
    ("gene_moments/nine outputs", 9, lambda f: f.SR_gene_moments(X, Y), ValueError, "outputs"),
    # ---- inputs of the wrong shape: the dataset prologue asserts, the semantic and the gene prologues raise
    ("fitness/inputs", 1, lambda f: f.SR_fitness(X3, Y), AssertionError, "inputs shape"),
    ("fitness/labels", 1, lambda f: f.SR_fitness(X, Y2), AssertionError, "outputs shape"),
    ("fitness/mode", 1, lambda f: f.SR_fitness(X, Y, execute_mode="fast"), AssertionError, "execute_mode"),
    ("forward/x", 1, lambda f: f.forward(X3), AssertionError, "x shape"),
    ("batch_forward/x", 1, lambda f: f.batch_forward(X3), AssertionError, "x shape"),
    ("case_errors/inputs", 1, lambda f: f.SR_case_errors(X3, Y), AssertionError, "inputs shape"),
    ("gradient/inputs", 1, lambda f: f.SR_gradient(X3, Y), AssertionError, "inputs shape"),
    ("gradient/labels", 1, lambda f: f.SR_gradient(X, Y2), AssertionError, "outputs shape"),
    ("normal_eq/inputs", 1, lambda f: f.SR_normal_equations(X3, Y), AssertionError, "inputs shape"),
    ("descent/inputs", 1, lambda f: f.optimize_constants(X3, Y, 1), AssertionError, "inputs shape"),
    ("lm/inputs", 1, lambda f: f.optimize_constants(X3, Y, 1, method="lm"), AssertionError, "inputs shape"),
    ("subtree/inputs", 1, lambda f: f.SR_subtree_errors(X3, Y), AssertionError, "inputs shape"),
    ("simplify/inputs", 1, lambda f: f.simplify(X3, Y), AssertionError, "inputs shape"),
    ("scaled/inputs", 1, lambda f: f.SR_scaled_fitness(X3, Y), AssertionError, "inputs shape"),
    ("semantic_hash/inputs", 1, lambda f: f.semantic_hash(X3), ValueError, "inputs shape"),
    ("semantic_classes/no rows", 1, lambda f: f.semantic_classes(X[:0]), ValueError, "inputs shape"),
    ("semantic_unique/inputs", 1, lambda f: f.semantic_unique(X3), ValueError, "inputs shape"),
    ("genes/inputs", 2, lambda f: f.SR_gene_fitness(X3, Y), ValueError, "inputs shape"),
    ("genes/labels", 2, lambda f: f.SR_gene_fitness(X, Y2), ValueError, "labels shape"),
    ("gene_moments/inputs", 2, lambda f: f.SR_gene_moments(X3, Y), ValueError, "inputs shape"),
    ("gene_predict/coef", 2, lambda f: f.gene_predict(X, torch.ones(POP, 2)), ValueError, "coef shape"),
    ("apply_scaling/shape", 1, lambda f: f.apply_scaling(ONES[:3], ONES), AssertionError, "slope and intercept"),
    # ---- keep, method, steps
    ("semantic_classes/keep", 1, lambda f: f.semantic_classes(X, keep="largest"), ValueError, "keep"),
    ("semantic_unique/keep", 1, lambda f: f.semantic_unique(X, keep="largest"), ValueError, "keep"),
    ("semantic_classes/keep before outputs", 2, lambda f: f.semantic_classes(X, keep="largest"), ValueError, "keep"),
    ("optimize/method", 1, lambda f: f.optimize_constants(X, Y, 1, method="newton"), ValueError, "method"),
    ("optimize-dedup/method", 1, lambda f: f.optimize_constants(X, Y, 1, method="newton", dedup=True), ValueError, "method"),
    ("optimize/steps", 1, lambda f: f.optimize_constants(X, Y, -1), AssertionError, "steps"),
    ("lm/MAE", 1, lambda f: f.optimize_constants(X, Y, 1, use_MSE=False, method="lm"), ValueError, "use_MSE"),
    ("lm/MAE before outputs", 2, lambda f: f.optimize_constants(X, Y2, 1, use_MSE=False, method="lm"), ValueError, "use_MSE"),
    # ---- the box, the variables, the constraints, the units
    ("intervals/order", 1, lambda f: f.SR_intervals(1.0, -1.0), ValueError, "lower"),
    ("intervals/length", 1, lambda f: f.SR_intervals(torch.zeros(3), torch.ones(3)), ValueError, "bounds"),
    ("safe_mask/finite", 1, lambda f: f.safe_mask(float("-inf"), 1.0), ValueError, "finite"),
    ("derivatives/box", 1, lambda f: f.SR_derivative_intervals(0.0, float("nan")), ValueError, "finite"),
    ("derivatives/wrt range", 1, lambda f: f.SR_derivative_intervals(-1.0, 1.0, wrt=[2]), ValueError, "wrt"),
    ("derivatives/wrt empty", 1, lambda f: f.SR_derivative_intervals(-1.0, 1.0, wrt=[]), ValueError, "wrt"),
    ("monotone_mask/empty", 1, lambda f: f.monotone_mask(-1.0, 1.0, {}), ValueError, None),
    ("monotone_mask/sign", 1, lambda f: f.monotone_mask(-1.0, 1.0, {0: 2}), ValueError, None),
    ("monotone_mask/word", 1, lambda f: f.monotone_mask(-1.0, 1.0, {0: "up"}), ValueError, None),
    ("monotone_mask/pair order", 1, lambda f: f.monotone_mask(-1.0, 1.0, {0: (1.0, -1.0)}), ValueError, None),
    ("monotone_mask/variable", 1, lambda f: f.monotone_mask(-1.0, 1.0, {2: 1}), ValueError, None),
    ("monotone_mask/box", 1, lambda f: f.monotone_mask(1.0, -1.0, {0: 1}), ValueError, "lower"),
    ("dimensions/rows", 1, lambda f: f.SR_dimensions([[1, 0]]), ValueError, "input_units"),
    ("dimensions/exponent", 1, lambda f: f.SR_dimensions([[1, 0], [0, "m"]]), ValueError, None),
    ("dimension_mask/label", 1, lambda f: f.dimension_mask(UNITS, [1]), ValueError, "label_units"),
]


@pytest.mark.parametrize("output_len, call, error, fragment", [pytest.param(*c[1:], id=c[0]) for c in FOREST_CASES])
def test_forest_method_raises(output_len, call, error, fragment):
    with pytest.raises(error, match=fragment) as caught:
        call(_forest(output_len))
    assert caught.type is error          # the type itself, not a subclass of it


def _problem(labels=Y, **kw):
    return SymbolicRegression(datapoints=X, labels=labels, **kw)


# (name, labels, keywords, exception type, fragment of the message or None); the last block holds inputs that fail TWO checks, and
# the fragment there says which of them fires
PROBLEM_CASES = [
    # ---- the four asserts
    ("execute_mode", Y, dict(execute_mode="fast"), AssertionError, "execute_mode"),
    ("const_opt_steps", Y, dict(const_opt_steps=-1), AssertionError, "const_opt_steps"),
    ("const_opt_method", Y, dict(const_opt_method="newton"), AssertionError, "const_opt_method"),
    ("simplify_every", Y, dict(simplify_every=-1), AssertionError, "simplify_every"),
    # ---- two label columns under a single-output feature
    ("linear_scaling/two columns", Y2, dict(linear_scaling=True), ValueError, "linear_scaling works on single-output"),
    ("interval_check/two columns", Y2, dict(interval_check=True), ValueError, "interval_check works on single-output"),
    ("monotonic/two columns", Y2, dict(monotonic={0: 1}), ValueError, "monotonic works on single-output"),
    ("input_units/two columns", Y2, dict(input_units=UNITS), ValueError, "input_units works on single-output"),
    ("semantic_dedup/two columns", Y2, dict(semantic_dedup=True), ValueError, "semantic_dedup works on single-output"),
    ("multigene/two columns", Y2, dict(multigene=True), ValueError, "multigene fits one label column"),
    ("linear_scaling/flat labels", Y[:, 0], dict(linear_scaling=True), ValueError, "single-output"),
    # ---- the box and the constraints
    ("input_bounds/word", Y, dict(interval_check=True, input_bounds="box"), ValueError, "input_bounds"),
    ("input_bounds/word, monotonic", Y, dict(monotonic={0: 1}, input_bounds="box"), ValueError, "input_bounds"),
    ("monotonic/empty", Y, dict(monotonic={}), ValueError, "at least one"),
    ("monotonic/sign", Y, dict(monotonic={0: 3}), ValueError, None),
    ("monotonic/zero", Y, dict(monotonic={0: 0}), ValueError, None),
    ("monotonic/pair order", Y, dict(monotonic={0: (2.0, 1.0)}), ValueError, None),
    ("monotonic/triple", Y, dict(monotonic={0: (0.0, 1.0, 2.0)}), ValueError, None),
    ("monotonic/variable", Y, dict(monotonic={2: 1}), ValueError, "variable"),
    ("monotonic/negative variable", Y, dict(monotonic={-1: 1}), ValueError, "variable"),
    ("monotonic/named variable", Y, dict(monotonic={"x0": 1}), ValueError, "variable"),
    # ---- units
    ("label_units alone", Y, dict(label_units=[1, 0]), ValueError, "need input_units"),
    ("dimension_penalty alone", Y, dict(dimension_penalty=1.0), ValueError, "need input_units"),
    ("dimension_penalty/negative", Y, dict(input_units=UNITS, dimension_penalty=-1.0), ValueError, "dimension_penalty"),
    ("dimension_penalty/bool", Y, dict(input_units=UNITS, dimension_penalty=True), ValueError, "dimension_penalty"),
    ("input_units/rows", Y, dict(input_units=[[1, 0]]), ValueError, "input_units"),
    ("label_units/length", Y, dict(input_units=UNITS, label_units=[1]), ValueError, "label_units"),
    # ---- multigene with each option it excludes
    ("multigene + linear_scaling", Y, dict(multigene=True, linear_scaling=True), ValueError, "combined with linear_scaling"),
    ("multigene + const_opt_steps", Y, dict(multigene=True, const_opt_steps=1), ValueError, "combined with const_opt_steps"),
    ("multigene + simplify_every", Y, dict(multigene=True, simplify_every=1), ValueError, "combined with simplify_every"),
    ("multigene + interval_check", Y, dict(multigene=True, interval_check=True), ValueError, "combined with interval_check"),
    ("multigene + monotonic", Y, dict(multigene=True, monotonic={0: 1}), ValueError, "combined with monotonic"),
    ("multigene + input_units", Y, dict(multigene=True, input_units=UNITS), ValueError, "combined with input_units"),
    ("multigene + semantic_dedup", Y, dict(multigene=True, semantic_dedup=True), ValueError, "combined with semantic_dedup"),
    ("semantic_keep", Y, dict(semantic_keep="largest"), ValueError, "semantic_keep"),
    # ---- two checks apply: the earlier one fires (scaling, interval, monotonic, multigene, units, semantic_keep, semantic_dedup)
    ("scaling before interval", Y2, dict(linear_scaling=True, interval_check=True), ValueError, "linear_scaling works"),
    ("interval before monotonic", Y2, dict(interval_check=True, monotonic={0: 1}), ValueError, "interval_check works"),
    ("columns before constraints", Y2, dict(monotonic={}), ValueError, "monotonic works on single-output"),
    ("monotonic before multigene", Y, dict(monotonic={0: 3}, multigene=True), ValueError, "must be"),
    ("multigene: scaling before dedup", Y, dict(multigene=True, linear_scaling=True, semantic_dedup=True), ValueError,
     "combined with linear_scaling"),
    ("multigene before units", Y, dict(multigene=True, simplify_every=1, input_units=UNITS), ValueError, "combined with simplify_every"),
    ("units before semantic_keep", Y, dict(label_units=[1, 0], semantic_keep="largest"), ValueError, "need input_units"),
    ("semantic_keep before semantic_dedup", Y2, dict(semantic_dedup=True, semantic_keep="largest"), ValueError, "semantic_keep"),
    ("assert before ValueError", Y2, dict(linear_scaling=True, simplify_every=-1), AssertionError, "simplify_every"),
]


@pytest.mark.parametrize("labels, kw, error, fragment", [pytest.param(*c[1:], id=c[0]) for c in PROBLEM_CASES])
def test_problem_constructor_raises(labels, kw, error, fragment):
    with pytest.raises(error, match=fragment) as caught:
        _problem(labels, **kw)
    assert caught.type is error


def test_constructor_without_data_or_function_asserts():
    with pytest.raises(AssertionError, match="func and num_inputs"):
        SymbolicRegression()
    with pytest.raises(AssertionError, match="func and num_inputs"):
        SymbolicRegression(datapoints=X)


def test_problem_methods_without_their_option_raise():
    plain = _problem()
    for call in (plain.monotone_mask, plain.dimensions, plain.dimension_mask):
        with pytest.raises(ValueError, match="this problem has no"):
            call(_forest())
    for kw in (dict(linear_scaling=True), dict(multigene=True)):
        prob = _problem(**kw)
        for call in (prob.evaluate, prob.scores):
            with pytest.raises(ValueError, match="use_MSE"):
                call(_forest(), use_MSE=False)


def test_the_tiny_inputs_are_accepted():
    """the other half of the table: with nothing wrong, the same forests and the same data go through"""
    f = _forest()
    assert f.SR_fitness(X, Y).shape == (POP,) and f.batch_forward(X).shape == (POP, ROWS, 1)
    class_id, is_first = f.duplicate_classes()
    assert class_id.tolist() == [0] * POP and is_first.tolist() == [True, False, False, False]
    prob = _problem(linear_scaling=True, interval_check=True, monotonic={0: 1, 1: (-1.0, 2.0)}, input_units=UNITS, label_units=[1, 0],
                    semantic_dedup=True, input_bounds=(0.0, torch.tensor([2.0, 3.0])), input_margin=0.5)
    assert prob.monotonic == {0: 1, 1: (-1.0, 2.0)} and prob.input_lower.tolist() == [-1.0, -1.5] and prob.input_upper.tolist() == [3.0, 4.5]
    assert _problem(multigene=True).multigene and _problem(Y2).solution_dim == 2
