"""CPU: the host logic of multi-gene fitness (Forest.SR_gene_fitness / SR_gene_moments / gene_predict, SymbolicRegression(multigene=),
StandardPipeline.best_coef) with the numpy restatement registered as test-only CPU kernels (tests/cpu_gene_ops.py), and the argument
checks of the new C entry point, which return before any launch."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cpu_dedup_ops  # noqa: E402
import cpu_gene_ops  # noqa: E402
import cpu_grad_ops  # noqa: E402
import cpu_ops  # noqa: E402
import cpu_scale_ops  # noqa: E402
import gene_ref as GR  # noqa: E402
from grad_trees import ALL_FUNCS, ARITH, random_forest  # noqa: E402

cpu_ops.register()
cpu_grad_ops.register()
cpu_dedup_ops.register()
cpu_scale_ops.register()
cpu_gene_ops.register()

from evogp_amd.problem import SymbolicRegression  # noqa: E402
from evogp_amd.tree import Forest, GenerateDescriptor, set_default_device  # noqa: E402
from evogp_amd.tree import utils as _tree_utils  # noqa: E402

D = 40


@pytest.fixture(autouse=True)
def _cpu_default_device():
    saved = _tree_utils._DEVICE
    set_default_device("cpu")
    yield
    _tree_utils._DEVICE = saved


def _data(rng, var_len=2):
    X = rng.uniform(0.5, 1.5, (D, var_len)).astype(np.float32)
    y = (2.0 * X[:, :1] * X[:, 1:2] - 0.5 * X[:, :1]).astype(np.float32)
    return torch.from_numpy(X), torch.from_numpy(y)


def _forest(rng, pop=30, G=3, funcs=ARITH):
    value, type_, size = random_forest(rng, pop, 32, funcs, 2, G, max_depth=4)
    return Forest(2, G, *(torch.from_numpy(a) for a in (value, type_, size)))


def _bits(t):
    return t.contiguous().numpy().view(np.uint32)


def _ref(forest, X, y):
    return GR.fit(cpu_gene_ops.outputs(*(a.numpy() for a in forest._tensors()), X.numpy(), forest.output_len), y.numpy())


def test_default_problem_calls_none_of_the_new_ops(rng):
    forest = _forest(rng, G=1)
    X, y = _data(rng)
    before = dict(cpu_gene_ops.calls)
    prob = SymbolicRegression(datapoints=X, labels=y)
    assert prob.multigene is False
    fit = forest.SR_fitness(X, y)
    assert np.array_equal(_bits(prob.evaluate(forest)), _bits(-fit))
    assert np.array_equal(_bits(prob.scores(forest)), _bits(torch.where(torch.isnan(fit), torch.full_like(fit, float("-inf")), -fit)))
    SymbolicRegression(datapoints=X, labels=y, linear_scaling=True).scores(forest)
    assert cpu_gene_ops.calls == before


def test_value_errors(rng):
    X, y = _data(rng)
    with pytest.raises(ValueError):
        SymbolicRegression(datapoints=X, labels=torch.cat([y, y], dim=1), multigene=True)
    with pytest.raises(ValueError):
        SymbolicRegression(datapoints=X, labels=y[:, 0], multigene=True)
    for other in (dict(linear_scaling=True), dict(const_opt_steps=2), dict(simplify_every=1), dict(interval_check=True), dict(monotonic={0: 1})):
        with pytest.raises(ValueError):
            SymbolicRegression(datapoints=X, labels=y, multigene=True, **other)
    prob = SymbolicRegression(datapoints=X, labels=y, multigene=True)
    forest = _forest(rng, 4)
    with pytest.raises(ValueError):
        prob.evaluate(forest, use_MSE=False)
    with pytest.raises(ValueError):
        prob.scores(forest, use_MSE=False)
    assert prob.optimize(forest) is forest
    wide = Forest(2, 9, *(torch.from_numpy(a) for a in random_forest(rng, 4, 32, ARITH, 2, 9, max_depth=3)))
    for call in (wide.SR_gene_fitness, wide.SR_gene_moments):
        with pytest.raises(ValueError):
            call(X, y)
    for call in (forest.SR_gene_fitness, forest.SR_gene_moments):
        with pytest.raises(ValueError):
            call(X, torch.zeros(D, 3))        # one label column, not one per output
        with pytest.raises(ValueError):
            call(X[:, :1], y)
    with pytest.raises(ValueError):
        forest.gene_predict(X, torch.zeros(4, 3))


def test_gene_fitness_moments_dedup_and_predict(rng):
    forest = _forest(rng, 40, 3, ALL_FUNCS)
    forest.batch_subtree_size[3, 0] = 0   # malformed
    X, y = _data(rng)
    ref = _ref(forest, X, y)
    n0 = dict(cpu_gene_ops.calls)
    loss, coef = forest.SR_gene_fitness(X, y)
    assert cpu_gene_ops.calls == dict(n0, gene_fitness=n0["gene_fitness"] + 1)
    assert loss.shape == (40,) and coef.shape == (40, 4) and loss.dtype == coef.dtype == torch.float32
    # (the CPU stand-in IS the restatement: this checks the plumbing, tests/test_gpu_genes.py checks the arithmetic on the device)
    with np.errstate(over="ignore"):
        assert np.array_equal(_bits(loss), ref["loss"].astype(np.float32).view(np.uint32))
        assert np.array_equal(_bits(coef), ref["coef"].astype(np.float32).view(np.uint32))
    assert np.isnan(float(loss[3])) and np.isfinite(loss.numpy()).sum() > 20
    l1, c1 = forest.SR_gene_fitness(X, y[:, 0])   # labels (D,) as well
    assert np.array_equal(_bits(l1), _bits(loss))
    # the moments: float64, the triangle mirrored
    mean, cov, cov_y = forest.SR_gene_moments(X, y)
    assert cpu_gene_ops.calls["gene_moments"] == n0["gene_moments"] + 1
    assert mean.shape == (40, 3) and cov.shape == (40, 3, 3) and cov_y.shape == (40, 3) and cov.dtype == torch.float64
    assert np.array_equal(mean.numpy(), ref["mean"]) and np.array_equal(cov_y.numpy(), ref["c"])
    iu = np.triu_indices(3)
    assert np.array_equal(cov.numpy()[:, iu[0], iu[1]], ref["C"][:, iu[0], iu[1]]) and torch.equal(cov, cov.transpose(1, 2))
    # dedup: the same bits, every row takes its class's first row
    twice = forest + forest[:10]
    a = twice.SR_gene_fitness(X, y)
    h0 = cpu_dedup_ops.calls["tree_classes"]
    b = twice.SR_gene_fitness(X, y, dedup=True)
    assert cpu_dedup_ops.calls["tree_classes"] == h0 + 1
    for g, w in zip(b, a):
        assert np.array_equal(_bits(g), _bits(w))
    assert np.array_equal(_bits(a[0][40:]), _bits(loss[:10])) and np.array_equal(_bits(a[1][40:]), _bits(coef[:10]))
    # gene_predict: coef[:, 0] + batch_forward @ coef[:, 1:], whose MSE is the loss
    pred = forest.gene_predict(X, coef)
    assert pred.shape == (40, D) and pred.dtype == torch.float32
    genes = forest.batch_forward(X)
    want = coef[:, :1] + (genes * coef[:, None, 1:]).sum(2)
    ok = torch.isfinite(loss)
    assert torch.allclose(pred[ok], want[ok], rtol=1e-5, atol=1e-6)
    mse = ((pred.double() - y[:, 0].double()[None, :]) ** 2).mean(1)
    assert torch.allclose(mse[ok], loss[ok].double(), rtol=1e-3, atol=1e-5 * ref["syy_D"])


def test_problem_scores_and_torch_mode(rng):
    forest = _forest(rng, 40, 4, ALL_FUNCS)
    X, y = _data(rng)
    prob = SymbolicRegression(datapoints=X, labels=y, multigene=True)
    loss, coef = prob.gene_model(forest)
    assert np.array_equal(_bits(prob.evaluate(forest)), _bits(-loss))
    assert np.array_equal(_bits(prob.scores(forest)), _bits(torch.where(torch.isnan(loss), torch.full_like(loss, float("-inf")), -loss)))
    dd = SymbolicRegression(datapoints=X, labels=y, multigene=True, dedup=True)
    h0 = cpu_dedup_ops.calls["tree_classes"]
    assert np.array_equal(_bits(dd.gene_model(forest)[0]), _bits(loss)) and cpu_dedup_ops.calls["tree_classes"] == h0 + 1
    # execute_mode="torch": the same definition from batch_forward in float64 torch, none of the new ops
    n0 = dict(cpu_gene_ops.calls)
    tprob = SymbolicRegression(datapoints=X, labels=y, multigene=True, execute_mode="torch")
    tl, tc = tprob.gene_model(forest)
    assert cpu_gene_ops.calls == n0
    ref = _ref(forest, X, y)
    nan = np.isnan(ref["loss"])
    assert np.array_equal(np.isnan(tl.numpy()), nan) and np.array_equal(np.isnan(tc.numpy()).any(1), nan)
    ok = ~nan & ~GR.borderline(ref["ratio"], GR.TAU / 2, GR.TAU * 2)
    assert ok.sum() >= 20
    # float64 torch against float64 numpy: the float32 rounding of the outputs, and the order of the float64 sums through the solve
    rtol = 2.0 ** -23 + ref["cond"] * 4 * D * 2.0 ** -52
    assert np.all(np.abs(tl.numpy() - ref["loss"])[ok] <= (rtol * np.abs(ref["loss"]) + rtol * ref["syy_D"])[ok])
    scale = np.abs(ref["coef"]).max(1)
    assert np.all(np.abs(tc.numpy() - ref["coef"])[ok] <= (rtol * scale)[ok, None] + 1e-30)
    assert np.array_equal(tc.numpy()[ok] == 0, ref["coef"][ok] == 0)   # flat and dropped genes: exactly 0 in both
    assert np.array_equal(_bits(tprob.evaluate(forest)), _bits(-tl))
    assert np.array_equal(_bits(tprob.scores(forest)), _bits(torch.where(torch.isnan(tl), torch.full_like(tl, float("-inf")), -tl)))


def test_pipeline_keeps_the_best_coefficients(rng):
    from evogp_amd.algorithm import DefaultCrossover, DefaultMutation, DefaultSelection, GeneticProgramming
    from evogp_amd.pipeline import StandardPipeline

    d = GenerateDescriptor(max_tree_len=32, input_len=2, output_len=4, using_funcs=["+", "-", "*", "/"], max_layer_cnt=4,
                           const_samples=[-1, 0, 1])
    X, y = _data(rng)

    def pipeline(**kw):
        algo = GeneticProgramming(Forest.random_generate(60, d, keys=torch.tensor([1, 2])), DefaultCrossover(), DefaultMutation(0.2, d),
                                  DefaultSelection(0.3, 2))
        return algo, StandardPipeline(algo, SymbolicRegression(datapoints=X, labels=y, **kw), generation_limit=3, is_show_details=False)

    algo, pipe = pipeline(multigene=True)
    assert pipe.best_coef is None
    start = algo.forest
    loss, coef = start.SR_gene_fitness(X, y)
    n0 = cpu_gene_ops.calls["gene_fitness"]
    host = pipe.step()
    assert cpu_gene_ops.calls["gene_fitness"] == n0 + 2   # the population, then the one best tree
    assert np.array_equal(_bits(host), _bits(torch.where(torch.isnan(loss), torch.full_like(loss, float("-inf")), -loss)))
    best = int(torch.argmax(host))
    assert pipe.best_coef.shape == (5,) and pipe.best_coef.device.type == "cpu"
    assert np.array_equal(_bits(pipe.best_coef), _bits(coef[best])) and torch.equal(pipe.best_tree.node_value, start[best].node_value)
    # three generations: best_coef stays the model of best_tree, and is computed only when the best fitness improves
    algo, pipe = pipeline(multigene=True)
    n0 = cpu_gene_ops.calls["gene_fitness"]
    pipe.run()
    one = Forest(2, 4, pipe.best_tree.node_value[None].contiguous(), pipe.best_tree.node_type[None].contiguous(),
                 pipe.best_tree.subtree_size[None].contiguous())
    model = SymbolicRegression(datapoints=X, labels=y, multigene=True).gene_model(one)
    assert np.array_equal(_bits(pipe.best_coef), _bits(model[1][0])) and float(pipe.best_fitness) == -float(model[0][0])
    used = cpu_gene_ops.calls["gene_fitness"] - n0 - 1   # (minus the gene_model call just above)
    assert 3 + 1 <= used <= 3 + 3   # one call per generation, and one more for every generation that improved the best
    # without the option: no coefficients, none of the new ops
    algo, pipe = pipeline()
    n0 = dict(cpu_gene_ops.calls)
    with pytest.raises(AssertionError):
        pipe.step()   # (labels (D, 1) against a 4-output forest: the plain fitness refuses, as before)
    assert cpu_gene_ops.calls == n0 and pipe.best_coef is None


def test_argument_errors_without_gpu():
    from evogp_amd import _lib

    L = _lib.lib
    p, q = 8, 16  # (never dereferenced: the host checks come first)
    f = L.evogp_hip_sr_gene_fitness
    assert f(0, 8, 32, 3, 2, p, p, p, p, p, q, q, q, None) == -1
    assert f(4, 0, 32, 3, 2, p, p, p, p, p, q, q, q, None) == -1
    assert f(4, 8, 1025, 3, 2, p, p, p, p, p, q, q, q, None) == -1
    assert f(4, 8, 32, 0, 2, p, p, p, p, p, q, q, q, None) == -1
    assert f(4, 8, 32, 3, 0, p, p, p, p, p, q, q, q, None) == -1
    assert f(4, 8, 32, 3, 9, p, p, p, p, p, q, q, q, None) == -3      # more than EVOGP_GENES_MAX outputs: unsupported
    assert f(4, 8, 32, 3, 8, p, p, p, p, p, None, q, q, None) == -2
    assert f(4, 8, 32, 3, 8, p, p, p, p, p, q, None, None, None) == -2
    assert f(4, 8, 32, 3, 1, p, p, p, p, None, q, q, None, None) == -2
    assert L.evogp_hip_abi_version() == _lib.ABI_VERSION
