"""GPU: per-case SR errors (tree_SR_case_errors) against the twin's formula on batch_forward outputs, bit for bit, and
epsilon-lexicase selection (lexicase_select, LexicaseSelection) against the numpy twin (tests/lexicase_ref.py), event for event."""
import os
import sys

import numpy as np
import pytest
import torch

import evogp_amd  # noqa: F401  (registers the ops)
from evogp_amd.algorithm import lexicase_epsilon

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lexicase_ref as R  # noqa: E402
from grad_trees import ALL_FUNCS, ARITH, random_forest  # noqa: E402
from helpers import assert_within_sensitivity, per_tree_tolerance  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _forest(value, type_, size, var_len, out_len):
    from evogp_amd.tree import Forest

    v, t, s = _dev(value, type_, size)
    return Forest(var_len, out_len, v, t, s)


def _select(E, eps, n_events, seed, gen):
    E_d, eps_d = _dev(E, eps)
    return torch.ops.evogp_hip.lexicase_select(E_d, eps_d, n_events, seed, gen).cpu().numpy()


def _check_events(E, eps, n_events, seed, gen, sample=None, rng=None):
    """all events (or a seeded sample of them) against the twin"""
    got = _select(E, eps, n_events, seed, gen)
    assert got.shape == (n_events,) and got.dtype == np.int32
    if n_events == 0:
        return got
    ks = np.arange(n_events) if sample is None or n_events <= sample else np.sort(rng.choice(n_events, sample, replace=False))
    want = R.select(E, eps, n_events, seed, gen, events=ks)
    bad = np.flatnonzero(got[ks] != want)
    assert not len(bad), f"{len(bad)} of {len(ks)} events differ, e.g. event {ks[bad[0]]}: {got[ks[bad[0]]]} vs {want[bad[0]]}"
    return got


# ---- case errors ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 63, 1024, 5000])
@pytest.mark.parametrize("gp_len", [64, 1024])
@pytest.mark.parametrize("out_len", [1, 3])
@pytest.mark.parametrize("funcs", ["arith", "all"])
def test_case_errors_equal_formula_on_batch_forward(rng, funcs, out_len, gp_len, D):
    var_len = 3
    value, type_, size = random_forest(rng, 40, gp_len, ARITH if funcs == "arith" else ALL_FUNCS, var_len, out_len, max_depth=5)
    value[0, 0], type_[0, 0], size[0, 0] = np.nan, 1, 1            # a NaN tree (single output: the constant is the output)
    f = _forest(value, type_, size, var_len, out_len)
    X, y = _dev(rng.uniform(0.5, 1.5, (D, var_len)).astype(np.float32), rng.uniform(-1, 1, (D, out_len)).astype(np.float32))
    pred = f.batch_forward(X).cpu().numpy()
    for mse in (True, False):
        e = f.SR_case_errors(X, y, use_MSE=mse)
        assert e.shape == (40, D) and e.stride() == (1, 40) and e.dtype == torch.float32 and e.is_cuda
        got = e.t().contiguous().cpu().numpy()
        want = R.case_errors(pred, y.cpu().numpy(), mse)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "case errors differ from the formula"
        assert np.array_equal(np.isnan(got), np.isnan(pred).any(axis=2).T)   # NaN stays NaN
        if out_len == 1:
            assert np.isnan(got[:, 0]).all()


@pytest.mark.parametrize("funcs,out_len", [("arith", 1), ("all", 1), ("all", 4)])
def test_row_means_match_fitness(rng, oracle, funcs, out_len):
    value, type_, size = random_forest(rng, 200, 64, ARITH if funcs == "arith" else ALL_FUNCS, 3, out_len, max_depth=5)
    X = rng.uniform(0.5, 1.5, (300, 3)).astype(np.float32)
    y = rng.uniform(-1, 1, (300, out_len)).astype(np.float32)
    f = _forest(value, type_, size, 3, out_len)
    Xd, yd = _dev(X, y)
    means = f.SR_case_errors(Xd, yd).double().mean(dim=1).cpu().numpy() * out_len   # SR fitness sums over the outputs
    want, tol, unstable = per_tree_tolerance(oracle, (value, type_, size), X, y)
    assert_within_sensitivity(means, want, tol, unstable, "row mean of the case errors")
    fit = f.SR_fitness(Xd, yd).cpu().numpy().astype(np.float64)
    assert_within_sensitivity(means, fit, tol, unstable, "row mean vs SR_fitness")


# ---- lexicase_select against the twin ------------------------------------------------------------------------------------------
def _errors(rng, n, pop, kind):
    if kind == "continuous":
        E = rng.exponential(1.0, (n, pop)).astype(np.float32)
    else:   # quantized: many ties
        E = rng.integers(0, 4, (n, pop)).astype(np.float32) * 0.25
    E[rng.random((n, pop)) < 0.03] = np.nan
    E[rng.random((n, pop)) < 0.02] = np.inf
    E[rng.random((n, pop)) < 0.02] = -0.0
    return E


def _eps(E, mode):
    n = E.shape[0]
    if mode == "zero":
        return np.zeros(n, np.float32)
    if mode == "large":
        return np.full(n, 1e6, np.float32)
    got = lexicase_epsilon(torch.from_numpy(E).cuda().t()).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), R.epsilon(E.T).view(np.uint32))   # on the device too
    return got


@pytest.mark.parametrize("pop", [1, 2, 7, 64, 4099])
@pytest.mark.parametrize("n", [1, 3, 64, 1024, 4097])
def test_select_equals_twin(rng, pop, n):
    combos = [(kind, eps) for kind in ("continuous", "quantized") for eps in ("zero", "auto", "large")]
    small = pop * n <= 64 * 1024
    for i, (kind, eps_mode) in enumerate(combos if small else combos[(pop + n) % 2::2]):
        E = _errors(rng, n, pop, kind)
        eps = _eps(E, eps_mode)
        n_events = [0, 1, pop, 3 * pop + 1][i % 4]
        _check_events(E, eps, n_events, 1000 + i, i, sample=None if small else 24, rng=rng)


def test_clones_and_identical_population(rng):
    n, pop = 64, 3000
    base = _errors(rng, n, 40, "quantized")
    E = base[:, rng.integers(0, 40, pop)]                          # 40 clone classes of ~75 trees
    for eps_mode in ("zero", "auto"):
        got = _check_events(E, _eps(E, eps_mode), 2 * pop, 5, 1, sample=200, rng=rng)
        assert len(set(got.tolist())) > 40                       # members of a class are drawn, not only its first tree
    same = np.tile(base[:, :1], (1, pop))                         # one class: uniform over the whole population
    got = _check_events(same, np.zeros(n, np.float32), 3 * pop + 1, 6, 2, sample=200, rng=rng)
    assert len(set(got.tolist())) > pop // 2


def test_first_pools_larger_than_lds(rng):
    n, pop = 48, 50_000
    E = (rng.random((n, pop)) < 0.5).astype(np.float32)           # every first pool holds about 25 000 classes
    E[:, :1000] = E[:, 1000:2000]                                  # and some clones
    _check_events(E, np.zeros(n, np.float32), pop, 9, 3, sample=48, rng=rng)


def test_determinism_and_generations(rng):
    E = _errors(rng, 64, 4099, "continuous")
    eps = _eps(E, "auto")
    a, b = _select(E, eps, 5000, 77, 4), _select(E, eps, 5000, 77, 4)
    assert np.array_equal(a, b)
    assert not np.array_equal(a, _select(E, eps, 5000, 77, 5))


# ---- configs[1]: 100 k trees x 1024 rows ---------------------------------------------------------------------------------------
def _configs1():
    from evogp_amd.tree import Forest, GenerateDescriptor
    from helpers import c2_dataset

    X, y = c2_dataset()
    X, y = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
    desc = GenerateDescriptor(max_tree_len=64, input_len=10, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=6,
                              const_samples=[-1, 0, 1])
    f = Forest.random_generate(100_000, desc, keys=torch.tensor([42, 0], dtype=torch.uint32, device="cuda"))
    return desc, f, X, y


def test_configs1_size_sampled_events(rng):
    from evogp_amd.algorithm import DefaultCrossover, DefaultMutation, GeneticProgramming, LexicaseSelection

    desc, f, X, y = _configs1()
    torch.manual_seed(0)
    sel = LexicaseSelection(X, y)
    algo = GeneticProgramming(f, DefaultCrossover(), DefaultMutation(0.2, desc), sel)
    for stage in ("fresh", "evolved"):
        if stage == "evolved":
            for _ in range(3):
                algo.step(-algo.forest.SR_fitness(X, y))
        forest = algo.forest
        errors = forest.SR_case_errors(X, y, use_MSE=False)
        E = errors.t().contiguous()
        eps = lexicase_epsilon(errors)
        got = torch.ops.evogp_hip.lexicase_select(E, eps, 100_000, 31, 7).cpu().numpy()
        ks = np.sort(rng.choice(100_000, 256, replace=False))
        want = R.select(E.cpu().numpy(), eps.cpu().numpy(), 100_000, 31, 7, events=ks)
        assert np.array_equal(got[ks], want), stage


# ---- the operator on the fused generation step ---------------------------------------------------------------------------------
def _small_problem():
    from evogp_amd.tree import Forest, GenerateDescriptor

    desc = GenerateDescriptor(max_tree_len=32, input_len=2, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=4,
                              const_samples=[-1, 0.5, 1])
    g = np.random.default_rng(5)
    X = torch.from_numpy(g.uniform(-1, 1, (128, 2)).astype(np.float32)).cuda()
    y = (X[:, :1] * X[:, 1:] + 0.5).contiguous()
    f = Forest.random_generate(2000, desc, keys=torch.tensor([7, 8], dtype=torch.uint32, device="cuda"))
    return desc, f, X, y


def test_fused_generation_step():
    from evogp_amd.algorithm import DefaultCrossover, DefaultMutation, GeneticProgramming, LexicaseSelection

    class Recording(LexicaseSelection):
        def __call__(self, forest, fitness):
            gen = self.generation
            out = super().__call__(forest, fitness)
            self.seen.append((forest, gen, out[1]))
            return out

    runs = []
    for _ in range(2):
        desc, f, X, y = _small_problem()
        torch.manual_seed(123)
        sel = Recording(X, y, elite_cnt=5, survivor_rate=0.5, downsample_rate=0.5)
        sel.seen = []
        algo = GeneticProgramming(f, DefaultCrossover(), DefaultMutation(0.2, desc), sel)
        assert algo._native_plan() is not None                       # the fused path
        for _ in range(3):
            nxt = algo.step(-algo.forest.SR_fitness(X, y))
            assert nxt.pop_size == 2000
            assert algo._last_n_elite == 5                            # (set by the fused pass)
        # the survivors the step used are lexicase_select's on the same errors
        assert len(sel.seen) == 3
        for forest, gen, surv in sel.seen:
            rows = torch.from_numpy(R.sample_rows(sel.seed, gen, 128, 0.5)).cuda()
            errors = forest.SR_case_errors(X[rows], y[rows], use_MSE=False)
            want = torch.ops.evogp_hip.lexicase_select(errors.t().contiguous(), lexicase_epsilon(errors), 1000, sel.seed, gen)
            assert torch.equal(surv, want)
        runs.append(algo.forest)
    for name in ("batch_node_value", "batch_node_type", "batch_subtree_size"):
        assert torch.equal(getattr(runs[0], name), getattr(runs[1], name))


def test_no_host_sync_inside_call():
    from evogp_amd.algorithm import LexicaseSelection

    for kw in ({}, {"downsample_rate": 0.25, "epsilon": 0.01}):
        _, f, X, y = _small_problem()
        sel = LexicaseSelection(X, y, elite_cnt=3, **kw)
        fit = -f.SR_fitness(X, y)
        sel(f, fit)                                                  # (warm-up: engine buffers, allocator)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            elites, surv = sel(f, fit)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert surv.shape == (2000,) and elites.shape == (3,)
