"""GPU: the Pareto ranking (pareto_rank) against the numpy twin (tests/nsga2_ref.py) word for word -- fronts and order as integers, the
crowding distances as bit patterns, no tolerance --, the tournaments (nsga2_select) against the twin for every tournament, and
NSGA2Selection on the fused generation step."""
import os
import sys

import numpy as np
import pytest
import torch

import evogp_amd  # noqa: F401  (registers the ops)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nsga2_ref as R  # noqa: E402
from test_nsga2_ref import POPS, SPANS, assert_same, population  # noqa: E402

pytestmark = pytest.mark.gpu


def _rank(err, cx, cx_bound=R.CX_MAX):
    out = torch.ops.evogp_hip.pareto_rank(torch.from_numpy(np.ascontiguousarray(err)).cuda(), torch.from_numpy(np.ascontiguousarray(cx)).cuda(),
                                          cx_bound)
    front, crowding, order = (t.cpu().numpy() for t in out)
    assert front.dtype == np.int32 and crowding.dtype == np.float32 and order.dtype == np.int32
    return front, crowding, order


def _check(err, cx, cx_bound=R.CX_MAX, what=""):
    want = R.rank(err, cx, cx_bound)
    got = _rank(err, cx, cx_bound)
    n_fronts = int(want[0][want[0] != R.UNRANKED].max()) + 1 if (want[0] != R.UNRANKED).any() else 0
    print(f"{what}: pop {len(err)}, {n_fronts} fronts, {len(np.unique(cx))} distinct cx")
    assert_same(got, want, what)
    return got


# ---- pareto_rank against the twin ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pop", POPS)
@pytest.mark.parametrize("span", SPANS)
@pytest.mark.parametrize("kind", ["continuous", "quantised"])
def test_rank_equals_twin(rng, kind, span, pop):
    err, cx = population(rng, pop, kind, span)
    _check(err, cx, what=f"{kind} pop {pop} span {span}")


def test_all_unranked_all_clones_and_the_bound(rng):
    for pop in (1, 7, 300, 5000):
        err = np.full(pop, np.nan, np.float32)
        err[::2] = np.inf
        front, crowd, order = _check(err, (np.arange(pop) % 5).astype(np.int32), what="all unranked")
        assert (front == R.UNRANKED).all() and (crowd == 0).all() and order.tolist() == list(range(pop))
        front, crowd, order = _check(np.full(pop, 0.5, np.float32), np.full(pop, 9, np.int32), what="all clones")
        assert (front == 0).all() and np.isinf(crowd[0]) and (crowd[1:] == 0).all() and order.tolist() == list(range(pop))
    # trees outside [0, cx_bound] are unranked; the bound itself is inside
    err, cx = population(rng, 3000, "quantised", 40)
    cx[::7] = -3
    cx[1::7] = 70000
    front, _, _ = _check(err, cx, 25, what="cx_bound 25")
    assert (front[(cx < 0) | (cx > 25)] == R.UNRANKED).all() and (front[cx == 25] != R.UNRANKED).any()
    _check(err, np.zeros(3000, np.int32), 0, what="cx_bound 0")
    with pytest.raises(RuntimeError, match="cx_bound"):
        _rank(err, cx, 65536)


def _tree_sizes(pop, L):
    """the sizes of ``pop`` freshly generated trees of at most L nodes"""
    from evogp_amd.tree import Forest, GenerateDescriptor

    layers = {64: 6, 512: 9, 1024: 10}[L]
    desc = GenerateDescriptor(max_tree_len=L, input_len=3, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=layers,
                              layer_leaf_prob=0.1, const_samples=[-1, 0, 1])
    f = Forest.random_generate(pop, desc, keys=torch.tensor([11, L], dtype=torch.uint32, device="cuda"))
    return f.batch_subtree_size[:, 0].to(torch.int32).cpu().numpy()


@pytest.mark.parametrize("pop", [4099, 100_000])
@pytest.mark.parametrize("L", [64, 512, 1024])
def test_rank_equals_twin_on_tree_sizes(rng, L, pop):
    cx = _tree_sizes(pop, L)
    assert cx.min() >= 1 and cx.max() <= L
    for kind in ("continuous", "quantised"):
        err, _ = population(rng, pop, kind, 2)
        front, _, _ = _check(err, cx, L, what=f"{kind} pop {pop} L {L}")
        # trees of equal size chain by error: there are at least as many fronts as the fullest bucket has distinct keys
        ranked = front != R.UNRANKED
        pairs = np.unique(cx[ranked].astype(np.int64) << 32 | R.keys(err)[ranked].view(np.uint32))
        assert front[ranked].max() + 1 >= np.bincount(pairs >> 32).max()


def test_clones_of_few_points(rng):
    base_err, base_cx = population(rng, 5000, "continuous", 64)
    pick = rng.integers(0, 5000, 100_000)                           # 5 000 distinct points, each cloned about 20 times
    front, crowd, _ = _check(base_err[pick], base_cx[pick], 64, what="clones")
    ranked = front != R.UNRANKED
    points = R.keys(base_err[pick]).view(np.uint32).astype(np.int64) << 17 | base_cx[pick]
    assert (crowd[ranked] > 0).sum() == len(np.unique(points[ranked]))   # one representative per distinct point


def _configs1(pop=100_000):
    from evogp_amd.tree import Forest, GenerateDescriptor
    from helpers import c2_dataset

    X, y = c2_dataset()
    X, y = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
    desc = GenerateDescriptor(max_tree_len=64, input_len=10, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=6,
                              const_samples=[-1, 0, 1])
    f = Forest.random_generate(pop, desc, keys=torch.tensor([42, 0], dtype=torch.uint32, device="cuda"))
    return desc, f, X, y


def test_real_forest_configs1():
    from evogp_amd.algorithm import NSGA2Selection

    _, f, X, y = _configs1()
    fit = -f.SR_fitness(X, y)
    sel = NSGA2Selection()
    got = [t.cpu().numpy() for t in sel.rank(f, fit)]
    want = R.rank((-fit).cpu().numpy(), f.batch_subtree_size[:, 0].cpu().numpy().astype(np.int32), 64)
    assert_same(got, want, "configs[1]")
    mask = sel.pareto_set(f, fit).cpu().numpy()
    assert mask.tolist() == ((want[0] == 0) & (want[1] > 0)).tolist() and 1 <= mask.sum() <= 64


def test_one_million_trees(rng):
    pop = 1_000_000
    err = rng.exponential(1.0, pop).astype(np.float32)
    err[rng.random(pop) < 0.35] = np.nan
    cx = np.minimum(rng.geometric(0.08, pop), 64).astype(np.int32)
    front, _, _ = _check(err, cx, 64, what="1 M")
    assert front[front != R.UNRANKED].max() > 10_000


def test_two_calls_give_identical_bits(rng):
    err, cx = population(rng, 100_000, "quantised", 64)
    a, b = _rank(err, cx, 64), _rank(err, cx, 64)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


# ---- nsga2_select against the twin -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pop", [1, 7, 4099])
def test_select_equals_twin(rng, pop):
    order = rng.permutation(pop).astype(np.int32)
    order_d = torch.from_numpy(order).cuda()
    for t_size in (1, 2, 7):
        for pool in sorted({1, max(pop // 2, 1), pop}):
            for i, n in enumerate((0, 1, pop, 3 * pop + 1)):
                got = torch.ops.evogp_hip.nsga2_select(order_d, pool, n, t_size, 500 + t_size, i).cpu().numpy()
                want = R.select(order, pool, n, t_size, 500 + t_size, i)
                assert got.dtype == np.int32 and got.shape == (n,)
                assert np.array_equal(got, want), f"t_size {t_size} pool {pool} n {n}"
    for bad in ((0, 5, 2), (pop + 1, 5, 2), (1, 5, 0), (1, 5, 2**20 + 1), (1, -1, 2)):
        with pytest.raises(RuntimeError):
            torch.ops.evogp_hip.nsga2_select(order_d, bad[0], bad[1], bad[2], 0, 0)


# ---- the operator ----------------------------------------------------------------------------------------------------------------
def _small_problem():
    from evogp_amd.tree import Forest, GenerateDescriptor

    desc = GenerateDescriptor(max_tree_len=32, input_len=2, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=4,
                              const_samples=[-1, 0.5, 1])
    g = np.random.default_rng(5)
    X = torch.from_numpy(g.uniform(-1, 1, (128, 2)).astype(np.float32)).cuda()
    y = (X[:, :1] * X[:, 1:] + 0.5).contiguous()
    f = Forest.random_generate(2000, desc, keys=torch.tensor([7, 8], dtype=torch.uint32, device="cuda"))
    return desc, f, X, y


def test_no_host_sync_inside_call():
    from evogp_amd.algorithm import NSGA2Selection

    depth = lambda forest: (forest.batch_subtree_size[:, 0] // 4).to(torch.int64)   # noqa: E731
    for kw in ({}, {"elite_rate": 0.5, "mating_pool": "elites", "tournament_size": 3}, {"complexity": depth, "max_complexity": 8, "elite_cnt": 3}):
        _, f, X, y = _small_problem()
        sel = NSGA2Selection(**kw)
        fit = -f.SR_fitness(X, y)
        sel(f, fit)                                                  # (warm-up: allocator)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            elites, surv = sel(f, fit)
            mask = sel.pareto_set(f, fit)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        n_elite, n_surv = sel.counts(2000)
        assert surv.shape == (n_surv,) and elites.shape == (n_elite,) and mask.shape == (2000,)
        cx = depth(f) if "complexity" in kw else f.batch_subtree_size[:, 0]
        _, _, order = R.rank((-fit).cpu().numpy(), cx.cpu().numpy().astype(np.int32), kw.get("max_complexity", 32))
        assert elites.cpu().tolist() == order[:n_elite].tolist()
        pool = n_elite if kw.get("mating_pool") == "elites" else 2000
        assert surv.cpu().tolist() == R.select(order, pool, n_surv, sel.t_size, sel.seed, 1).tolist()


def test_fused_generation_step():
    """the next forest is what breed_rows_hashed makes of the TWIN's lists"""
    from evogp_amd.algorithm import DefaultCrossover, DefaultMutation, GeneticProgramming, NSGA2Selection
    from evogp_amd.tree import Forest

    runs = []
    for _ in range(2):
        desc, f, X, y = _small_problem()
        torch.manual_seed(123)
        sel = NSGA2Selection(elite_rate=0.5, mating_pool="elites")
        mut = DefaultMutation(0.2, desc)
        algo = GeneticProgramming(f, DefaultCrossover(), mut, sel)
        assert algo._native_plan() is not None                       # the fused path
        for gen in range(3):
            cur = algo.forest
            fit = -cur.SR_fitness(X, y)
            nxt = algo.step(fit)
            assert nxt.pop_size == 2000 and algo._last_n_elite == 1000 and sel.generation == gen + 1
            _, _, order = R.rank((-fit).cpu().numpy(), cur.batch_subtree_size[:, 0].cpu().numpy().astype(np.int32), 32)
            elites = torch.from_numpy(order[:1000].copy()).cuda()
            parents = torch.from_numpy(R.select(order, 1000, 2000, 2, sel.seed, gen)).cuda()
            below = int(0.2 * (2**31 - 1))
            donors = torch.ops.evogp_hip.tree_generate_masked_hashed(
                1000, 32, desc.input_len, desc.output_len, desc.const_samples.shape[0], desc.out_prob, desc.const_prob, desc.depth2leaf_probs,
                desc.roulette_funcs, desc.const_samples, 0, algo._word_seed, algo._steps, below)
            want = torch.ops.evogp_hip.breed_rows_hashed(2000, 32, *cur._tensors(), elites, parents, algo._word_seed, algo._steps, below, *donors,
                                                         0, 2000)
            for got_t, want_t in zip(nxt._tensors(), want):
                assert torch.equal(got_t.view(torch.int32) if got_t.dtype == torch.float32 else got_t,
                                   want_t.view(torch.int32) if want_t.dtype == torch.float32 else want_t), f"generation {gen}"
        runs.append(algo.forest)
    for name in ("batch_node_value", "batch_node_type", "batch_subtree_size"):
        assert torch.equal(getattr(runs[0], name), getattr(runs[1], name))

