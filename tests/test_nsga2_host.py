"""CPU: the host logic of NSGA2Selection with the numpy twin registered as a test-only CPU kernel (tests/cpu_nsga2_ops.py), a composed
GeneticProgramming step on a CPU forest, and the argument checks of the three new C entry points, which return before any launch."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cpu_nsga2_ops  # noqa: E402
import nsga2_ref as R  # noqa: E402

cpu_nsga2_ops.register()

from evogp_amd.algorithm import NSGA2Selection  # noqa: E402
from evogp_amd.tree import Forest, GenerateDescriptor, set_default_device  # noqa: E402
from evogp_amd.tree import utils as _tree_utils  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _cpu_default_device():
    saved = _tree_utils._DEVICE
    set_default_device("cpu")
    yield
    _tree_utils._DEVICE = saved


def _problem(rng, pop=60):
    d = GenerateDescriptor(max_tree_len=32, input_len=2, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=4,
                           const_samples=[-1, 0.5, 1])
    f = Forest.random_generate(pop, d, keys=torch.tensor([3, 4]))
    fit = -torch.from_numpy((rng.integers(0, 8, pop) * 0.5).astype(np.float32))       # many ties
    fit[5] = float("nan")
    fit[6] = float("-inf")
    fit[7] = float("inf")
    return d, f, fit


def _twin(f, fit, bound=None, cx=None):
    cx = f.batch_subtree_size[:, 0].numpy().astype(np.int32) if cx is None else cx
    return R.rank((-fit).numpy(), cx, f.max_tree_len if bound is None else bound)


def test_exported_under_both_import_roots():
    import evogp.algorithm
    import evogp_amd.algorithm

    assert evogp.algorithm.NSGA2Selection is evogp_amd.algorithm.NSGA2Selection is NSGA2Selection
    assert "NSGA2Selection" in evogp_amd.algorithm.__all__


def test_argument_checks():
    for kw in ({"tournament_size": 0}, {"tournament_size": 2**20 + 1}, {"survivor_rate": 1.5}, {"elite_rate": -0.1}, {"mating_pool": "front"},
               {"complexity": 3, "max_complexity": 4}, {"complexity": lambda forest: None}, {"max_complexity": 5},
               {"complexity": lambda forest: None, "max_complexity": 65536}):
        with pytest.raises(AssertionError):
            NSGA2Selection(**kw)


def test_lists_counts_and_reproducibility(rng):
    _, f, fit = _problem(rng)
    torch.manual_seed(7)
    sel = NSGA2Selection(survivor_rate=0.5, elite_cnt=3)
    elites, surv = sel(f, fit)
    assert elites.dtype == surv.dtype == torch.int32 and surv.shape == (30,) and elites.shape == (3,)
    front, crowd, order = _twin(f, fit)
    assert front[5] == front[6] == front[7] == R.UNRANKED         # NaN and infinite fitness are unranked
    assert elites.tolist() == order[:3].tolist()
    assert surv.tolist() == R.select(order, 60, 30, 2, sel.seed, 0).tolist()
    assert sel.generation == 1
    # rank() and pareto_set()
    got = sel.rank(f, fit)
    for g, w in zip(got, (front, crowd, order)):
        assert np.array_equal(g.numpy(), w)
    mask = sel.pareto_set(f, fit)
    assert mask.dtype == torch.bool and mask.tolist() == ((front == 0) & (crowd > 0)).tolist() and mask.any()
    assert sel.generation == 1                                    # (neither draws)
    # same torch seed -> same draws; the next call is another generation
    torch.manual_seed(7)
    sel2 = NSGA2Selection(survivor_rate=0.5, elite_cnt=3)
    assert sel2.seed == sel.seed and sel2(f, fit)[1].tolist() == surv.tolist()
    assert sel(f, fit)[1].tolist() == R.select(order, 60, 30, 2, sel.seed, 1).tolist()
    # counts: survivor_cnt / elite_rate, the defaults, the tournament size
    e, s = NSGA2Selection(survivor_cnt=7, elite_rate=0.1)(f, fit)
    assert e.shape == (6,) and s.shape == (7,)
    sel = NSGA2Selection(tournament_size=7)
    e, s = sel(f, fit)
    assert e.shape == (0,) and s.shape == (60,) and s.tolist() == R.select(order, 60, 60, 7, sel.seed, 0).tolist()


def test_mating_pool_of_elites(rng):
    _, f, fit = _problem(rng)
    _, _, order = _twin(f, fit)
    sel = NSGA2Selection(elite_rate=0.5, mating_pool="elites")
    elites, surv = sel(f, fit)
    assert elites.tolist() == order[:30].tolist() and surv.shape == (60,)
    assert surv.tolist() == R.select(order, 30, 60, 2, sel.seed, 0).tolist()
    assert set(surv.tolist()) <= set(elites.tolist())
    with pytest.raises(AssertionError, match="elites"):
        NSGA2Selection(mating_pool="elites")(f, fit)              # no elite: nobody to draw from


def test_complexity_callable(rng):
    _, f, fit = _problem(rng)
    depth = torch.from_numpy(rng.integers(0, 9, 60))              # int64: any integer dtype
    seen = []

    def hook(forest):
        seen.append(forest)
        return depth

    sel = NSGA2Selection(complexity=hook, max_complexity=6, elite_cnt=4)    # 7 and 8 are outside the bound: unranked
    elites, surv = sel(f, fit)
    assert seen == [f]
    front, _, order = R.rank((-fit).numpy(), depth.numpy().astype(np.int32), 6)
    assert (front[depth.numpy() > 6] == R.UNRANKED).all()
    assert elites.tolist() == order[:4].tolist() and surv.tolist() == R.select(order, 60, 60, 2, sel.seed, 0).tolist()
    for bad in (lambda forest: torch.zeros(3, dtype=torch.int32), lambda forest: torch.zeros(60)):
        with pytest.raises(AssertionError):
            NSGA2Selection(complexity=bad, max_complexity=6)(f, fit)


def test_composed_generation_step_on_a_cpu_forest(rng):
    from evogp_amd.algorithm import DefaultCrossover, DefaultMutation, GeneticProgramming

    d, f, _ = _problem(rng)
    X = torch.from_numpy(rng.uniform(-1, 1, (24, 2)).astype(np.float32))
    y = torch.from_numpy(rng.uniform(-1, 1, (24, 1)).astype(np.float32))

    class Recording(NSGA2Selection):
        def __call__(self, forest, fitness):
            out = super().__call__(forest, fitness)
            self.seen.append(out)
            return out

    torch.manual_seed(3)
    sel = Recording(elite_rate=0.5, mating_pool="elites")
    sel.seen = []
    algo = GeneticProgramming(f, DefaultCrossover(), DefaultMutation(0.2, d), sel)
    for gen in range(2):
        cur = algo.forest
        fit = -cur.SR_fitness(X, y)
        _, _, order = _twin(cur, fit)
        nxt = algo.step(fit)
        elites, surv = sel.seen[gen]
        assert elites.tolist() == order[:30].tolist() and surv.tolist() == R.select(order, 30, 60, 2, sel.seed, gen).tolist()
        # the forest the lists imply: the elites first, unchanged, then the offspring
        assert nxt.pop_size == 60
        for name in ("batch_node_value", "batch_node_type", "batch_subtree_size"):
            assert torch.equal(getattr(nxt, name)[:30], getattr(cur, name)[torch.from_numpy(order[:30].astype(np.int64))])


def test_sharded_step_is_refused():
    from evogp_amd.parallel import _Population

    with pytest.raises(TypeError, match="sharded"):
        NSGA2Selection()(_Population(4), torch.zeros(4))


def test_argument_errors_without_gpu():
    from evogp_amd import _lib

    L = _lib.lib
    p = 8  # (never dereferenced: the host checks come first)
    b = ctypes.c_ulonglong(0)
    assert L.evogp_hip_pareto_rank_workspace_bytes(0, ctypes.byref(b)) == -1
    assert L.evogp_hip_pareto_rank_workspace_bytes(0x7FFFFFFF, ctypes.byref(b)) == -1
    assert L.evogp_hip_pareto_rank_workspace_bytes(10, None) == -2
    assert L.evogp_hip_pareto_rank(0, 64, p, p, p, p, p, p, None) == -1
    assert L.evogp_hip_pareto_rank(10, 65536, p, p, p, p, p, p, None) == -1          # cx_bound above 65535
    assert L.evogp_hip_pareto_rank(10, 64, p, None, p, p, p, p, None) == -2
    assert L.evogp_hip_pareto_rank(10, 64, p, p, p, p, p, None, None) == -2
    assert L.evogp_hip_nsga2_select(0, p, 1, 3, 2, 1, 2, p, None) == -1
    assert L.evogp_hip_nsga2_select(10, p, 0, 3, 2, 1, 2, p, None) == -1             # empty pool
    assert L.evogp_hip_nsga2_select(10, p, 11, 3, 2, 1, 2, p, None) == -1            # pool larger than the population
    assert L.evogp_hip_nsga2_select(10, p, 5, 3, 0, 1, 2, p, None) == -1
    assert L.evogp_hip_nsga2_select(10, p, 5, 3, 2**20 + 1, 1, 2, p, None) == -1
    assert L.evogp_hip_nsga2_select(10, p, 5, 0, 2, 1, 2, None, None) == 0           # no tournament: nothing to do
    assert L.evogp_hip_nsga2_select(10, None, 5, 3, 2, 1, 2, p, None) == -2
    assert L.evogp_hip_nsga2_select(10, p, 5, 3, 2, 1, 2, None, None) == -2


def test_product_registers_no_cpu_kernel():
    code = ("import torch, evogp_amd\n"
            "for call in (lambda: torch.ops.evogp_hip.pareto_rank(torch.zeros(3), torch.zeros(3, dtype=torch.int32), 8),\n"
            "             lambda: torch.ops.evogp_hip.nsga2_select(torch.zeros(3, dtype=torch.int32), 3, 3, 2, 0, 0)):\n"
            "    try:\n"
            "        call()\n"
            "    except (RuntimeError, NotImplementedError) as e:\n"
            "        print('REJECTED', 'pareto_rank' in str(e) or 'nsga2_select' in str(e))\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.stdout.count("REJECTED True") == 2, r.stdout + r.stderr
