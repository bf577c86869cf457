"""CPU: the default generation step against recorded runs of the REFERENCE's own Python operators (DefaultSelection ->
DefaultCrossover -> DefaultMutation inside GeneticProgramming.step; genetic_programming.py:101-120, selection/default.py:42-71,
crossover/default.py:16-66, mutation/default.py:32-75).  tests/golden/default_step_<case>.npz hold, per generation, the input
forest, the fitness, every draw and every intermediate of the reference (tests/golden/make_default_step_golden.py); the ops run
on the TEST-ONLY oracle back end (tests/cpu_ops.py).  Bit for bit, whole rows.

  1. the composed path (GeneticProgramming._breed where the fused pass does not take the step) on the reference's draws;
  2. `_expected`, the restatement the large breeding tests of tests/test_gpu_breed.py compare the kernels with;
  3. the selection: parallel.default_lists and DefaultSelection.__call__ against the reference's lists.
tests/test_gpu_default_step_parity.py runs the kernels on the same fixtures.

Two deliberate deviations, both in the ranking.  NaN fitness ranks worst here, behind -inf; the reference's
torch.sort(descending=True) ranks it FIRST (`nan_inf` records that: NaN trees are its elites).  Trees of equal fitness are listed
by tree index here (a stable sort: replicated ranks of a sharded run agree); the reference's sort leaves them in another order
(`ties`).  The tests assert the deviations themselves: our lists are the reference's ranking with every NaN moved to the back; where
a tie straddles a threshold the selected fitness values are the reference's; and breeding from the reference's own lists still
gives the reference's population (tests/default_step_replay.py OWN_ORDER)."""
import numpy as np
import pytest
import torch

import cpu_ops
import default_step_replay as dr
from helpers import assert_forest_equal


@pytest.fixture(scope="module", autouse=True)
def _cpu_ops():
    cpu_ops.register()
    from evogp_amd.tree import default_device, set_default_device

    old = default_device()
    set_default_device("cpu")
    yield
    set_default_device(old)


@pytest.fixture(scope="module")
def oracle():
    from oracle.pyoracle import Oracle

    return Oracle("port")


@pytest.mark.parametrize("case", dr.CASES)
def test_fixture_keeps_its_edges(case):
    """the edge conditions of every case, derived again from the arrays (a regenerated fixture cannot silently lose one)"""
    meta, gens = dr.load(case)
    found = [dr.edges(g) for g in gens]
    assert found == meta["edges"]
    dr.check_edges(case, found)
    assert all(g.pop <= 400 for g in gens)


@pytest.mark.parametrize("case", dr.CASES)
def test_composed_path_reproduces_the_reference(case):
    dr.check_composed_path(case, "cpu")


@pytest.mark.parametrize("case", dr.CASES)
def test_restatement_reproduces_the_reference(case, oracle):
    """`_expected` from the replay arguments = the reference's final population and its decisions: what makes the 100 k and 1 M
    breeding tests of tests/test_gpu_breed.py descend from the reference.  Both calling forms (one order; two lists)."""
    _, gens = dr.load(case)
    for gen in gens:
        a = dr.replay_args(gen)
        out, dec = dr._expected(oracle, gen.forest, a["order"], a["rnd"], a["below"], a["n_elite"], a["n_surv"], a["donors"])
        assert np.array_equal(dec, dr.recorded_decisions(gen)), "decisions differ"
        assert_forest_equal(out, gen.out, f"{case}: _expected, one order")
        out, dec = dr._expected(oracle, gen.forest, a["elites"], a["rnd"], a["below"], a["n_elite"], a["n_surv"], a["donors"], parents=a["parents"])
        assert np.array_equal(dec, dr.recorded_decisions(gen))
        assert_forest_equal(out, gen.out, f"{case}: _expected, two lists")


@pytest.mark.parametrize("case", dr.CASES)
def test_selection_agrees_with_the_reference(case):
    from evogp_amd.algorithm import DefaultSelection
    from evogp_amd.parallel import default_lists

    meta, gens = dr.load(case)
    sel = DefaultSelection(**meta["selection"])
    for gen in gens:
        fit = torch.from_numpy(gen.fitness)
        assert sel.counts(gen.pop) == (len(gen.elite), len(gen.survivor))
        dr.check_selection(case, gen, *(x.numpy() for x in default_lists(fit, *sel.counts(gen.pop))))
        elites, parents = (x.numpy() for x in sel(dr.forest_of(gen.forest, meta, "cpu"), fit))
        dr.check_selection(case, gen, elites, parents)
        if case not in dr.OWN_ORDER:   # the composed operator returns the ranking itself: the reference's lists, entry by entry
            assert np.array_equal(elites, gen.elite) and np.array_equal(parents, gen.survivor)


def test_both_selections_choose_the_same_sets_on_nan():
    """DefaultSelection.__call__ (the composed path) and default_lists (the fused path) on the `nan_inf` fitness -- NaN, -inf, +inf,
    -0.0 and +0.0 -- and on the same vector with NaN at every threshold"""
    from evogp_amd.algorithm import DefaultSelection
    from evogp_amd.parallel import default_lists

    meta, (gen,) = dr.load("nan_inf")
    forest = dr.forest_of(gen.forest, meta, "cpu")
    fit = torch.from_numpy(gen.fitness)
    n_real = int((~torch.isnan(fit)).sum())
    for kw in (meta["selection"], dict(survival_rate=1.0, elite_cnt=n_real), dict(survival_rate=0.99, elite_cnt=n_real + 3),
               dict(survival_rate=0.1, elite_cnt=395)):
        sel = DefaultSelection(**kw)
        e, p = sel(forest, fit)
        assert not torch.isnan(fit[e.long()][:n_real]).any() and not torch.isnan(fit[p.long()][:n_real]).any()
        assert dr.sets_of(e.numpy(), p.numpy()) == dr.sets_of(*(x.numpy() for x in default_lists(fit, *sel.counts(gen.pop))))
    # -0.0 and +0.0 tie by index
    z = torch.tensor([0.0, -0.0, 1.0, -0.0, 0.0, float("nan"), float("-inf")])
    e, p = DefaultSelection(1.0, elite_cnt=3)(dr.forest_of(tuple(a[:7] for a in gen.forest), meta, "cpu"), z)
    assert e.tolist() == [2, 0, 1] and p.tolist() == [2, 0, 1, 3, 4, 6, 5]


def test_replayer_refuses_a_run_that_draws_differently():
    """the replayer itself: another shape, dtype, bound or order fails, and so do draws left over"""
    _, (gen,) = dr.load("base")
    n = gen.log[0][1].shape[1]
    hi = gen.log[0][0]["high"]
    with dr.Replayer(gen.log[:2]) as r:
        a = torch.randint(0, hi, (2, n), dtype=torch.int32, device="cpu")
        b = torch.randint(low=0, high=2**31 - 1, size=(2, n), dtype=torch.int32)
    assert np.array_equal(a.numpy(), gen.log[0][1]) and np.array_equal(b.numpy(), gen.log[1][1]) and r.at == 2
    assert torch.randint is not r.randint and torch.rand is not r.rand
    for bad in (lambda: torch.randint(0, hi + 1, (2, n), dtype=torch.int32), lambda: torch.randint(0, hi, (2, n + 1), dtype=torch.int32),
                lambda: torch.randint(0, hi, (2, n)), lambda: torch.rand(2, n), lambda: torch.randint(1, hi, (2, n), dtype=torch.int32)):
        with pytest.raises(AssertionError):
            with dr.Replayer(gen.log):
                bad()
    with pytest.raises(AssertionError, match="never requested"):
        with dr.Replayer(gen.log):
            torch.randint(0, hi, (2, n), dtype=torch.int32)
    with pytest.raises(AssertionError, match="holds only"):
        with dr.Replayer(gen.log[:1]):
            torch.randint(0, hi, (2, n), dtype=torch.int32)
            torch.rand(n)
