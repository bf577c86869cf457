"""GPU: the kernels of the default generation step against recorded runs of the REFERENCE's own Python operators -- see
tests/test_default_step_parity.py and tests/golden/make_default_step_golden.py.  Reads tests/golden only.  Bit for bit, whole rows.

The chain that ties every form of the step to the reference:
    reference's GeneticProgramming.step, recorded          (tests/golden/default_step_*.npz)
 -> the array forms: evogp_hip_generate, evogp_hip_breed_default, evogp_hip_breed_lists, torch.ops.evogp_hip.breed_rows,
    select_survivors, and the composed operators on the device                                        (this file)
 -> the hashed forms evogp_hip_generate_masked_hashed / evogp_hip_breed_lists_hashed that GeneticProgramming.step runs
                                                      (tests/test_gpu_breed.py test_hashed_words_equal_the_array_forms)
The fused hashed step computes counter-based words in the kernels and cannot replay a recording; it replaces the reference's
draws one for one -- words 0, 1 the two parent indices, 2, 3 the two unlimited positions, 4 the Bernoulli number of the mutation
mask (word < rate * (2^31 - 1) instead of rand < rate), 5 the mutation position (word % 1024), words (7, 0) and (7, 1) modulo 10^6
the two generation keys -- and generates a donor per mutating SLOT (seeded by the slot) where the reference generates a compact
forest (seeded by the rank among the mutating trees): the replay scatters the compact donors into the slots.

`ties` and `nan_inf` breed from the reference's recorded lists: our selection lists equal fitness by tree index and NaN last, on
purpose (tests/default_step_replay.py OWN_ORDER); the selection test asserts exactly that deviation."""
import numpy as np
import pytest

import default_step_replay as dr
from helpers import assert_forest_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    import gpu_capi

    return gpu_capi


@pytest.fixture(scope="module")
def recorded():
    """every fixture, loaded once: case -> (meta, generations, replay arguments per generation)"""
    out = {}
    for case in dr.CASES:
        meta, gens = dr.load(case)
        out[case] = (meta, gens, [dr.replay_args(gen) for gen in gens])
    return out


@pytest.fixture
def device():
    import torch

    import evogp_amd  # noqa: F401
    from evogp_amd.tree import default_device, set_default_device

    old = default_device()
    set_default_device("cuda:0")
    yield torch.device("cuda", 0)
    set_default_device(old)


@pytest.mark.parametrize("case", dr.CASES)
def test_generate_gives_the_recorded_donors(g, recorded, device, case):
    """evogp_hip_generate with the two recorded keys = the compact donor forest of the reference's Forest.random_generate; the tables
    are those of this repository's GenerateDescriptor"""
    meta, gens, _ = recorded[case]
    _, d = dr.descriptors(meta)
    for gen in gens:
        if gen.donors is None:     # rate 0: the reference returns before it draws keys (mutation/default.py:46-47)
            assert case == "no_mutation" and gen.keys is None and len(gen.log) == 3
            continue
        n = int(gen.mask.sum())
        assert n == gen.donors[0].shape[0] and gen.keys.shape == (2,)
        got = g.generate(n, gen.L, d.input_len, d.output_len, d.out_prob, d.const_prob, gen.keys, d.depth2leaf_probs.cpu().numpy(),
                         d.roulette_funcs.cpu().numpy(), d.const_samples.cpu().numpy())
        assert_forest_equal(got, gen.donors, f"{case}: donors")


@pytest.mark.parametrize("case", dr.CASES)
def test_breed_default_reproduces_the_reference(g, recorded, case):
    """evogp_hip_breed_default on the recorded ranking and draws.  `order` is the longer of the reference's two lists, both being
    prefixes of one ranking, so `more_elites_than_parents` is expressed like every other case."""
    _, gens, args = recorded[case]
    for gen, a in zip(gens, args):
        got, dec = g.breed_default(*gen.forest, a["order"], a["rnd"], a["below"], a["n_elite"], a["n_surv"], *a["donors"])
        assert np.array_equal(dec, dr.recorded_decisions(gen)), f"{case}: decisions differ"
        assert_forest_equal(got, gen.out, f"{case}: breed_default")


@pytest.mark.parametrize("case", dr.CASES)
def test_breed_lists_reproduces_the_reference(g, recorded, device, case):
    """evogp_hip_breed_lists on the reference's two lists: the whole population, three ragged slices, and the torch op"""
    import torch

    _, gens, args = recorded[case]
    for gen, a in zip(gens, args):
        pop, n_elite = gen.pop, a["n_elite"]
        pad = [np.concatenate([np.full((n_elite, gen.L), fill, x.dtype), x]) for x, fill in zip(a["donors"], (np.nan, -7, -7))]
        got, dec = g.breed_lists(*gen.forest, a["elites"], a["parents"], a["rnd"], a["below"], *pad)
        assert np.array_equal(dec[n_elite:], dr.recorded_decisions(gen)), f"{case}: decisions differ"
        assert_forest_equal(got, gen.out, f"{case}: breed_lists")
        cuts = [0, pop // 3 + 1, pop // 3 + 2, pop]
        parts = [g.breed_lists(*gen.forest, a["elites"], a["parents"], a["rnd"], a["below"], *[x[lo:hi] for x in pad], pop=pop, row_begin=lo,
                               row_count=hi - lo)[0] for lo, hi in zip(cuts[:-1], cuts[1:])]
        assert_forest_equal(tuple(np.concatenate([p[k] for p in parts]) for k in range(3)), gen.out, f"{case}: breed_lists in slices")
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device)  # noqa: E731
        out = torch.ops.evogp_hip.breed_rows(pop, gen.L, *(t(x) for x in gen.forest), t(a["elites"]), t(a["parents"]), t(a["rnd"]), a["below"],
                                             *(t(x) for x in pad), 0, pop)
        assert_forest_equal(tuple(x.cpu().numpy() for x in out), gen.out, f"{case}: breed_rows")


@pytest.mark.parametrize("case", dr.CASES)
def test_select_survivors_agrees_with_the_reference(recorded, device, case):
    """csrc/select.hip on the recorded fitness: the reference's two sets, by the rule of tests/default_step_replay.py
    check_selection (`nan_inf`: the reference's ranking with NaN moved behind -inf); DefaultSelection.__call__ on the device gives
    the same sets"""
    import torch

    from evogp_amd.algorithm import DefaultSelection
    from evogp_amd.parallel import default_lists

    meta, gens, _ = recorded[case]
    sel = DefaultSelection(**meta["selection"])
    for gen in gens:
        fit = torch.from_numpy(gen.fitness).to(device)
        n_elite, n_surv = sel.counts(gen.pop)
        assert (n_elite, n_surv) == (len(gen.elite), len(gen.survivor))
        order = torch.ops.evogp_hip.select_survivors(fit, min(n_elite, n_surv), max(n_elite, n_surv)).cpu().numpy()
        dr.check_selection(case, gen, order[:n_elite], order[:n_surv])
        fused = tuple(x.cpu().numpy() for x in default_lists(fit, n_elite, n_surv))
        assert np.array_equal(fused[0], order[:n_elite]) and np.array_equal(fused[1], order[:n_surv])
        composed = tuple(x.cpu().numpy() for x in sel(dr.forest_of(gen.forest, meta, device), fit))
        dr.check_selection(case, gen, *composed)
        assert dr.sets_of(*composed) == dr.sets_of(*fused)


@pytest.mark.parametrize("case", dr.CASES)
def test_composed_path_on_the_device_reproduces_the_reference(g, device, monkeypatch, case):
    """GeneticProgramming with the fused pass switched off: tree_crossover, tree_mutate, tree_generate and the gathers in the
    reference's composition, on the reference's draws"""
    monkeypatch.setenv("EVOGP_NATIVE_STEP", "0")
    dr.check_composed_path(case, device)
