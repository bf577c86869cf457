"""Replay a recorded run of the REFERENCE's default generation step (tests/golden/default_step_*.npz, written by
tests/golden/make_default_step_golden.py: DefaultSelection -> DefaultCrossover -> DefaultMutation inside
GeneticProgramming.step, genetic_programming.py:101-120, with every random number and every intermediate recorded).

A fixture becomes two things here:
  * `replay_args`: the arguments of the C ABI breeding passes (tests/gpu_capi.py breed_default / breed_lists) and of `_expected`,
    the restatement of the step the large breeding tests of tests/test_gpu_breed.py compare the kernels with;
  * `Replayer`: a context manager under which torch.rand / torch.randint hand out the recorded draws in order, so that this
    repository's composed operators (GeneticProgramming._breed without the fused pass) run on the reference's own numbers.
`edges` derives, from the arrays alone, the edge conditions every case was recorded for."""
import json
import os

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("base", "all_mutate_overflow", "no_mutation", "multi_output", "row50", "row400", "ties", "nan_inf", "more_elites_than_parents",
         "one_parent", "two_generations_pareto")
INACTIVE = 2**31 - 2      # the largest raw word: never below a threshold


# ---- the restatement of the step -------------------------------------------------------------------------------------------------
def _expected(oracle, forest, order, rnd, below, n_elite, n_surv, donors, parents=None, pop=None):
    """What the reference's operators produce for these draws (genetic_programming.py:110-122: elites = forest[elite indices],
    parents drawn from forest[survivor indices] — a list that may repeat trees)."""
    v, t, s = forest
    pop = v.shape[0] if pop is None else pop
    L = v.shape[1]
    n_new = pop - n_elite
    sizes = s[:, 0].astype(np.int64)
    r = rnd.astype(np.int64)
    parents = order if parents is None else parents
    li = parents[r[0] % n_surv]
    ri = parents[r[1] % n_surv]
    p = (r[2] % sizes[li]).astype(np.int32)
    q = (r[3] % sizes[ri]).astype(np.int32)
    child = [a.copy() for a in oracle.crossover(v, t, s, li.astype(np.int32), ri.astype(np.int32), p, q)]
    mut = r[4] < below
    pm = np.full(n_new, -1, np.int32)
    if mut.any():
        cs = child[2][mut, 0].astype(np.int64)
        pm_m = ((r[5][mut] % 1024) % cs).astype(np.int32)
        pm[mut] = pm_m
        res = oracle.mutate(child[0][mut], child[1][mut], child[2][mut], pm_m, donors[0][mut], donors[1][mut], donors[2][mut])
        for a, b in zip(child, res):
            a[mut] = b
    elite = order[:n_elite]
    out = tuple(np.concatenate([src[elite], ch]) for src, ch in zip((v, t, s), child))
    dec = np.stack([li, ri, p, q, mut.astype(np.int64), pm], axis=1).astype(np.int32)
    return out, dec


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------
class Generation:
    """one recorded call of the reference's GeneticProgramming.step"""

    def __init__(self, z, meta, g):
        p = f"g{g}_"

        def three(name):
            return tuple(z[p + name + "_" + k] for k in ("value", "type", "size")) if p + name + "_value" in z.files else None

        self.meta = meta
        self.L = int(z[p + "in_value"].shape[1])
        self.forest = three("in")
        self.fitness = z[p + "fitness"]
        self.elite, self.survivor = z[p + "elite"], z[p + "survivor"]
        self.full_order = z[p + "full_order"]          # the reference's selection asked for every tree: its whole ranking
        self.offspring = three("off")
        self.donors = three("donor")                    # the compact donor forest (one row per mutated offspring), or None
        self.keys = z[p + "keys"] if p + "keys" in z.files else None
        self.mask = z[p + "mask"]
        self.out = three("out")
        self.xo = tuple(z[p + "xo_" + k] for k in ("left", "right", "lpos", "rpos"))   # the arguments of the reference's tree_crossover call
        self.mut_pos = z[p + "mut_pos"] if p + "mut_pos" in z.files else None           # ... and of its tree_mutate call
        self.log = [(e, z[p + f"log{i}"]) for i, e in enumerate(meta["log"][g])]
        self.front = ((z[p + "front_fitness"],) + three("front")) if p + "front_fitness" in z.files else None

    @property
    def pop(self):
        return self.forest[0].shape[0]


def load(case):
    """-> (meta, [Generation, ...])"""
    z = np.load(os.path.join(GOLD, f"default_step_{case}.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    return meta, [Generation(z, meta, g) for g in range(meta["generations"])]


def replay_args(gen):
    """The recorded generation as the arguments of gpu_capi.breed_default / breed_lists and of `_expected`."""
    n_elite, n_surv = len(gen.elite), len(gen.survivor)
    n_new = gen.pop - n_elite
    longer, shorter = (gen.elite, gen.survivor) if n_elite >= n_surv else (gen.survivor, gen.elite)
    assert np.array_equal(longer[:len(shorter)], shorter), "the reference's two lists are prefixes of one ranking"
    tags = [e["tag"] for e, _ in gen.log]
    assert tags[:3] == ["torch_randint", "torch_randint", "rand"] and len(tags) in (3, 5), tags
    parents, unlimited = gen.log[0][1], gen.log[1][1]
    assert parents.shape == unlimited.shape == (2, n_new) and gen.mask.shape == (n_new,)
    mutated = len(tags) == 5
    rnd = np.zeros((6, n_new), np.int32)
    rnd[0:2], rnd[2:4] = parents, unlimited
    rnd[4] = np.where(gen.mask, 0, INACTIVE)
    L = gen.L
    donors = (np.full((n_new, L), np.nan, np.float32), np.full((n_new, L), -7, np.int16), np.full((n_new, L), -7, np.int16))   # poison
    if mutated:
        positions = gen.log[4][1]
        assert positions.shape == (int(gen.mask.sum()),) and int(positions.max()) < 1024 and int(positions.min()) >= 0
        rnd[5][gen.mask] = positions
        for full, compact in zip(donors, gen.donors):
            full[gen.mask] = compact
    else:
        assert not gen.mask.any() and gen.donors is None
    return dict(order=longer.astype(np.int32), elites=gen.elite.astype(np.int32), parents=gen.survivor.astype(np.int32), rnd=rnd,
                below=1 if mutated else 0, n_elite=n_elite, n_surv=n_surv, donors=donors)


def recorded_decisions(gen):
    """int32[n_new][6] = {left tree, right tree, left position, right position, mutated, mutation position or -1}: what the
    reference handed to its tree_crossover and tree_mutate calls, the parents as population indices"""
    left, right, lpos, rpos = (a.astype(np.int64) for a in gen.xo)
    pm = np.full(len(left), -1, np.int64)
    if gen.mut_pos is not None:
        pm[gen.mask] = gen.mut_pos
    surv = gen.survivor.astype(np.int64)
    return np.stack([surv[left], surv[right], lpos, rpos, gen.mask.astype(np.int64), pm], axis=1).astype(np.int32)


def descriptors(meta, device=None):
    """-> (the population's GenerateDescriptor, the donors' one) of this repository"""
    from evogp_amd.tree import GenerateDescriptor, set_default_device

    if device is not None:
        set_default_device(device)
    desc = GenerateDescriptor(**meta["descriptor"])
    return desc, desc.update(**meta["donor_update"])


def forest_of(arrays, meta, device):
    from evogp_amd.tree import Forest

    d = meta["descriptor"]
    return Forest(d["input_len"], d["output_len"], *(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in arrays))


def forest_np(f):
    return f.batch_node_value.cpu().numpy(), f.batch_node_type.cpu().numpy(), f.batch_subtree_size.cpu().numpy()


# ---- the edge conditions, from the arrays ---------------------------------------------------------------------------------------------
def edges(gen):
    """Counters of the edges a generation exercises, derived from its arrays alone (the recorder stores them in `meta`, the tests
    derive them again: a regenerated fixture cannot silently lose one)."""
    v, t, s = gen.forest
    L = gen.L
    surv = gen.survivor.astype(np.int64)
    left, right, lpos, rpos = (a.astype(np.int64) for a in gen.xo)
    ps = s[surv].astype(np.int64)                                   # the survivor forest's sizes
    child_len = ps[left, 0] - ps[left, lpos] + ps[right, rpos]
    too_long = child_len > L
    fell_back = all(np.array_equal(o[too_long], src[surv[left[too_long]]]) for o, src in zip(gen.offspring, (v, t, s)))
    drawn = np.bincount(np.concatenate([left, right]), minlength=len(surv))
    out = dict(children=int(len(left)), self_crossover=int((left == right).sum()), parents_drawn_twice=int((drawn > 1).sum()),
               child_too_long=int(too_long.sum()), child_too_long_is_left_parent=bool(fell_back), mutated=int(gen.mask.sum()),
               mutant_too_long=0, survivors=int(len(surv)), elites=int(len(gen.elite)), draws=[e["tag"] for e, _ in gen.log])
    if gen.mut_pos is not None:
        cs = gen.offspring[2][gen.mask].astype(np.int64)
        pos = gen.mut_pos.astype(np.int64)
        mutant_len = cs[:, 0] - cs[np.arange(len(pos)), pos] + gen.donors[2][:, 0].astype(np.int64)
        out["mutant_too_long"] = int((mutant_len > L).sum())
    f = gen.fitness
    out["nan_elites"] = int(np.isnan(f[gen.elite]).sum())
    out["nan"], out["neg_inf"], out["pos_inf"] = int(np.isnan(f).sum()), int(np.isneginf(f).sum()), int(np.isposinf(f).sum())
    out["neg_zero"] = int(((f == 0) & np.signbit(f)).sum())
    out["pos_zero"] = int(((f == 0) & ~np.signbit(f)).sum())
    out["distinct_fitness"] = int(len(np.unique(f[~np.isnan(f)])))
    out["tie_at_elites"], out["tie_at_survivors"] = (bool(tie_straddles(f, n)) for n in (len(gen.elite), len(gen.survivor)))
    return out


def check_edges(name, e):
    """the conditions a case is recorded for (e: `edges` of every generation)"""
    for g in e:
        assert g["child_too_long_is_left_parent"]
    e = e[0]
    share = e["mutated"] / e["children"]
    if name == "all_mutate_overflow":
        assert e["child_too_long"] >= 1 and e["mutant_too_long"] >= 1 and share == 1.0, e
    if name in ("base", "row50", "row400", "multi_output"):
        assert e["self_crossover"] >= 1 and e["parents_drawn_twice"] >= 1 and 0 < share < 1, e
    if name == "no_mutation":
        assert e["draws"] == ["torch_randint", "torch_randint", "rand"] and e["mutated"] == 0, e
    if name == "ties":
        assert e["distinct_fitness"] == 5 and e["tie_at_elites"] and e["tie_at_survivors"], e
    if name == "nan_inf":
        assert e["nan_elites"] >= 1 and e["nan"] >= 1 and e["neg_inf"] >= 1 and e["pos_inf"] >= 1 and e["neg_zero"] >= 1 and e["pos_zero"] >= 1, e
    if name == "more_elites_than_parents":
        assert e["elites"] > e["survivors"], e
    if name == "one_parent":
        assert e["survivors"] == 1 and e["self_crossover"] == e["children"], e


def tie_straddles(fitness, n):
    """the n-th and (n+1)-th best fitness values are equal: which tree a list of n takes is a matter of tie breaking"""
    if not 0 < n < len(fitness):
        return False
    nan = np.isnan(fitness)
    ranked = np.concatenate([np.sort(fitness[~nan])[::-1], fitness[nan]])     # NaN behind -inf
    a, b = ranked[n - 1], ranked[n]
    return bool(a == b or (np.isnan(a) and np.isnan(b)))


def nan_last(order, fitness):
    """a ranking with every NaN entry moved behind all others, the relative order inside both groups kept"""
    order = np.asarray(order)
    nan = np.isnan(fitness[order])
    return np.concatenate([order[~nan], order[nan]])


# ---- replaying the draws ---------------------------------------------------------------------------------------------------------------
def _shape(size):
    if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
        size = size[0]
    return tuple(int(x) for x in size)


class Replayer:
    """`with Replayer(gen.log):` torch.rand and torch.randint return the recorded draws, in order, on the requested device.  A request
    whose kind, shape, dtype or bounds differ from the recording's next entry fails, and so do draws left over at the end."""

    def __init__(self, log):
        self.log = list(log)
        self.at = 0

    def _next(self, tag, shape, dtype, device, low=None, high=None):
        assert self.at < len(self.log), f"draw {self.at}: {tag}{shape} requested, but the recording holds only {len(self.log)} draws"
        e, a = self.log[self.at]
        what = f"draw {self.at}: requested {tag}{shape} {dtype} [{low}, {high}), recorded {e}"
        assert e["tag"] == tag and tuple(e["shape"]) == shape and e["dtype"] == str(dtype).replace("torch.", ""), what
        assert e.get("low") == low and e.get("high") == high, what
        self.at += 1
        return torch.from_numpy(a.copy()).to(device if device is not None else "cpu")

    def rand(self, *size, dtype=None, device=None, **kw):
        return self._next("rand", _shape(size), dtype or torch.float32, device)

    def randint(self, *args, **kw):
        # torch.randint(high, size, ...) or torch.randint(low, high, size, ...), any of them by keyword
        kw.update(zip(("high", "size") if len(args) == 2 else ("low", "high", "size"), args))
        return self._next("torch_randint", _shape((kw["size"],)), kw.get("dtype") or torch.int64, kw.get("device"), int(kw.get("low", 0)),
                          int(kw["high"]))

    def __enter__(self):
        self._saved = (torch.rand, torch.randint)
        torch.rand, torch.randint = self.rand, self.randint
        return self

    def __exit__(self, exc_type, exc, tb):
        torch.rand, torch.randint = self._saved
        if exc_type is None:
            assert self.at == len(self.log), f"{len(self.log) - self.at} recorded draws were never requested (from draw {self.at} on)"
        return False


class Tap:
    """an operator that keeps a copy of the forest it is handed (the offspring after crossover) before the wrapped one runs"""

    def __init__(self, op):
        self.op = op
        self.seen = None

    def __call__(self, forest):
        self.seen = tuple(a.copy() for a in forest_np(forest))
        return self.op(forest)


def composed_step(algo, gen, fitness):
    """one `step` of this repository's GeneticProgramming on the recorded draws -> (next forest, the offspring after crossover)"""
    tap = Tap(algo.mutation)
    algo.mutation = tap
    try:
        with Replayer(gen.log):
            nxt = algo.step(fitness)
    finally:
        algo.mutation = tap.op
    return nxt, tap.seen


# ---- the checks the CPU and the GPU tests share ----------------------------------------------------------------------------------------
OWN_ORDER = ("nan_inf", "ties")     # cases whose lists are not the reference's, entry by entry: see RecordedLists


class RecordedLists:
    """a selection that hands back the reference's recorded lists, for the two cases where ours differ on purpose: `nan_inf` (NaN
    ranks last here) and `ties` (equal fitness is listed by tree index here, the sort being stable, and in whatever order torch's
    unstable sort leaves it in the reference; a parent draw r then names another tree of the same fitness)"""

    def __init__(self, gens):
        self.gens = iter(gens)

    def __call__(self, forest, fitness):
        gen = next(self.gens)
        return torch.from_numpy(gen.elite).to(fitness.device), torch.from_numpy(gen.survivor).to(fitness.device)


def make_algorithm(meta, gens, device):
    from evogp_amd.algorithm import DefaultCrossover, DefaultMutation, DefaultSelection, GeneticProgramming

    _, donor_desc = descriptors(meta, device)
    selection = RecordedLists(gens) if meta["case"] in OWN_ORDER else DefaultSelection(**meta["selection"])
    return GeneticProgramming(forest_of(gens[0].forest, meta, device), DefaultCrossover(), DefaultMutation(meta["mutation_rate"], donor_desc),
                              selection, enable_pareto_front=meta["pareto"])


def check_composed_path(case, device):
    """the composed operators of this repository, run generation by generation on a fixture's draws, give the reference's offspring,
    population and (where recorded) Pareto front"""
    from helpers import assert_forest_equal

    meta, gens = load(case)
    algo = make_algorithm(meta, gens, device)
    assert algo._native_plan() is None
    for g, gen in enumerate(gens):
        assert_forest_equal(forest_np(algo.forest), gen.forest, f"{case}: input of generation {g}")
        nxt, offspring = composed_step(algo, gen, torch.from_numpy(gen.fitness).to(device))
        assert_forest_equal(offspring, gen.offspring, f"{case}: offspring after crossover, generation {g}")
        assert_forest_equal(forest_np(nxt), gen.out, f"{case}: population after generation {g}")
        if meta["pareto"]:
            front = algo.pareto_front
            assert np.array_equal(front.fitness.cpu().numpy().view(np.uint32), gen.front[0].view(np.uint32)), f"{case}: front fitness, generation {g}"
            assert_forest_equal(forest_np(front.solution), gen.front[1:], f"{case}: front solutions, generation {g}")


def sets_of(elites, parents):
    """(the elite set, the set of the other survivors) of two index lists"""
    e, p = set(np.asarray(elites).tolist()), set(np.asarray(parents).tolist())
    assert len(e) == len(elites) and len(p) == len(parents), "an index is listed twice"
    return e, p - e


def check_selection(case, gen, elites, parents):
    """two lists of ours against the reference's recorded ones, by the rule of the issue: equal sets where no tie straddles a
    threshold, equal multisets of selected fitness values where one does, and for NaN the asserted deviation"""
    f = gen.fitness
    n_elite, n_surv = len(gen.elite), len(gen.survivor)
    assert len(elites) == n_elite and len(parents) == n_surv
    got = sets_of(elites, parents)
    if np.isnan(f).any():
        assert case == "nan_inf"
        ranking = nan_last(gen.full_order, f)
        assert np.array_equal(gen.full_order[:n_elite], gen.elite) and np.array_equal(gen.full_order[:n_surv], gen.survivor)
        assert np.isnan(f[gen.elite]).any() and not np.isnan(f[ranking[:n_surv]]).any()      # the deviation is exercised
        assert not tie_straddles(f, n_elite) and not tie_straddles(f, n_surv)
        assert got == sets_of(ranking[:n_elite], ranking[:n_surv])
        assert got != sets_of(gen.elite, gen.survivor)
        return
    want = sets_of(gen.elite, gen.survivor)
    if tie_straddles(f, n_elite) or tie_straddles(f, n_surv):
        assert case == "ties"
        for a, b in zip(got, want):
            assert sorted(f[sorted(a)].tolist()) == sorted(f[sorted(b)].tolist())
    else:
        assert got == want
