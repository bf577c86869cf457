#!/usr/bin/env python3
"""Golden vectors for the default generation step: the REFERENCE's own GeneticProgramming.step with
DefaultSelection, DefaultCrossover and DefaultMutation (/root/reference/src/evogp/algorithm/genetic_programming.py:101-120,
selection/default.py, crossover/default.py, mutation/default.py) executed in this container on the CPU, with every random number
it draws and every intermediate recorded.

The set-up is that of make_mutation_golden.py, which this script imports for it: "cuda" means the CPU, the five ops run on the CPU
oracle (tests/cpu_ops.py), the reference package is imported under its own name.  On top of it
  * torch.rand / torch.randint / the reference's randint are wrapped and logged in call order, with their bounds;
  * the three operator instances are wrapped in recording callables (the two index lists, the offspring after crossover);
  * the reference Forest's crossover / mutate / random_generate and its boolean-mask gather are wrapped, so that the arguments of
    the tree_crossover and tree_mutate calls, the compact donor forest and the mutation mask are the reference's own values.
Each case stores, per generation: input forest, fitness, both index lists, the reference's whole ranking (its DefaultSelection asked
for every tree), offspring, donors with their two keys, mask, final population, the log; and a JSON `meta`.
tests/default_step_replay.py turns a fixture into kernel arguments and into a replayer of the draws;
tests/test_default_step_parity.py (CPU) and tests/test_gpu_default_step_parity.py (GPU) compare bit for bit.

    python tests/golden/make_default_step_golden.py [case ...]     (needs /root/reference; never runs on the GPU box)
"""
import json
import os
import sys

import numpy as np
import torch

import make_mutation_golden as base  # noqa: F401  (patches torch, registers the CPU ops, imports the reference as `evogp`)
from make_mutation_golden import HERE, forest_np

from evogp.algorithm import DefaultCrossover, DefaultMutation, DefaultSelection, GeneticProgramming  # noqa: E402  (the reference)
from evogp.tree import Forest, GenerateDescriptor  # noqa: E402

import default_step_replay as dr  # noqa: E402  (the edge counters the tests derive again)

# ---- recording the draws, with their bounds ---------------------------------------------------------------------------------------
LOG = []
_depth = [0]


def _rec(tag, fn):
    def wrapped(*a, **k):
        _depth[0] += 1
        try:
            r = fn(*a, **k)
        finally:
            _depth[0] -= 1
        if _depth[0] == 0:
            entry = dict(tag=tag, dtype=str(r.dtype).replace("torch.", ""), shape=list(r.shape))
            if tag == "torch_randint":
                kw = dict(k)
                kw.update(zip(("high", "size") if len(a) == 2 else ("low", "high", "size"), a))
                entry.update(low=int(kw.get("low", 0)), high=int(kw["high"]))
            LOG.append((entry, r.detach().clone().numpy()))
        return r
    return wrapped


torch.rand = _rec("rand", base._rand0)
torch.randint = _rec("torch_randint", base._randint0)
_ref_randint = _rec("ref_randint", base._ref_randint0)
for _mod in list(sys.modules.values()):
    if _mod is not None and getattr(_mod, "__name__", "").startswith("evogp.") and getattr(_mod, "randint", None) is base._ref_randint:
        _mod.randint = _ref_randint

# ---- recording the intermediates ----------------------------------------------------------------------------------------------------
CAP = {}
_generate0, _crossover0, _mutate0, _getitem0 = Forest.random_generate, Forest.crossover, Forest.mutate, Forest.__getitem__


def _np(t):
    return t.detach().clone().numpy()


def _generate(pop_size, descriptor):
    out = _generate0(pop_size, descriptor)
    CAP.setdefault("generated", []).append(forest_np(out))
    return out


def _crossover(self, left_indices, right_indices, left_pos, right_pos):
    CAP["xo"] = tuple(_np(a) for a in (left_indices, right_indices, left_pos, right_pos))
    return _crossover0(self, left_indices, right_indices, left_pos, right_pos)


def _mutate(self, replace_pos, new_sub_forest):
    CAP["mut_pos"] = _np(replace_pos)
    return _mutate0(self, replace_pos, new_sub_forest)


def _getitem(self, index):
    if isinstance(index, torch.Tensor) and index.dtype == torch.bool:
        CAP.setdefault("masks", []).append(_np(index))
    return _getitem0(self, index)


Forest.random_generate = staticmethod(_generate)
Forest.crossover, Forest.mutate, Forest.__getitem__ = _crossover, _mutate, _getitem


class Recording:
    """an operator instance wrapped: calls the reference's operator and keeps what it returned"""

    def __init__(self, op, keep):
        self.op, self.keep = op, keep

    def __call__(self, *a, **k):
        out = self.op(*a, **k)
        self.keep(out)
        return out


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
ARITH = ["+", "-", "*", "/"]
CONSTS = [-1.0, 0.0, 1.0, 0.5, 2.0]


def _normal(rng, pop):
    return rng.normal(size=pop).astype(np.float32)


def _ties(rng, pop):
    return np.clip(np.round(rng.normal(size=pop)), -2, 2).astype(np.float32)      # 5 distinct values


def _nan_inf(rng, pop):
    f = rng.normal(size=pop).astype(np.float32)
    where = rng.permutation(pop)
    n = pop // 20
    f[where[:n]] = np.nan
    f[where[n:2 * n]] = -np.inf
    f[where[2 * n:2 * n + 3]] = np.inf
    f[where[2 * n + 3:2 * n + 7]] = -0.0
    f[where[2 * n + 7:2 * n + 11]] = 0.0
    return f


# name: population, row length, descriptor kwargs, layers, donor layers, selection kwargs, mutation rate, fitness, seed, extras.
# The layer counts are the deepest the reference's GenerateDescriptor accepts for the row length and the arity of the functions
# (descriptor.py:8-31 refuses a max_layer_cnt whose complete tree does not fit); `warmup` unrecorded generations of the same
# operators then let the trees grow into the rows, which is what makes children and mutants too long for them.
CASES = {
    "base": dict(pop=400, L=64, funcs=ARITH, layers=6, donor_layers=3, sel=dict(survival_rate=0.3, elite_rate=0.01), rate=0.2, fit=_normal, seed=101),
    "all_mutate_overflow": dict(pop=300, L=32, funcs=ARITH + ["sin", "neg", "if"], layers=3, donor_layers=3, sel=dict(survival_rate=0.5, elite_cnt=7),
                                rate=1.0, fit=_normal, seed=102, warmup=4),
    "no_mutation": dict(pop=256, L=64, funcs=ARITH, layers=6, donor_layers=3, sel=dict(survival_rate=1.0), rate=0.0, fit=_normal, seed=103),
    "multi_output": dict(pop=300, L=64, funcs=["+", "*", "max", "if"], layers=4, donor_layers=3, sel=dict(survival_rate=0.3, elite_rate=0.05), rate=0.5,
                         fit=_normal, seed=104, output_len=3, out_prob=0.5),
    "row50": dict(pop=300, L=50, funcs=ARITH, layers=5, donor_layers=3, sel=dict(survival_rate=0.3, elite_rate=0.03), rate=0.4, fit=_normal, seed=105),
    "row400": dict(pop=96, L=400, funcs=ARITH, layers=8, donor_layers=5, sel=dict(survival_rate=0.4, elite_rate=0.02), rate=0.3, fit=_normal, seed=106),
    "ties": dict(pop=400, L=64, funcs=ARITH, layers=6, donor_layers=3, sel=dict(survival_rate=0.3, elite_rate=0.1), rate=0.2, fit=_ties, seed=107),
    "nan_inf": dict(pop=400, L=64, funcs=ARITH, layers=6, donor_layers=3, sel=dict(survival_rate=0.3, elite_cnt=8), rate=0.2, fit=_nan_inf, seed=108),
    "more_elites_than_parents": dict(pop=400, L=64, funcs=ARITH, layers=6, donor_layers=3, sel=dict(survival_rate=0.1, elite_cnt=120), rate=0.2,
                                     fit=_normal, seed=109),
    "one_parent": dict(pop=200, L=64, funcs=ARITH, layers=6, donor_layers=3, sel=dict(survival_rate=0.005, elite_cnt=1), rate=0.5, fit=_normal, seed=110),
    "two_generations_pareto": dict(pop=300, L=32, funcs=ARITH, layers=5, donor_layers=3, sel=dict(survival_rate=0.3, elite_rate=0.01), rate=0.3,
                                   fit=_normal, seed=111, generations=2, pareto=True),
}
LIMIT = 120 * 1024     # bytes: no fixture above the largest one committed before


def record(name, c):
    torch.manual_seed(c["seed"])
    rng = np.random.default_rng(c["seed"])
    dk = dict(max_tree_len=c["L"], input_len=4, output_len=c.get("output_len", 1), out_prob=c.get("out_prob", 0.5), using_funcs=c["funcs"],
              max_layer_cnt=c["layers"], const_samples=CONSTS)
    donor_update = dict(max_layer_cnt=c["donor_layers"])
    desc = GenerateDescriptor(**dk)
    donor_desc = GenerateDescriptor(**dict(dk, **donor_update))
    forest = Forest.random_generate(c["pop"], desc)

    def operators(keep=None):
        ops = DefaultCrossover(), DefaultMutation(c["rate"], donor_desc), DefaultSelection(**c["sel"])
        if keep is None:
            return ops
        return (Recording(ops[0], lambda out: keep.__setitem__("offspring", forest_np(out))), Recording(ops[1], lambda out: None),
                Recording(ops[2], lambda out: keep.__setitem__("lists", tuple(_np(a) for a in out))))

    warmup = c.get("warmup", 0)
    if warmup:
        algo = GeneticProgramming(forest, *operators())
        for _ in range(warmup):
            forest = algo.step(torch.from_numpy(c["fit"](rng, c["pop"])))
    algo = GeneticProgramming(forest, *operators(CAP), enable_pareto_front=c.get("pareto", False))
    generations = c.get("generations", 1)
    arrays, logs, all_edges = {}, [], []
    for g in range(generations):
        p = f"g{g}_"
        fitness = c["fit"](rng, c["pop"])
        before = forest_np(algo.forest)
        whole = _np(DefaultSelection(survival_rate=1.0)(algo.forest, torch.from_numpy(fitness))[1])
        assert sorted(whole.tolist()) == list(range(c["pop"]))
        CAP.clear()
        del LOG[:]
        out = forest_np(algo.step(torch.from_numpy(fitness)))
        log = list(LOG)
        for k, a in zip(("value", "type", "size"), before):
            arrays[p + "in_" + k] = a
        arrays[p + "fitness"] = fitness
        arrays[p + "elite"], arrays[p + "survivor"] = CAP["lists"]
        arrays[p + "full_order"] = whole.astype(np.int32)
        for k, a in zip(("value", "type", "size"), CAP["offspring"]):
            arrays[p + "off_" + k] = a
        for k, a in zip(("left", "right", "lpos", "rpos"), CAP["xo"]):
            arrays[p + "xo_" + k] = a
        n_new = c["pop"] - len(CAP["lists"][0])
        if "masks" in CAP:
            assert len(CAP["masks"]) == 1 and len(CAP["generated"]) == 1
            arrays[p + "mask"] = CAP["masks"][0]
            for k, a in zip(("value", "type", "size"), CAP["generated"][0]):
                arrays[p + "donor_" + k] = a
            keys = [a for e, a in log if e["tag"] == "torch_randint" and e["shape"] == [2] and e["high"] == 1000000]
            assert len(keys) == 1
            arrays[p + "keys"] = keys[0]
            arrays[p + "mut_pos"] = CAP["mut_pos"]
        else:
            arrays[p + "mask"] = np.zeros(n_new, bool)
        for k, a in zip(("value", "type", "size"), out):
            arrays[p + "out_" + k] = a
        for i, (e, a) in enumerate(log):
            arrays[p + f"log{i}"] = a
        logs.append([e for e, _ in log])
        if c.get("pareto"):
            arrays[p + "front_fitness"] = _np(algo.pareto_front.fitness)
            for k, a in zip(("value", "type", "size"), forest_np(algo.pareto_front.solution)):
                arrays[p + "front_" + k] = a
    meta = dict(case=name, descriptor=dk, donor_update=donor_update, selection=c["sel"], mutation_rate=c["rate"], pop=c["pop"], seed=c["seed"],
                warmup=warmup, generations=generations, pareto=bool(c.get("pareto", False)), log=logs)
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    # the edge counters, derived the way the tests derive them: from the arrays as they will be loaded
    gens = [dr.Generation(_Files(arrays), meta, g) for g in range(generations)]
    all_edges = [dr.edges(g) for g in gens]
    # the mask is the comparison the operator makes (mutation/default.py:43), and the log is rand, then keys, then positions
    for g in gens:
        assert np.array_equal(g.mask, _np(torch.from_numpy(g.log[2][1]) < c["rate"]))
        dr.replay_args(g)
    dr.check_edges(name, all_edges)
    meta["edges"] = all_edges
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    return arrays, meta


class _Files(dict):
    files = property(lambda self: list(self))


def main(names):
    for name in names or list(CASES):
        arrays, meta = record(name, CASES[name])
        again, _ = record(name, CASES[name])
        assert arrays.keys() == again.keys() and all(np.array_equal(arrays[k].view(np.uint8), again[k].view(np.uint8)) for k in arrays), (
            f"{name}: a second run recorded other arrays")
        path = os.path.join(HERE, f"default_step_{name}.npz")
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        assert size <= LIMIT, f"{name}: {size} bytes, shrink the population"
        e = meta["edges"][0]
        print(f"{name}: {size} bytes, {len(meta['log'][0])} draws per generation, {e['mutated']} of {e['children']} children mutated, "
              f"{e['child_too_long']} children / {e['mutant_too_long']} mutants too long, {e['self_crossover']} self-crossovers")


if __name__ == "__main__":
    main(sys.argv[1:])
