"""Cost and yield of the population-built subtree library (csrc/sr_subtree_sig.hip; Forest.SR_subtree_signatures / subtree_library,
SemanticLibrary.update_library(source="subtrees")).  Device events around every call after a warm-up call, --reps repetitions each, all
in ONE process; writes one JSON object to --out (profiles/subtree_library_bench.json) and prints it.  No time is fixed in advance: the
signature pass is tree_SR_subtree_errors' walk with an integer epilogue and is judged against that pass measured here, on the same
forest -- the ratio is the cost of the epilogue and of the accumulator chosen for it.

Forests: configs[1] (100 k trees x 1024 rows, 10 variables, gp_len 64, + - * /) fresh, the same run after --generations generations of
DefaultSelection(0.3, elite_rate=0.01) / DefaultCrossover / DefaultMutation(0.2, depth-3 donors), and the fresh 1 M headline forest.
Per forest:
  signatures_ms         tree_SR_subtree_signatures;  subtree_errors_ms  tree_SR_subtree_errors, the yardstick;  signatures_over_errors
  select_ms             subtree_library_select on those signatures (k 1024, every size), two sorts over pop x gp_len words
  update_subtrees_ms    SemanticLibrary.update_library(forest, source="subtrees") end to end (wall clock around a synchronised call: it
                        waits for the host twice);  update_trees_ms  update_library(forest), today's whole-tree library
  live_nodes, eligible_nodes, subtree_classes   what the selection saw;  library_subtrees / library_trees  members after the reduction
  naive                 on the first --naive-pop trees: every subtree as a row of its own (the extraction is not timed) through
                        tree_SR_semantic_hash, next to the signature pass on the same slice
"evolution" (--only evolution, or all): scripts/bench_backprop.py's illustration -- its 10-variable target, 10 000 trees, 30 generations,
three seeds, SemanticBackpropMutation(0.2, library_size=1000, fallback=DefaultMutation) -- with the library static against
refresh_every=5, refresh_max_size=7.  An illustration, not a statistic.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_dedup import dataset  # noqa: E402
from bench_semantics import times  # noqa: E402


def wall(fn, reps):
    """{median, min, max} in ms of the wall-clock time of one synchronised call over reps calls, after one warm-up call"""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}


def all_subtree_rows(forest, limit):
    """every subtree of the first `limit` trees as a row of its own, by torch indexing on the device"""
    v, t, s = (a[:limit] for a in forest._tensors())
    L = v.shape[1]
    live = torch.arange(L, device=v.device)[None, :] < s[:, :1]
    tree, node = torch.nonzero(live, as_tuple=True)
    cols = torch.arange(L, device=v.device)[None, :]
    keep = cols < s[tree, node].to(torch.int64)[:, None]
    src = (node[:, None] + cols).clamp(max=L - 1)
    return tuple(torch.where(keep, a[tree[:, None], src], torch.zeros((), dtype=a.dtype, device=a.device)).contiguous() for a in (v, t, s))


def measure(forest, X, y, reps, naive_pop):
    from evogp_amd.algorithm import SemanticLibrary

    v, t, s = forest._tensors()
    pop, L = v.shape
    ops = torch.ops.evogp_hip
    shape = (pop, X.shape[0], L, X.shape[1], 1)
    sig = ops.tree_SR_subtree_signatures(*shape, v, t, s, X)
    member, count, n_classes = ops.subtree_library_select(sig, s, 1, L, 1024)
    out = {"pop": pop, "gp_len": L, "rows": int(X.shape[0]), "live_nodes": int(s[:, 0].to(torch.int64).clamp(0, L).sum()),
           "eligible_nodes": int((sig != 0).sum()), "subtree_classes": int(n_classes.item()), "largest_class": int(count[0].item()),
           "members_in_top_1024": int(count.sum().item())}
    out["signatures_ms"] = times(lambda: ops.tree_SR_subtree_signatures(*shape, v, t, s, X), reps)
    out["subtree_errors_ms"] = times(lambda: ops.tree_SR_subtree_errors(*shape[:5], True, v, t, s, X, y), reps)
    out["signatures_over_errors"] = out["signatures_ms"]["median"] / out["subtree_errors_ms"]["median"]
    out["select_ms"] = times(lambda: ops.subtree_library_select(sig, s, 1, L, 1024), reps)
    lib = SemanticLibrary(X, library=forest[:8])
    out["update_subtrees_ms"] = wall(lambda: lib.update_library(forest, source="subtrees"), reps)
    out["library_subtrees"] = lib.library.pop_size
    out["update_trees_ms"] = wall(lambda: lib.update_library(forest), reps)
    out["library_trees"] = lib.library.pop_size
    n = min(naive_pop, pop)
    rows = all_subtree_rows(forest, n)
    nshape = (rows[0].shape[0], X.shape[0], L, X.shape[1], 1)
    sshape = (n,) + shape[1:]
    vs, ts, ss = (a[:n].contiguous() for a in (v, t, s))
    out["naive"] = {"trees": n, "rows": int(rows[0].shape[0]),
                    "semantic_hash_of_all_subtree_rows_ms": times(lambda: ops.tree_SR_semantic_hash(*nshape, *rows, X), reps),
                    "signatures_ms": times(lambda: ops.tree_SR_subtree_signatures(*sshape, vs, ts, ss, X), reps)}
    return out


def evolve(X, y, seed, generations, pop, refresh_every):
    """the loss of the best tree after every generation (scripts/bench_backprop.py evolve, with the library's refresh as the arm)"""
    from bench_backprop import descriptor
    from evogp_amd.algorithm import DefaultCrossover, DefaultMutation, DefaultSelection, GeneticProgramming, SemanticBackpropMutation
    from evogp_amd.problem import SymbolicRegression
    from evogp_amd.tree import Forest

    torch.manual_seed(seed)
    d, sub = descriptor(5), descriptor(3)
    mutation = SemanticBackpropMutation(0.2, X, y, descriptor=sub, library_size=1000, fallback=DefaultMutation(0.2, sub),
                                        refresh_every=refresh_every, refresh_max_size=7)
    algo = GeneticProgramming(Forest.random_generate(pop, d, keys=torch.tensor([seed, 1], dtype=torch.uint32, device=X.device)), DefaultCrossover(),
                              mutation, DefaultSelection(0.3, elite_rate=0.01))
    problem = SymbolicRegression(datapoints=X, labels=y)
    best, curve = float("inf"), []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(generations):
        fitness = problem.scores(algo.forest)
        fin = torch.where(torch.isfinite(fitness), fitness, torch.full_like(fitness, float("-inf")))
        best = min(best, float(-fin.max()))
        curve.append(best)
        algo.step(fitness)
    torch.cuda.synchronize()
    return {"best_loss": curve, "seconds": time.perf_counter() - t0, "library": int(mutation.library.pop_size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["all", "forests", "evolution"], default="all")
    ap.add_argument("--evolve-pop", type=int, default=10_000)
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--generations", type=int, default=30)
    ap.add_argument("--pop", type=int, default=100_000)
    ap.add_argument("--headline-pop", type=int, default=1_000_000, help="0 skips the headline forest")
    ap.add_argument("--naive-pop", type=int, default=10_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subtree_library_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_subtree_library.py measures on the GPU only"
    from evogp_amd.algorithm import DefaultCrossover, DefaultMutation, DefaultSelection, GeneticProgramming
    from evogp_amd.tree import Forest, GenerateDescriptor

    dev = torch.device("cuda:0")
    X, y = dataset(dev)
    keys = torch.tensor([42, 0], dtype=torch.uint32, device=dev)
    desc = GenerateDescriptor(max_tree_len=64, input_len=10, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=6,
                              const_samples=[-1, 0, 1])
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "generations": args.generations, "forests": {}}

    if args.only != "forests":
        Xe, ye = X, y   # (the 10-variable target of bench_backprop.py's illustration is this dataset)
        result["evolution"] = {"pop": args.evolve_pop, "generations": args.generations, "refresh_max_size": 7,
                               "runs": [{"seed": sd, "static": evolve(Xe, ye, sd, args.generations, args.evolve_pop, 0),
                                         "refresh_every_5": evolve(Xe, ye, sd, args.generations, args.evolve_pop, 5)} for sd in args.seeds]}
    if args.only != "evolution":
        torch.manual_seed(0)
        algo = GeneticProgramming(Forest.random_generate(args.pop, desc, keys=keys), DefaultCrossover(),
                                  DefaultMutation(0.2, desc.update(max_layer_cnt=3)), DefaultSelection(0.3, elite_rate=0.01))
        result["forests"]["configs1_generation_0"] = measure(algo.forest, X, y, args.reps, args.naive_pop)
        for _ in range(args.generations):
            algo.step(torch.ops.evogp_hip.fitness_scores(algo.forest.SR_fitness(X, y), True))
        result["forests"]["configs1_generation_%d" % args.generations] = measure(algo.forest, X, y, args.reps, args.naive_pop)
        del algo
    if args.headline_pop and args.only != "evolution":
        torch.cuda.empty_cache()
        big = Forest.random_generate(args.headline_pop, desc, keys=keys)
        result["forests"]["headline_generation_0"] = measure(big, X, y, max(1, args.reps // 2), args.naive_pop)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
