"""Cost and yield of exact semantic intron removal (csrc/sr_introns.hip; Forest.SR_subtree_introns / remove_introns,
SymbolicRegression(intron_removal_every=)).  Device events around every call after a warm-up call, medians of --reps repetitions, all in
ONE process; writes one JSON object to --out (profiles/introns_bench.json) and prints it.  No time is fixed in advance: the intron pass is
tree_SR_subtree_signatures' walk with a compare in place of the 64-bit epilogue, plus the candidate scan, and is judged against that pass
measured here on the same forest; the rewrite is judged against tree_prune.

Forests: configs[1] (100 k trees x 1024 rows, 10 variables, gp_len 64, + - * /) fresh, the same run after --generations generations of
DefaultSelection(0.3, elite_rate=0.01) / DefaultCrossover / DefaultMutation(0.2, depth-3 donors), and the fresh 1 M headline forest.
Per forest:
  introns_ms            tree_SR_subtree_introns (signatures given);  signatures_ms  tree_SR_subtree_signatures, the yardstick;  their ratio
  remove_ms             tree_remove_introns;  prune_ms  tree_prune (hoist and fold on the same forest's subtree errors), the yardstick
  trees_with_intron, nodes_removed, live_nodes      what the rewrite took out
  trees_without_candidate   the trees whose walk the intron pass skips (no node shares a signature with a descendant)
  gradient_before_ms / gradient_after_ms            tree_SR_gradient on the forest and on the forest without its introns
"evolution" (--only evolution, or all): 10 000 trees, --generations generations, three seeds, DefaultMutation / DefaultCrossover, the
mean tree size and the best loss per generation with and without intron_removal_every=1.  An illustration, not a statistic.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_dedup import dataset  # noqa: E402
from bench_semantics import times  # noqa: E402


def trees_without_candidate(sig, size, chunk=8192):
    """the number of trees in which no node has a descendant of its own signature (torch, in chunks of trees)"""
    pop, L = sig.shape
    cols = torch.arange(L, device=sig.device)
    none = 0
    for a in range(0, pop, chunk):
        s, z = sig[a:a + chunk], size[a:a + chunk].to(torch.int64)
        n = z[:, :1].clamp(0, L)
        span = torch.minimum(z.clamp(min=1), (n - cols[None, :]).clamp(min=1))
        below = (cols[None, None, :] > cols[None, :, None]) & (cols[None, None, :] < (cols[None, :] + span)[:, :, None])   # [t][i][j]
        hit = below & (s[:, :, None] == s[:, None, :]) & (s[:, :, None] != 0)
        none += int((~hit.flatten(1).any(1)).sum())
    return none


def measure(forest, X, y, reps):
    v, t, s = forest._tensors()
    pop, L = v.shape
    ops = torch.ops.evogp_hip
    shape = (pop, X.shape[0], L, X.shape[1], 1)
    sig = ops.tree_SR_subtree_signatures(*shape, v, t, s, X)
    rep = ops.tree_SR_subtree_introns(*shape, v, t, s, X, sig)
    nv, nt, ns, removed = ops.tree_remove_introns(v, t, s, rep)
    node_err, node_const = ops.tree_SR_subtree_errors(*shape, True, v, t, s, X, y)
    live = int(s[:, 0].to(torch.int64).clamp(0, L).sum())
    out = {"pop": pop, "gp_len": L, "rows": int(X.shape[0]), "live_nodes": live, "nodes_removed": int(removed.sum()),
           "share_of_nodes_removed": int(removed.sum()) / live, "trees_with_intron": int((removed > 0).sum()),
           "share_of_trees_with_intron": int((removed > 0).sum()) / pop}
    none = trees_without_candidate(sig, s)
    out["trees_without_candidate"], out["share_of_trees_that_skip_the_walk"] = none, none / pop
    out["introns_ms"] = times(lambda: ops.tree_SR_subtree_introns(*shape, v, t, s, X, sig), reps)
    out["signatures_ms"] = times(lambda: ops.tree_SR_subtree_signatures(*shape, v, t, s, X), reps)
    out["introns_over_signatures"] = out["introns_ms"]["median"] / out["signatures_ms"]["median"]
    out["remove_ms"] = times(lambda: ops.tree_remove_introns(v, t, s, rep), reps)
    out["prune_ms"] = times(lambda: ops.tree_prune(1, True, True, v, t, s, node_err, node_const), reps)
    out["remove_over_prune"] = out["remove_ms"]["median"] / out["prune_ms"]["median"]
    out["gradient_before_ms"] = times(lambda: ops.tree_SR_gradient(*shape, True, v, t, s, X, y), reps)
    out["gradient_after_ms"] = times(lambda: ops.tree_SR_gradient(*shape, True, nv, nt, ns, X, y), reps)
    out["gradient_after_over_before"] = out["gradient_after_ms"]["median"] / out["gradient_before_ms"]["median"]
    return out


def evolve(X, y, seed, generations, pop, every):
    """mean tree size and the loss of the best tree after every generation, through StandardPipeline's step"""
    from bench_backprop import descriptor
    from evogp_amd.algorithm import DefaultCrossover, DefaultMutation, DefaultSelection, GeneticProgramming
    from evogp_amd.pipeline import StandardPipeline
    from evogp_amd.problem import SymbolicRegression
    from evogp_amd.tree import Forest

    torch.manual_seed(seed)
    d, sub = descriptor(5), descriptor(3)
    algo = GeneticProgramming(Forest.random_generate(pop, d, keys=torch.tensor([seed, 1], dtype=torch.uint32, device=X.device)), DefaultCrossover(),
                              DefaultMutation(0.2, sub), DefaultSelection(0.3, elite_rate=0.01))
    pipe = StandardPipeline(algo, SymbolicRegression(datapoints=X, labels=y, intron_removal_every=every), is_show_details=False,
                            generation_limit=generations)
    best, curve, sizes = float("inf"), [], []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(generations):
        fitness = pipe.step()
        fin = torch.where(torch.isfinite(fitness), fitness, torch.full_like(fitness, float("-inf")))
        best = min(best, float(-fin.max()))
        curve.append(best)
        sizes.append(float(algo.forest.batch_subtree_size[:, 0].float().mean()))
    torch.cuda.synchronize()
    return {"best_loss": curve, "mean_size": sizes, "seconds": time.perf_counter() - t0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["all", "forests", "evolution"], default="all")
    ap.add_argument("--evolve-pop", type=int, default=10_000)
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--generations", type=int, default=30)
    ap.add_argument("--pop", type=int, default=100_000)
    ap.add_argument("--headline-pop", type=int, default=1_000_000, help="0 skips the headline forest")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "introns_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_introns.py measures on the GPU only"
    from evogp_amd.algorithm import DefaultCrossover, DefaultMutation, DefaultSelection, GeneticProgramming
    from evogp_amd.tree import Forest, GenerateDescriptor

    dev = torch.device("cuda:0")
    X, y = dataset(dev)
    keys = torch.tensor([42, 0], dtype=torch.uint32, device=dev)
    desc = GenerateDescriptor(max_tree_len=64, input_len=10, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=6,
                              const_samples=[-1, 0, 1])
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "generations": args.generations, "forests": {}}

    if args.only != "evolution":
        torch.manual_seed(0)
        algo = GeneticProgramming(Forest.random_generate(args.pop, desc, keys=keys), DefaultCrossover(),
                                  DefaultMutation(0.2, desc.update(max_layer_cnt=3)), DefaultSelection(0.3, elite_rate=0.01))
        result["forests"]["configs1_generation_0"] = measure(algo.forest, X, y, args.reps)
        for _ in range(args.generations):
            algo.step(torch.ops.evogp_hip.fitness_scores(algo.forest.SR_fitness(X, y), True))
        result["forests"]["configs1_generation_%d" % args.generations] = measure(algo.forest, X, y, args.reps)
        del algo
        if args.headline_pop:
            torch.cuda.empty_cache()
            big = Forest.random_generate(args.headline_pop, desc, keys=keys)
            result["forests"]["headline_generation_0"] = measure(big, X, y, args.reps)
            del big
    if args.only != "forests":
        result["evolution"] = {"pop": args.evolve_pop, "generations": args.generations,
                               "runs": [{"seed": sd, "plain": evolve(X, y, sd, args.generations, args.evolve_pop, 0),
                                         "intron_removal_every_1": evolve(X, y, sd, args.generations, args.evolve_pop, 1)} for sd in args.seeds]}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
