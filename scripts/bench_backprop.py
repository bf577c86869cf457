"""Semantic backpropagation (csrc/sr_backprop.hip) next to the pass it shares its forward walk with, and what the operator buys, on the
configs[1] forest (100 k trees x 1024 rows, 10 variables, gp_len 64, + - * /, the forest of scripts/bench_sr_grad.py) and on the 1 M
forest, in one process, alternating after warm-up:

  * tree_SR_desired (materialising desired and state, (pop, D) each);
  * tree_SR_backprop_match (fused: no (pop, D) array) at K = 64, 256 and 1024 library members (the 1 M forest: K = 256);
  * tree_SR_subtree_errors, the same forward walk with a per-node epilogue: the yardstick.

The positions are drawn as SemanticBackpropMutation draws them (a random node of every tree); the library is the semantics of K random
trees of at most three layers.  Then the loss of the best tree over 30 generations with SemanticBackpropMutation(fallback=
DefaultMutation) against DefaultMutation alone, same seed: the dataset above, 10 000 trees of gp_len 64, + - * /, DefaultSelection(0.3,
elite_rate=0.01), mutation rate 0.2, three seeds.

Device events around each call.  Prints one JSON object and writes it to --out (default profiles/backprop_bench.json).  The ratios are
recorded, not asserted."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.bench_sr_grad import dataset, timed  # noqa: E402

FUNCS = ["+", "-", "*", "/"]


def descriptor(layers, gp_len=64):
    from evogp_amd.tree import GenerateDescriptor

    return GenerateDescriptor(max_tree_len=gp_len, input_len=10, output_len=1, using_funcs=FUNCS, max_layer_cnt=layers, const_samples=[-1, 0, 1])


def measure(pop, X, y, reps, rounds, Ks):
    from evogp_amd.tree import Forest

    dev = X.device
    f = Forest.random_generate(pop, descriptor(6), keys=torch.tensor([42, 0], dtype=torch.uint32, device=dev))
    value, ntype, size = f._tensors()
    D = X.shape[0]
    hip = torch.ops.evogp_hip
    torch.manual_seed(7)
    pos = (torch.randint(0, 1024, (pop,), dtype=torch.int32, device=dev) % size[:, 0]).to(torch.int32)
    libs = {K: Forest.random_generate(K, descriptor(3), keys=torch.tensor([7, K], dtype=torch.uint32, device=dev)).batch_forward(X)[:, :, 0].contiguous()
            for K in Ks}
    calls = {"subtree_errors": lambda: hip.tree_SR_subtree_errors(pop, D, 64, 10, 1, True, value, ntype, size, X, y),
             "desired": lambda: hip.tree_SR_desired(value, ntype, size, X, y, pos)}
    for K in Ks:
        calls[f"match_k{K}"] = (lambda K=K: hip.tree_SR_backprop_match(value, ntype, size, X, y, pos, libs[K]))
    for fn in calls.values():   # warm-up
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(rounds):   # alternating, same process
        for k, fn in calls.items():
            times[k].append(timed(fn, reps))
    best = {k: min(v) for k, v in times.items()}
    print(f"# {pop} trees: " + ", ".join(f"{k} {v:.2f} ms" for k, v in best.items()), file=sys.stderr, flush=True)
    out = hip.tree_SR_backprop_match(value, ntype, size, X, y, pos, libs[Ks[-1]])
    counts, status = out[4].double(), out[5]
    return {"pop": pop, "rows": D, "var_len": 10, "gp_len": 64, "ms": best, "ms_all": times,
            "ratio_to_subtree_errors": {k: best[k] / best["subtree_errors"] for k in calls if k != "subtree_errors"},
            "status_share": [float((status == s).double().mean()) for s in range(4)],
            "row_share_required_free_impossible": (counts.sum(0) / counts.sum()).tolist(), "matched_share": float((out[0] >= 0).double().mean()),
            "finite_library_rows": {K: int(torch.isfinite(libs[K]).all(1).sum()) for K in Ks}}


def evolve(X, y, seed, generations, pop, semantic):
    """the loss of the best tree after every generation"""
    from evogp_amd.algorithm import DefaultCrossover, DefaultMutation, DefaultSelection, GeneticProgramming, SemanticBackpropMutation
    from evogp_amd.problem import SymbolicRegression
    from evogp_amd.tree import Forest

    dev = X.device
    torch.manual_seed(seed)
    d, sub = descriptor(5), descriptor(3)
    mutation = DefaultMutation(0.2, sub)
    if semantic:
        mutation = SemanticBackpropMutation(0.2, X, y, descriptor=sub, library_size=1000, fallback=DefaultMutation(0.2, sub))
    algo = GeneticProgramming(Forest.random_generate(pop, d, keys=torch.tensor([seed, 1], dtype=torch.uint32, device=dev)), DefaultCrossover(), mutation,
                              DefaultSelection(0.3, elite_rate=0.01))
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
    print(f"# seed {seed}, {'semantic backprop' if semantic else 'default'}: best loss {curve[-1]:.6g} after {generations} generations", file=sys.stderr, flush=True)
    return {"best_loss": curve, "seconds": time.perf_counter() - t0, "library": int(mutation.library.pop_size) if semantic else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--generations", type=int, default=30)
    ap.add_argument("--evolve-pop", type=int, default=10_000)
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "backprop_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    X, y = dataset(dev)
    result = {"device": torch.cuda.get_device_name(0),
              "forests": [measure(100_000, X, y, args.reps, args.rounds, [64, 256, 1024]), measure(1_000_000, X, y, args.reps, args.rounds, [256])],
              "evolution": {"pop": args.evolve_pop, "generations": args.generations,
                            "runs": [{"seed": s, "default": evolve(X, y, s, args.generations, args.evolve_pop, False),
                                      "semantic_backprop": evolve(X, y, s, args.generations, args.evolve_pop, True)} for s in args.seeds]}}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
