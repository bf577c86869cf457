"""Cost of the pairwise semantic moments (csrc/sr_pair.hip; Forest.SR_pair_moments) and what a semantically chosen mate does to a
run (SemanticMate, SemanticMateCrossover, ApproxGeometricCrossover(mate=)).  Device events around every call after a warm-up call, medians
of --reps repetitions, all in ONE process; writes one JSON object to --out (profiles/pair_moments_bench.json) and prints it.  No time is
fixed in advance.

Forests: configs[1] (100 k trees x 1024 rows, 10 variables, gp_len 64, + - * /) fresh, the same run after --generations generations of
DefaultSelection(0.3, elite_rate=0.01) / DefaultCrossover / DefaultMutation(0.2, depth-3 donors), and the fresh 1 M headline forest.
Per forest, with E = pop events of uniformly drawn indices and M candidates each:
  pairs_ms[M]                       tree_SR_pair_moments
  scaling_ms                        tree_SR_linear_scaling on the same forest, the yardstick: one interpretation per tree, three float64 sums
  per_interpretation_over_scaling   (pairs_ms / ((M + 1) E)) / (scaling_ms / pop): the cost model says about 1
  nan_share                         pairs whose words are NaN
"torch": batch_forward + float64 torch on (n, D) matrices next to the op, on a slice of --slice trees, M = 8.
"evolution" (--only evolution, or all): 10 000 trees, --generations generations, three seeds, the benchmark's 10-variable target,
DefaultMutation in all arms: ApproxGeometricCrossover with uniform mates against mate=SemanticMate("midpoint") and ("blend");
DefaultCrossover against SemanticMateCrossover("angle") and ("competent").  An illustration, not a statistic.
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


def measure(forest, X, y, reps, Ms):
    v, t, s = forest._tensors()
    pop, L = v.shape
    ops = torch.ops.evogp_hip
    y1 = y[:, 0].contiguous()
    torch.manual_seed(7)
    first = torch.randint(0, pop, (pop,), dtype=torch.int32, device=v.device)
    out = {"pop": pop, "gp_len": L, "rows": int(X.shape[0]), "events": pop, "pairs_ms": {}, "per_interpretation_over_scaling": {}}
    out["scaling_ms"] = times(lambda: ops.tree_SR_linear_scaling(pop, X.shape[0], L, X.shape[1], 1, v, t, s, X, y), reps)
    per_tree = out["scaling_ms"]["median"] / pop
    for M in Ms:
        cand = torch.randint(0, pop, (pop, M), dtype=torch.int32, device=v.device)
        call = lambda: ops.tree_SR_pair_moments(v, t, s, v, t, s, X, y1, first, cand)   # noqa: E731
        out["pairs_ms"][str(M)] = times(call, reps)
        out["per_interpretation_over_scaling"][str(M)] = out["pairs_ms"][str(M)]["median"] / ((M + 1) * pop) / per_tree
        if M == Ms[-1]:
            out["nan_share"] = float(torch.isnan(call()[1][..., 0]).double().mean())
    print(f"# {pop} trees: scaling {out['scaling_ms']['median']:.3f} ms, pairs "
          + ", ".join(f"M={m} {r['median']:.3f} ms" for m, r in out["pairs_ms"].items()), file=sys.stderr, flush=True)
    return out


def torch_route(forest, X, y, reps, n, M):
    """the same numbers through batch_forward and float64 torch on a slice small enough to materialise"""
    sub = forest[:n]
    v, t, s = sub._tensors()
    y1 = y[:, 0].contiguous()
    torch.manual_seed(9)
    first = torch.randint(0, n, (n,), dtype=torch.int32, device=v.device)
    cand = torch.randint(0, n, (n, M), dtype=torch.int32, device=v.device)

    def by_torch():
        P = sub.batch_forward(X)[:, :, 0].double()
        R = P - y1.double()[None, :]
        ra, rb = R[first.long()], R[cand.long()]
        return (ra * ra).sum(1), torch.stack([(rb * rb).sum(2), (ra[:, None] * rb).sum(2), ((P[first.long()][:, None] - P[cand.long()]) ** 2).sum(2)], 2)

    return {"trees": n, "M": M, "op_ms": times(lambda: torch.ops.evogp_hip.tree_SR_pair_moments(v, t, s, v, t, s, X, y1, first, cand), reps),
            "torch_ms": times(by_torch, reps)}


def evolve(X, y, seed, generations, pop, arm):
    """the loss of the best tree after every generation"""
    from bench_backprop import descriptor
    from evogp_amd.algorithm import (ApproxGeometricCrossover, DefaultCrossover, DefaultMutation, DefaultSelection, GeneticProgramming, SemanticMate,
                                     SemanticMateCrossover)
    from evogp_amd.problem import SymbolicRegression
    from evogp_amd.tree import Forest

    torch.manual_seed(seed)
    d, sub = descriptor(5), descriptor(3)
    kind, criterion = arm
    mate = SemanticMate(X, y, candidates=8, criterion=criterion) if criterion else None
    if kind == "agx":
        crossover = ApproxGeometricCrossover(X, descriptor=sub, library_size=1000, fallback=DefaultCrossover(), mate=mate)
    else:
        crossover = SemanticMateCrossover(mate) if mate else DefaultCrossover()
    algo = GeneticProgramming(Forest.random_generate(pop, d, keys=torch.tensor([seed, 1], dtype=torch.uint32, device=X.device)), crossover,
                              DefaultMutation(0.2, sub), DefaultSelection(0.3, elite_rate=0.01))
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
    return {"best_loss": curve, "seconds": time.perf_counter() - t0}


ARMS = {"agx_uniform": ("agx", None), "agx_midpoint": ("agx", "midpoint"), "agx_blend": ("agx", "blend"),
        "default": ("default", None), "mate_angle": ("default", "angle"), "mate_competent": ("default", "competent")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["all", "forests", "evolution"], default="all")
    ap.add_argument("--evolve-pop", type=int, default=10_000)
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--generations", type=int, default=30)
    ap.add_argument("--pop", type=int, default=100_000)
    ap.add_argument("--slice", type=int, default=10_000)
    ap.add_argument("--headline-pop", type=int, default=1_000_000, help="0 skips the headline forest")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_moments_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_pairs.py measures on the GPU only"
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
        result["forests"]["configs1_generation_0"] = measure(algo.forest, X, y, args.reps, [1, 4, 8, 16])
        result["torch"] = torch_route(algo.forest, X, y, args.reps, args.slice, 8)
        for _ in range(args.generations):
            algo.step(torch.ops.evogp_hip.fitness_scores(algo.forest.SR_fitness(X, y), True))
        result["forests"]["configs1_generation_%d" % args.generations] = measure(algo.forest, X, y, args.reps, [1, 4, 8, 16])
        del algo
        if args.headline_pop:
            torch.cuda.empty_cache()
            big = Forest.random_generate(args.headline_pop, desc, keys=keys)
            result["forests"]["headline_generation_0"] = measure(big, X, y, args.reps, [8])
            del big
    if args.only != "forests":
        result["evolution"] = {"pop": args.evolve_pop, "generations": args.generations,
                               "runs": [dict({"seed": sd}, **{name: evolve(X, y, sd, args.generations, args.evolve_pop, arm)
                                                              for name, arm in ARMS.items()}) for sd in args.seeds]}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
