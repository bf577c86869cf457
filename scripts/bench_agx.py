"""The midpoint builds of semantic backpropagation (csrc/sr_backprop.hip with MID: tree_SR_desired_mid, tree_SR_agx_match) next to the
labelled builds they extend, and what the crossover built on them buys, on the configs[1] forest (100 k trees x 1024 rows, 10 variables,
gp_len 64, + - * /, the forest of scripts/bench_backprop.py) and on the 1 M forest, in one process, alternating after warm-up:

  * tree_SR_desired_mid against tree_SR_desired (materialising);
  * tree_SR_agx_match against tree_SR_backprop_match (fused) at K = 64, 256 and 1024 library members.

The mates are the forest itself under a random pairing (as ApproxGeometricCrossover pairs survivors); positions and libraries are those
of scripts/bench_backprop.py.  The cost model is the labelled pass plus one forward walk of the mate per tile.

--match-only measures tree_SR_backprop_match at K = 256 on the configs[1] forest alone and prints its rounds: run once with --root
pointing at a build of the parent commit and once on this tree, alternately (in the order parent, branch, branch, parent, so that neither
build always runs first), and hand the files to the full run as --parent-runs and --branch-runs.  The full run records both under "parent_commit_comparison": the labelled kernel must not have changed.

Then the loss of the best tree over 30 generations under DefaultCrossover against ApproxGeometricCrossover(fallback=DefaultCrossover()),
each with DefaultMutation, same seed: bench_backprop.py's target, 10 000 trees of gp_len 64, three seeds.  An illustration, not a
statistic.

Device events around each call.  Prints one JSON object and writes it to --out (default profiles/agx_bench.json).  Nothing is asserted."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _use(root):
    sys.path.insert(0, root)
    from scripts.bench_backprop import descriptor
    from scripts.bench_sr_grad import dataset, timed
    return descriptor, dataset, timed


def _setup(pop, X, Ks, descriptor):
    from evogp_amd.tree import Forest

    dev = X.device
    f = Forest.random_generate(pop, descriptor(6), keys=torch.tensor([42, 0], dtype=torch.uint32, device=dev))
    size = f._tensors()[2]
    torch.manual_seed(7)
    pos = (torch.randint(0, 1024, (pop,), dtype=torch.int32, device=dev) % size[:, 0]).to(torch.int32)
    mate = torch.randint(0, pop, (pop,), dtype=torch.int32, device=dev)
    libs = {K: Forest.random_generate(K, descriptor(3), keys=torch.tensor([7, K], dtype=torch.uint32, device=dev)).batch_forward(X)[:, :, 0].contiguous()
            for K in Ks}
    return f, pos, mate, libs


def _alternate(calls, timed, reps, rounds):
    for fn in calls.values():   # warm-up
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(rounds):   # alternating, same process
        for k, fn in calls.items():
            times[k].append(timed(fn, reps))
    return times


def measure(pop, X, y, reps, rounds, Ks, descriptor, timed):
    f, pos, mate, libs = _setup(pop, X, Ks, descriptor)
    value, ntype, size = f._tensors()
    hip = torch.ops.evogp_hip
    calls = {"desired": lambda: hip.tree_SR_desired(value, ntype, size, X, y, pos),
             "desired_mid": lambda: hip.tree_SR_desired_mid(value, ntype, size, value, ntype, size, X, pos, mate)}
    for K in Ks:
        calls[f"match_k{K}"] = (lambda K=K: hip.tree_SR_backprop_match(value, ntype, size, X, y, pos, libs[K]))
        calls[f"agx_match_k{K}"] = (lambda K=K: hip.tree_SR_agx_match(value, ntype, size, value, ntype, size, X, pos, mate, libs[K]))
    times = _alternate(calls, timed, reps, rounds)
    best = {k: min(v) for k, v in times.items()}
    print(f"# {pop} trees: " + ", ".join(f"{k} {v:.2f} ms" for k, v in best.items()), file=sys.stderr, flush=True)
    out = hip.tree_SR_agx_match(value, ntype, size, value, ntype, size, X, pos, mate, libs[Ks[-1]])
    counts, status = out[4].double(), out[5]
    ratio = {"desired_mid": best["desired_mid"] / best["desired"]}
    ratio.update({f"agx_match_k{K}": best[f"agx_match_k{K}"] / best[f"match_k{K}"] for K in Ks})
    return {"pop": pop, "rows": X.shape[0], "var_len": 10, "gp_len": 64, "ms": best, "ms_all": times, "ratio_to_the_labelled_build": ratio,
            "status_share": [float((status == s).double().mean()) for s in range(5)],
            "row_share_required_free_impossible": (counts.sum(0) / counts.sum()).tolist(), "matched_share": float((out[0] >= 0).double().mean())}


def match_only(X, y, reps, rounds, descriptor, timed):
    """tree_SR_backprop_match at K = 256 on the configs[1] forest: the rounds of one build"""
    f, pos, _, libs = _setup(100_000, X, [256], descriptor)
    value, ntype, size = f._tensors()
    times = _alternate({"match_k256": lambda: torch.ops.evogp_hip.tree_SR_backprop_match(value, ntype, size, X, y, pos, libs[256])}, timed, reps, rounds)
    return {"match_k256_ms": times["match_k256"]}


def evolve(X, y, seed, generations, pop, geometric, descriptor):
    """the loss of the best tree after every generation"""
    from evogp_amd.algorithm import ApproxGeometricCrossover, DefaultCrossover, DefaultMutation, DefaultSelection, GeneticProgramming
    from evogp_amd.problem import SymbolicRegression
    from evogp_amd.tree import Forest

    dev = X.device
    torch.manual_seed(seed)
    d, sub = descriptor(5), descriptor(3)
    crossover = ApproxGeometricCrossover(X, descriptor=sub, library_size=1000, fallback=DefaultCrossover()) if geometric else DefaultCrossover()
    algo = GeneticProgramming(Forest.random_generate(pop, d, keys=torch.tensor([seed, 1], dtype=torch.uint32, device=dev)), crossover,
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
    print(f"# seed {seed}, {'geometric' if geometric else 'default'} crossover: best loss {curve[-1]:.6g} after {generations} generations",
          file=sys.stderr, flush=True)
    return {"best_loss": curve, "seconds": time.perf_counter() - t0, "library": int(crossover.library.pop_size) if geometric else None}


def _load(paths):
    return [json.load(open(p))["match_k256_ms"] for p in paths]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--generations", type=int, default=30)
    ap.add_argument("--evolve-pop", type=int, default=10_000)
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--root", default=ROOT, help="the checkout whose package is measured (--match-only: a build of the parent commit)")
    ap.add_argument("--match-only", action="store_true")
    ap.add_argument("--parent-runs", nargs="*", default=[], help="--match-only outputs of the parent commit")
    ap.add_argument("--branch-runs", nargs="*", default=[], help="--match-only outputs of this tree, taken alternately with them")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    descriptor, dataset, timed = _use(os.path.abspath(args.root))
    dev = torch.device("cuda:0")
    X, y = dataset(dev)
    if args.match_only:
        result = match_only(X, y, args.reps, args.rounds, descriptor, timed)
    else:
        parent, branch = _load(args.parent_runs), _load(args.branch_runs)
        comparison = None
        if parent and branch:
            flat = lambda runs: [t for r in runs for t in r]  # noqa: E731
            comparison = {"op": "tree_SR_backprop_match", "K": 256, "pop": 100_000, "parent_ms": min(flat(parent)), "branch_ms": min(flat(branch)),
                          "parent_ms_all": parent, "branch_ms_all": branch,
                          "spread_between_rounds_ms": {"parent": max(flat(parent)) - min(flat(parent)), "branch": max(flat(branch)) - min(flat(branch))}}
        result = {"device": torch.cuda.get_device_name(0),
                  "forests": [measure(pop, X, y, args.reps, args.rounds, [64, 256, 1024], descriptor, timed) for pop in (100_000, 1_000_000)],
                  "parent_commit_comparison": comparison,
                  "evolution": {"pop": args.evolve_pop, "generations": args.generations, "note": "an illustration, not a statistic",
                                "runs": [{"seed": s, "default_crossover": evolve(X, y, s, args.generations, args.evolve_pop, False, descriptor),
                                          "geometric_crossover": evolve(X, y, s, args.generations, args.evolve_pop, True, descriptor)}
                                         for s in args.seeds]}}
    line = json.dumps(result)
    print(line)
    out = args.out or (None if args.match_only else os.path.join(ROOT, "profiles", "agx_bench.json"))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
