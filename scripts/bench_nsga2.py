"""Cost of NSGA-II selection (csrc/nsga2.hip, NSGA2Selection), stage by stage: the key order, the bucket order, the fronts (the
one-workgroup chain over the complexity buckets), the crowding distances, the final order (evogp_hip_debug_pareto_rank stops the call
after a stage; the differences of the timed calls are the stages), the tournaments and the whole ``__call__``.  Next to each, on the
same forest: tree_SR_fitness, TournamentSelection.counter_based, the mean tree size, the number of fronts and K, the number of
distinct complexity values.  Device events around each call after warm-up; prints one JSON object (and writes it to --out).

  fresh      100 k trees x 1024 rows, 10 variables, gp_len 64, + - * / (BASELINE configs[1]), Forest.random_generate
  evolved    the same forest after 30 generations under NSGA2Selection(elite_rate=0.5, mating_pool="elites")
  zero       Forest.zero_generate: one point
  long512    100 k fresh trees of gp_len 512
  headline   1 M trees x 1024 rows, fresh (--headline)

and, as a statement of what happened: mean tree size and best fitness after the same number of generations under
TournamentSelection(2) from the same start."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def dataset(device):
    rng = np.random.default_rng(1234)
    X = rng.uniform(-5, 5, (1024, 10)).astype(np.float32)
    y = (X[:, 0] * X[:, 1] + X[:, 2] * X[:, 3] - X[:, 4] + 0.5 * X[:, 5] ** 2).astype(np.float32)[:, None]
    return torch.from_numpy(X).to(device), torch.from_numpy(y).to(device)


def timed(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    fn()
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def measure(forest, X, y, reps):
    from evogp_amd import _lib
    from evogp_amd.algorithm import NSGA2Selection, TournamentSelection

    L = _lib.lib
    pop = forest.pop_size
    sel = NSGA2Selection(elite_rate=0.5, mating_pool="elites")
    fit = -forest.SR_fitness(X, y)
    err, cx, bound = sel.objectives(forest, fit)
    rank = lambda: torch.ops.evogp_hip.pareto_rank(err, cx, bound)   # noqa: E731
    t = []
    for stop in (1, 2, 3, 4, 0):
        assert L.evogp_hip_debug_pareto_rank(stop) == 0
        t.append(timed(rank, reps))
    out = {"key_order_ms": t[0], "bucket_order_ms": t[1] - t[0], "fronts_ms": t[2] - t[1], "crowding_ms": t[3] - t[2], "order_ms": t[4] - t[3],
           "pareto_rank_ms": t[4]}
    front, crowding, order = rank()
    out["tournaments_ms"] = timed(lambda: torch.ops.evogp_hip.nsga2_select(order, pop // 2, pop, 2, sel.seed, 0), reps)
    out["operator_ms"] = timed(lambda: sel(forest, fit), reps)
    ranked = front != 0x7FFFFFFF
    out.update(ranked=int(ranked.sum()), fronts=int(front[ranked].max()) + 1 if bool(ranked.any()) else 0, K=int(torch.unique(cx[ranked]).numel()),
               points=int((crowding > 0).sum()), pareto_set=int(((front == 0) & (crowding > 0)).sum()),
               mean_tree_size=float(forest.batch_subtree_size[:, 0].float().mean()), gp_len=forest.max_tree_len)
    # context on the same forest
    out["sr_fitness_ms"] = timed(lambda: forest.SR_fitness(X, y), reps)
    tour = TournamentSelection(2, survivor_rate=1.0, elite_rate=0.01)
    clean = torch.nan_to_num(fit, nan=float("-inf"))
    out["tournament_counter_based_ms"] = timed(lambda: tour.counter_based(clean, 1, 0), reps)
    return out


def evolve(forest, desc, selection, X, y, generations, clean):
    from evogp_amd.algorithm import DefaultCrossover, DefaultMutation, GeneticProgramming

    torch.manual_seed(0)
    algo = GeneticProgramming(forest, DefaultCrossover(), DefaultMutation(0.2, desc), selection)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(generations):
        fit = -algo.forest.SR_fitness(X, y)
        algo.step(torch.nan_to_num(fit, nan=float("-inf")) if clean else fit)
    ev[1].record()
    ev[1].synchronize()
    fit = torch.nan_to_num(-algo.forest.SR_fitness(X, y), nan=float("-inf"))
    return algo.forest, {"generation_ms": ev[0].elapsed_time(ev[1]) / max(generations, 1), "generations": generations,
                         "mean_tree_size": float(algo.forest.batch_subtree_size[:, 0].float().mean()), "best_fitness": float(fit.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--generations", type=int, default=30)
    ap.add_argument("--headline", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from evogp_amd.algorithm import NSGA2Selection, TournamentSelection
    from evogp_amd.tree import Forest, GenerateDescriptor

    dev = torch.device("cuda:0")
    X, y = dataset(dev)
    desc = GenerateDescriptor(max_tree_len=64, input_len=10, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=6,
                              const_samples=[-1, 0, 1])
    keys = torch.tensor([42, 0], dtype=torch.uint32, device=dev)
    result = {"device": torch.cuda.get_device_name(0), "pop": 100_000, "rows": 1024, "selection": "NSGA2Selection(elite_rate=0.5, mating_pool='elites')"}
    fresh = Forest.random_generate(100_000, desc, keys=keys)
    result["fresh"] = measure(fresh, X, y, args.reps)
    result["zero"] = measure(Forest.zero_generate(100_000, 64, 10, 1), X, y, args.reps)
    evolved, result["run_nsga2"] = evolve(fresh, desc, NSGA2Selection(elite_rate=0.5, mating_pool="elites"), X, y, args.generations, clean=False)
    result["evolved"] = measure(evolved, X, y, args.reps)
    result["evolved"]["selection_share_of_generation"] = result["evolved"]["operator_ms"] / result["run_nsga2"]["generation_ms"]
    _, result["run_tournament2"] = evolve(fresh, desc, TournamentSelection(2, survivor_rate=1.0, elite_rate=0.01), X, y, args.generations, clean=True)
    del evolved
    desc512 = GenerateDescriptor(max_tree_len=512, input_len=10, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=9,
                                 const_samples=[-1, 0, 1])
    result["long512"] = measure(Forest.random_generate(100_000, desc512, keys=keys), X, y, args.reps)
    if args.headline:
        del fresh
        torch.cuda.empty_cache()
        result["headline"] = measure(Forest.random_generate(1_000_000, desc, keys=keys), X, y, max(1, args.reps // 2))
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
