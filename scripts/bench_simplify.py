"""Cost and effect of tree simplification (csrc/sr_subtree.hip, Forest.simplify): the two launches (tree_SR_subtree_errors, tree_prune)
next to tree_SR_gradient and tree_SR_fitness on the same forest in the same process, alternating; the mean tree size before and after
one ``simplify``; and what ``SymbolicRegression(simplify_every=1)`` does to a run.  Device events around each call after warm-up;
prints one JSON object and writes it to --out (default profiles/simplify_bench.json).

  configs1   100 k trees x 1024 rows, 10 variables, gp_len 64, + - * /           (BASELINE configs[1])
  headline   1 M trees x 1024 rows, same descriptor                            (bench.py's headline forest; --headline)
  evolved    6 000 trees of gp_len 512 over + - * / sin cos tan after 30 generations of example/uci_sr.py's operators
  runs       those 30 generations with simplify_every = 0 and = 1 from the same seed: mean tree size, best fitness, time per generation

The yardstick: the subtree pass is the gradient kernel's forward walk without its reverse walk, so ``subtree_errors_ms`` should not
exceed ``gradient_ms`` on the same forest ("subtree_over_gradient" <= 1)."""
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
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def measure(f, X, y, reps, rounds):
    value, ntype, size = f._tensors()
    node_err, node_const = f.SR_subtree_errors(X, y)
    calls = {
        "fitness_ms": lambda: f.SR_fitness(X, y),
        "gradient_ms": lambda: f.SR_gradient(X, y),
        "subtree_errors_ms": lambda: f.SR_subtree_errors(X, y),
        "prune_ms": lambda: torch.ops.evogp_hip.tree_prune(1, True, True, value, ntype, size, node_err, node_const),
        "simplify_ms": lambda: f.simplify(X, y),
    }
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(rounds):                      # alternating, same process
        for k, fn in calls.items():
            times[k].append(timed(fn, reps))
    out = {k: min(v) for k, v in times.items()}
    out.update({k + "_all": v for k, v in times.items()})
    g, loss = f.simplify(X, y)
    own = node_err[:, 0]
    fin = torch.isfinite(own)
    nodes = int(size[:, 0].clamp(min=0).sum())
    out.update(pop=f.pop_size, gp_len=f.max_tree_len, live_nodes=nodes, subtree_over_gradient=out["subtree_errors_ms"] / out["gradient_ms"],
               subtree_node_rows_per_s=nodes * X.shape[0] / (out["subtree_errors_ms"] * 1e-3),
               mean_tree_size_before=float(size[:, 0].float().mean()), mean_tree_size_after=float(g.batch_subtree_size[:, 0].float().mean()),
               max_tree_size_before=int(size[:, 0].max()), max_tree_size_after=int(g.batch_subtree_size[:, 0].max()),
               trees_smaller=float((g.batch_subtree_size[:, 0] < size[:, 0]).float().mean()),
               trees_better=float((loss[fin] < own[fin]).float().mean()), trees_rescued=int((~fin & torch.isfinite(loss)).sum()),
               nan_trees_before=int((~fin).sum()))
    return out


def uci_run(X, y, generations, simplify_every, pop=6000):
    """example/uci_sr.py's shape: + - * / sin cos tan, max_tree_len 512, DefaultCrossover, DefaultMutation(0.1, max_layer_cnt 4),
    TournamentSelection(20, 0.5, 0.1), through StandardPipeline.step"""
    from evogp_amd.algorithm import DefaultCrossover, DefaultMutation, GeneticProgramming
    from evogp_amd.algorithm.selection import TournamentSelection
    from evogp_amd.pipeline import StandardPipeline
    from evogp_amd.problem import SymbolicRegression
    from evogp_amd.tree import Forest, GenerateDescriptor

    torch.manual_seed(11)
    desc = GenerateDescriptor(max_tree_len=512, input_len=10, output_len=1, using_funcs=["+", "-", "*", "/", "sin", "cos", "tan"],
                              max_layer_cnt=9, const_range=[-5, 5], sample_cnt=10000, layer_leaf_prob=0.3)
    algo = GeneticProgramming(Forest.random_generate(pop, desc, keys=torch.tensor([42, 0], dtype=torch.uint32, device=X.device)),
                              DefaultCrossover(), DefaultMutation(0.1, desc.update(max_layer_cnt=4)), TournamentSelection(20, 0.5, 0.1))
    pipe = StandardPipeline(algo, SymbolicRegression(datapoints=X, labels=y, simplify_every=simplify_every), is_show_details=False)
    pipe.step()   # (warm-up of every kernel; part of the run)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(generations - 1):
        pipe.step()
    ev[1].record()
    ev[1].synchronize()
    size = algo.forest.batch_subtree_size[:, 0]
    return algo.forest, {"simplify_every": simplify_every, "generations": generations, "pop": pop,
                         "generation_ms": ev[0].elapsed_time(ev[1]) / max(generations - 1, 1), "mean_tree_size": float(size.float().mean()),
                         "max_tree_size": int(size.max()), "best_fitness": float(pipe.best_fitness)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--generations", type=int, default=30)
    ap.add_argument("--headline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simplify_bench.json"))
    args = ap.parse_args()
    from evogp_amd.tree import Forest, GenerateDescriptor

    dev = torch.device("cuda:0")
    X, y = dataset(dev)
    desc = GenerateDescriptor(max_tree_len=64, input_len=10, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=6,
                              const_samples=[-1, 0, 1])
    keys = torch.tensor([42, 0], dtype=torch.uint32, device=dev)
    result = {"device": torch.cuda.get_device_name(0), "rows": 1024, "var_len": 10,
              "yardstick": "subtree_errors_ms <= gradient_ms on the same forest in the same process"}
    f = Forest.random_generate(100_000, desc, keys=keys)
    result["configs1"] = measure(f, X, y, args.reps, args.rounds)
    print("configs1", json.dumps(result["configs1"]), flush=True)
    del f
    torch.cuda.empty_cache()
    if args.headline:
        f = Forest.random_generate(1_000_000, desc, keys=keys)
        result["headline"] = measure(f, X, y, max(1, args.reps // 2), max(1, args.rounds - 1))
        print("headline", json.dumps(result["headline"]), flush=True)
        del f
        torch.cuda.empty_cache()
    evolved, result["run_simplify_every_0"] = uci_run(X, y, args.generations, 0)
    print("run0", json.dumps(result["run_simplify_every_0"]), flush=True)
    result["evolved"] = measure(evolved, X, y, args.reps, args.rounds)
    print("evolved", json.dumps(result["evolved"]), flush=True)
    del evolved
    _, result["run_simplify_every_1"] = uci_run(X, y, args.generations, 1)
    print("run1", json.dumps(result["run_simplify_every_1"]), flush=True)
    result["yardstick_met"] = all(result[k]["subtree_over_gradient"] <= 1.0 for k in ("configs1", "headline", "evolved") if k in result)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
