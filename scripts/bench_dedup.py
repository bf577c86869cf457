"""Cost and yield of structural duplicate detection (csrc/dedup.hip; Forest.duplicate_classes, dedup=True, regenerate_duplicates).
Device events around every call after a warm-up call, medians over --reps; writes one JSON object to --out
(profiles/dedup_bench.json) and prints it.  No time or ratio is fixed in advance; the cost model to check against is "detection costs
well under one gradient launch, and the saving of a dedup=True call then approaches the duplicate share".

  (a) detect     tree_hash, tree_classes (sort + runs + comparisons) and both, next to tree_SR_fitness and one tree_SR_gradient launch on
                 the same forest: configs[1] (100 k trees x 1024 rows, 10 variables, gp_len 64, + - * /) and the 1 M headline forest
  (b) shares     share of rows that duplicate an earlier row, per generation over --generations generations:
                   configs1          DefaultSelection(0.3, elite_rate=0.01), DefaultCrossover, DefaultMutation(0.2, depth-3 donors)
                   configs1_simplify the same with SymbolicRegression(simplify_every=5)
                   uci_sr            the reference's example/uci_sr.py shape (gp_len 512, + - * / sin cos tan, TournamentSelection(20, 0.5, 0.1))
                 each with and without regenerate_duplicates (the share is taken on the forest the generation scores)
  (c) tuning     optimize_constants(method="lm", steps=3) and the 10-step descent with dedup on and off, on the generation-0, -5 and
                 -last forests of (b) configs1
"""
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
    """median over reps of the device time of one call, after one warm-up call"""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        fn()
        ev[1].record()
        ev[1].synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
    return float(np.median(ms))


def detect(forest, X, y, reps):
    v, t, s = forest._tensors()
    pop, L = v.shape
    ops = torch.ops.evogp_hip
    h = ops.tree_hash(v, t, s)
    out = {"pop": pop, "gp_len": L, "duplicate_share": 1.0 - float(forest.duplicate_classes()[1].float().mean())}
    out["tree_hash_ms"] = timed(lambda: ops.tree_hash(v, t, s), reps)
    out["tree_classes_ms"] = timed(lambda: ops.tree_classes(v, t, s, h), reps)
    out["duplicate_classes_ms"] = timed(forest.duplicate_classes, reps)
    out["sr_fitness_ms"] = timed(lambda: forest.SR_fitness(X, y), reps)
    out["sr_gradient_ms"] = timed(lambda: forest.SR_gradient(X, y), reps)
    out["detect_over_fitness"] = out["duplicate_classes_ms"] / out["sr_fitness_ms"]
    out["detect_over_gradient"] = out["duplicate_classes_ms"] / out["sr_gradient_ms"]
    return out


def shares(make_algo, problem, generations, score, keep=()):
    """duplicate share of the forest every generation scores (no host sync inside the loop), and the forests of the generations in keep"""
    algo = make_algo()
    firsts, kept = [], {}
    for g in range(generations + 1):
        if problem is not None:
            algo.forest = problem.optimize(algo.forest)
        if g in keep:
            kept[g] = algo.forest
        firsts.append(algo.forest.duplicate_classes()[1].sum())
        if g < generations:
            algo.step(score(algo.forest))
    pop = algo.forest.pop_size
    return [1.0 - int(f) / pop for f in firsts], kept


def tuning(forest, X, y, reps):
    out = {"duplicate_share": 1.0 - float(forest.duplicate_classes()[1].float().mean())}
    for name, kw in (("lm3", dict(steps=3, method="lm")), ("descent10", dict(steps=10))):
        off = timed(lambda: forest.optimize_constants(X, y, **kw), reps)
        on = timed(lambda: forest.optimize_constants(X, y, dedup=True, **kw), reps)
        out[name] = {"dedup_off_ms": off, "dedup_on_ms": on, "saving": 1.0 - on / off}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--generations", type=int, default=30)
    ap.add_argument("--pop", type=int, default=100_000)
    ap.add_argument("--headline-pop", type=int, default=1_000_000, help="0 skips the headline forest")
    ap.add_argument("--no-uci", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dedup_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_dedup.py measures on the GPU only"
    from evogp_amd.algorithm import DefaultCrossover, DefaultMutation, DefaultSelection, GeneticProgramming
    from evogp_amd.algorithm.selection import TournamentSelection
    from evogp_amd.problem import SymbolicRegression
    from evogp_amd.tree import Forest, GenerateDescriptor

    dev = torch.device("cuda:0")
    X, y = dataset(dev)
    score = lambda f: torch.ops.evogp_hip.fitness_scores(f.SR_fitness(X, y), True)   # noqa: E731
    G = args.generations
    keys = torch.tensor([42, 0], dtype=torch.uint32, device=dev)
    desc = GenerateDescriptor(max_tree_len=64, input_len=10, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=6,
                              const_samples=[-1, 0, 1])
    result = {"device": torch.cuda.get_device_name(0), "rows": 1024, "reps": args.reps, "generations": G}

    def configs1(regen):
        torch.manual_seed(0)
        return GeneticProgramming(Forest.random_generate(args.pop, desc, keys=keys), DefaultCrossover(),
                                  DefaultMutation(0.2, desc.update(max_layer_cnt=3)), DefaultSelection(0.3, elite_rate=0.01),
                                  regenerate_duplicates=desc if regen else None)

    # (b) and the forests of (c)
    keep = sorted({0, min(5, G), G})
    result["shares"] = {}
    plain, kept = shares(lambda: configs1(False), None, G, score, keep)
    result["shares"]["configs1"] = {"plain": plain, "regenerate_duplicates": shares(lambda: configs1(True), None, G, score)[0]}
    simplify = lambda: SymbolicRegression(datapoints=X, labels=y, simplify_every=5)   # noqa: E731
    result["shares"]["configs1_simplify_every_5"] = {"plain": shares(lambda: configs1(False), simplify(), G, score)[0],
                                                     "regenerate_duplicates": shares(lambda: configs1(True), simplify(), G, score)[0]}
    # (a)
    result["detect"] = {"configs1_generation_%d" % g: detect(f, X, y, args.reps) for g, f in kept.items()}
    # (c)
    result["tuning"] = {"generation_%d" % g: tuning(f, X, y, args.reps) for g, f in kept.items()}
    del kept
    if not args.no_uci:
        torch.manual_seed(42)
        udesc = GenerateDescriptor(max_tree_len=512, input_len=10, output_len=1, using_funcs=["+", "-", "*", "/", "sin", "cos", "tan"],
                                   max_layer_cnt=9, const_range=[-5, 5], sample_cnt=10000, layer_leaf_prob=0.3)

        def uci(regen):
            torch.manual_seed(42)
            return GeneticProgramming(Forest.random_generate(args.pop, udesc, keys=keys), DefaultCrossover(),
                                      DefaultMutation(0.1, udesc.update(max_layer_cnt=4)),
                                      TournamentSelection(tournament_size=20, survivor_rate=0.5, elite_rate=0.1),
                                      regenerate_duplicates=udesc if regen else None)

        result["shares"]["uci_sr"] = {"plain": shares(lambda: uci(False), None, G, score)[0], "regenerate_duplicates": shares(lambda: uci(True), None, G, score)[0]}
    if args.headline_pop:
        torch.cuda.empty_cache()
        big = Forest.random_generate(args.headline_pop, desc, keys=keys)
        result["detect"]["headline_generation_0"] = detect(big, X, y, max(1, args.reps // 2))
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
