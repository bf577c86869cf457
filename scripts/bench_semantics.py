"""Cost and yield of semantic duplicate classes (csrc/sr_semantic.hip; Forest.semantic_hash / semantic_classes).  Device events around
every call after a warm-up call, --reps repetitions each, all in ONE process; writes one JSON object to --out
(profiles/semantic_bench.json) and prints it.  No time is fixed in advance: the signature pass has tree_SR_linear_scaling's structure
with a lighter epilogue and is judged against that pass measured here, on the same forest -- "exceeds" means by more than the
scaling pass's own spread (max - min over its repetitions).

Forests: configs[1] (100 k trees x 1024 rows, 10 variables, gp_len 64, + - * /) fresh, the same run after --generations generations of
DefaultSelection(0.3, elite_rate=0.01) / DefaultCrossover / DefaultMutation(0.2, depth-3 donors), and the fresh 1 M headline forest.
Per forest:
  signature_ms          tree_SR_semantic_hash
  classes_ms            tree_SR_semantic_classes on those signatures; stages_1_3_ms is the same op given pairwise different hash words
                        (every position heads its run: pairs, sort, runs and an idle stage 4), stage_4_ms the difference of the medians
  linear_scaling_ms     tree_SR_linear_scaling, the yardstick; tree_hash_ms / tree_classes_ms the structural passes
  semantic_share        share of trees that are not the representative of their semantic class, next to structural_share
  word_compare_share    share of stage-4 comparisons settled by the word compare, without an evaluation: with no colliding signatures
                        every non-representative makes ONE comparison, with its class's first tree, and the word compare settles it
                        when the two are structural duplicates
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_dedup import dataset  # noqa: E402


def times(fn, reps):
    """{median, min, max} in ms of the device time of one call over reps calls, after one warm-up call"""
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
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}


def measure(forest, X, y, reps):
    v, t, s = forest._tensors()
    pop, L = v.shape
    ops = torch.ops.evogp_hip
    shape = (pop, X.shape[0], L, X.shape[1], 1)
    sig = ops.tree_SR_semantic_hash(*shape, v, t, s, X)
    sem = ops.tree_SR_semantic_classes(*shape, v, t, s, X, sig).to(torch.int64)
    h = ops.tree_hash(v, t, s)
    struct = ops.tree_classes(v, t, s, h).to(torch.int64)
    index = torch.arange(pop, device=v.device)
    follower = sem != index
    out = {"pop": pop, "gp_len": L, "rows": int(X.shape[0]),
           "semantic_share": float(follower.float().mean()), "structural_share": float((struct != index).float().mean()),
           "semantic_classes": int((~follower).sum()), "structural_classes": int((struct == index).sum()),
           "largest_semantic_class": int(torch.bincount(sem).max()),
           "distinct_signatures": int(torch.unique(sig[~follower]).numel())}
    out["word_compare_share"] = float((struct[follower] == struct[sem[follower]]).float().mean()) if bool(follower.any()) else None
    distinct = index   # pairwise different hash words: every run has one member
    out["signature_ms"] = times(lambda: ops.tree_SR_semantic_hash(*shape, v, t, s, X), reps)
    out["classes_ms"] = times(lambda: ops.tree_SR_semantic_classes(*shape, v, t, s, X, sig), reps)
    out["stages_1_3_ms"] = times(lambda: ops.tree_SR_semantic_classes(*shape, v, t, s, X, distinct), reps)
    out["stage_4_ms"] = out["classes_ms"]["median"] - out["stages_1_3_ms"]["median"]
    out["linear_scaling_ms"] = times(lambda: ops.tree_SR_linear_scaling(*shape, v, t, s, X, y), reps)
    out["tree_hash_ms"] = times(lambda: ops.tree_hash(v, t, s), reps)
    out["tree_classes_ms"] = times(lambda: ops.tree_classes(v, t, s, h), reps)
    spread = out["linear_scaling_ms"]["max"] - out["linear_scaling_ms"]["min"]
    excess = out["signature_ms"]["median"] - out["linear_scaling_ms"]["median"]
    out["signature_minus_scaling_ms"] = excess
    out["scaling_spread_ms"] = spread
    out["signature_exceeds_scaling"] = bool(excess > spread)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--generations", type=int, default=30)
    ap.add_argument("--pop", type=int, default=100_000)
    ap.add_argument("--headline-pop", type=int, default=1_000_000, help="0 skips the headline forest")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "semantic_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_semantics.py measures on the GPU only"
    from evogp_amd.algorithm import DefaultCrossover, DefaultMutation, DefaultSelection, GeneticProgramming
    from evogp_amd.tree import Forest, GenerateDescriptor

    dev = torch.device("cuda:0")
    X, y = dataset(dev)
    keys = torch.tensor([42, 0], dtype=torch.uint32, device=dev)
    desc = GenerateDescriptor(max_tree_len=64, input_len=10, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=6,
                              const_samples=[-1, 0, 1])
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "generations": args.generations, "forests": {}}

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
        result["forests"]["headline_generation_0"] = measure(big, X, y, max(1, args.reps // 2))
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
