"""The weighted tuning passes next to the unweighted ones on the configs[1] forest (100 k trees x 1024 rows, 10 variables, gp_len 64,
+ - * /, the forest of scripts/bench_sr_lm.py), in one process, alternating after warm-up:

  * tree_SR_gradient against tree_SR_weighted_gradient with no weights (MSE), one weight row, 20 % of the rows held out at random, 20 %
    held out as one contiguous block, and no weights under Huber and log-cosh;
  * tree_SR_normal_eq against tree_SR_weighted_normal_eq with no weights and with the contiguous mask;
  * 10 descent steps of Forest.optimize_constants, unweighted and under the contiguous mask with Huber.

Device events around each call; every new time is also given as a ratio to the unweighted op of the same kind in the same process.
Prints one JSON object and writes it to --out (default profiles/weighted_tuning_bench.json)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.bench_sr_grad import dataset, timed  # noqa: E402

MSE, HUBER, LOGCOSH = 0, 2, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pop", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weighted_tuning_bench.json"))
    args = ap.parse_args()
    from evogp_amd.tree import Forest, GenerateDescriptor

    dev = torch.device("cuda:0")
    X, y = dataset(dev)
    D = X.shape[0]
    desc = GenerateDescriptor(max_tree_len=64, input_len=10, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=6,
                              const_samples=[-1, 0, 1])
    f = Forest.random_generate(args.pop, desc, keys=torch.tensor([42, 0], dtype=torch.uint32, device=dev))
    value, ntype, size = f._tensors()
    shape = (args.pop, D, 64, 10, 1)
    rng = np.random.default_rng(20261020)
    w_row = torch.from_numpy(rng.uniform(0.5, 2, D).astype(np.float32)).to(dev)
    w_rand = torch.from_numpy((rng.random(D) >= 0.2).astype(np.float32)).to(dev)
    w_block = torch.ones(D, device=dev)
    w_block[D - D // 5:] = 0   # the last 20 % of the rows: 3 whole 64-row tiles and part of a fourth
    hip = torch.ops.evogp_hip
    wgrad = lambda w, kind, prm: (lambda: hip.tree_SR_weighted_gradient(*shape, value, ntype, size, X, y, w, kind, prm))   # noqa: E731
    wneq = lambda w: (lambda: hip.tree_SR_weighted_normal_eq(*shape, value, ntype, size, X, y, w))                         # noqa: E731
    calls = {
        "gradient": lambda: hip.tree_SR_gradient(*shape, True, value, ntype, size, X, y),
        "wgradient_no_weights_mse": wgrad(None, MSE, 0.0),
        "wgradient_weight_row_mse": wgrad(w_row, MSE, 0.0),
        "wgradient_random_mask_mse": wgrad(w_rand, MSE, 0.0),
        "wgradient_block_mask_mse": wgrad(w_block, MSE, 0.0),
        "wgradient_no_weights_huber": wgrad(None, HUBER, 1.0),
        "wgradient_no_weights_logcosh": wgrad(None, LOGCOSH, 0.0),
        "normal_eq": lambda: hip.tree_SR_normal_eq(*shape, value, ntype, size, X, y),
        "wnormal_eq_no_weights": wneq(None),
        "wnormal_eq_block_mask": wneq(w_block),
        "descent_10_steps": lambda: f.optimize_constants(X, y, steps=10),
        "descent_10_steps_block_mask_huber": lambda: f.optimize_constants(X, y, steps=10, weights=w_block, loss="huber", param=1.0),
    }
    for fn in calls.values():   # warm-up
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(args.rounds):   # alternating, same process
        for k, fn in calls.items():
            times[k].append(timed(fn, 1 if k.startswith("descent") else args.reps))
    best = {k: min(v) for k, v in times.items()}
    base = lambda k: "gradient" if "gradient" in k else "normal_eq" if "normal_eq" in k else "descent_10_steps"   # noqa: E731
    result = {"device": torch.cuda.get_device_name(0), "pop": args.pop, "rows": D, "var_len": 10, "gp_len": 64,
              "held_out_rows_random": int((w_rand == 0).sum()), "held_out_rows_block": int((w_block == 0).sum()),
              "ms": best, "ms_all": times,
              "ratio_to_unweighted": {k: best[k] / best[base(k)] for k in calls if k != base(k)}}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
