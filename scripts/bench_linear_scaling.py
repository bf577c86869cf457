"""Cost of linear scaling (csrc/sr_scale.hip, Forest.SR_scaled_fitness) next to the two things it stands between: SR_fitness on the same
forest (the floor: the threaded-code path, untouched) and the composition a user had before -- batch_forward plus float64 torch
reductions (SymbolicRegression(linear_scaling=True, execute_mode="torch")), which writes and rereads the (pop, D) predictions.
One device-event pair around EVERY call after warm-up, the calls of the three kinds alternating in the same process; median, min and
max over --calls calls (>= 20).  Prints one JSON object and writes it to --out (default profiles/linear_scaling_bench.json).

  configs1   100 k trees x 1024 rows, 10 variables, gp_len 64, + - * /           (BASELINE configs[1]); all three
  headline   1 M trees x 1024 rows, same descriptor                            (bench.py's headline forest); no composition there:
                                                                                 its predictions alone are 4 GB

Ready when, at configs1, the median of the new call lies below the composition's median by more than the composition's own
min-to-median spread ("ready").  The ratio to SR_fitness is reported, not gated."""
import argparse
import json
import os
import statistics
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


def measure(calls, n_calls, warmup):
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(n_calls):                      # alternating, same process
        for k, fn in calls.items():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            fn()
            ev[1].record()
            ev[1].synchronize()
            times[k].append(ev[0].elapsed_time(ev[1]))
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "calls": len(v)} for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-headline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_scaling_bench.json"))
    args = ap.parse_args()
    assert args.calls >= 20, "median and min over at least 20 calls"
    from evogp_amd.problem import SymbolicRegression
    from evogp_amd.tree import Forest, GenerateDescriptor

    dev = torch.device("cuda:0")
    X, y = dataset(dev)
    desc = GenerateDescriptor(max_tree_len=64, input_len=10, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=6,
                              const_samples=[-1, 0, 1])
    keys = torch.tensor([42, 0], dtype=torch.uint32, device=dev)
    composed = SymbolicRegression(datapoints=X, labels=y, linear_scaling=True, execute_mode="torch")
    result = {"device": torch.cuda.get_device_name(0), "rows": 1024, "var_len": 10, "gp_len": 64, "timing": "one event pair per call"}

    f = Forest.random_generate(100_000, desc, keys=keys)
    r = measure({"scaled_fitness": lambda: f.SR_scaled_fitness(X, y), "sr_fitness": lambda: f.SR_fitness(X, y),
                 "batch_forward_plus_torch_float64": lambda: composed.scaled_fitness(f)}, args.calls, args.warmup)
    comp, new = r["batch_forward_plus_torch_float64"], r["scaled_fitness"]
    r["pop"] = f.pop_size
    r["scaled_over_sr_fitness"] = new["median_ms"] / r["sr_fitness"]["median_ms"]
    r["composition_over_scaled"] = comp["median_ms"] / new["median_ms"]
    r["composition_spread_ms"] = comp["median_ms"] - comp["min_ms"]
    r["ready"] = new["median_ms"] < comp["median_ms"] - r["composition_spread_ms"]
    loss, slope, intercept = f.SR_scaled_fitness(X, y)
    tl, _, _ = composed.scaled_fitness(f)
    fin = torch.isfinite(loss) & torch.isfinite(tl)
    r["nan_trees"] = int(torch.isnan(loss).sum())
    r["nan_masks_equal"] = bool(torch.equal(torch.isnan(loss), torch.isnan(tl)))
    r["max_rel_diff_to_composition"] = float(((loss[fin] - tl[fin]).abs() / tl[fin].abs().clamp(min=1e-30)).max())
    plain = f.SR_fitness(X, y)
    both = fin & torch.isfinite(plain)
    r["median_loss_plain"] = float(plain[both].double().median())
    r["median_loss_scaled"] = float(loss[both].double().median())
    result["configs1"] = r
    print("configs1", json.dumps(r), flush=True)
    del f
    torch.cuda.empty_cache()

    if not args.no_headline:
        f = Forest.random_generate(1_000_000, desc, keys=keys)
        r = measure({"scaled_fitness": lambda: f.SR_scaled_fitness(X, y), "sr_fitness": lambda: f.SR_fitness(X, y)}, args.calls, args.warmup)
        r["pop"] = f.pop_size
        r["scaled_over_sr_fitness"] = r["scaled_fitness"]["median_ms"] / r["sr_fitness"]["median_ms"]
        result["headline"] = r
        print("headline", json.dumps(r), flush=True)
        del f
        torch.cuda.empty_cache()

    result["ready"] = result["configs1"]["ready"]
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
