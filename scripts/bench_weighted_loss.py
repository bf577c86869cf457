"""Cost of the weighted losses (csrc/sr_wloss.hip, Forest.SR_weighted_loss) next to what stands around them: tree_SR_linear_scaling
(the same interpreter skeleton with three float64 sums per row), SR_fitness on the same forest (the threaded-code path, untouched) and
the composition a user had before -- SR_case_errors plus float64 torch ``(E * w).sum(1) / w.sum()``, which writes and rereads the
(pop, D) errors.  One device-event pair around EVERY call after warm-up, the calls of all kinds alternating in the same process;
median, min, max and the spread (median - min) over --calls calls (>= 20).  Prints one JSON object and writes it to --out (default
profiles/weighted_loss_bench.json).

  configs1   100 k trees x 1024 rows, 10 variables, gp_len 64, + - * /           (BASELINE configs[1]); every call
  headline   1 M trees x 1024 rows, same descriptor                            (bench.py's headline forest); no composition there:
                                                                                 its errors alone are 4 GB

No time is fixed in advance.  What is reported:
  (a) "weighted_beats_composition": the K = 1 weighted mse call -- the one loss the composition can express -- lies below the
      composition by more than the spreads of the two ("huber_K1_beats_composition": the same of the Huber call);
  (b) "unweighted_within_linear_scaling": the unweighted mse call does not exceed tree_SR_linear_scaling by more than their spreads;
  (c) "second_column_over_full_call": (K = 2 minus K = 1) over K = 1 -- the price of a validation score against a second full call;
      "eight_columns_over_one" likewise for K = 8."""
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
    W = rng.uniform(0, 2, (8, 1024)).astype(np.float32)
    W[rng.random((8, 1024)) < 1 / 3] = 0
    return tuple(torch.from_numpy(a).to(device) for a in (X, y, W))


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
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "spread_ms": statistics.median(v) - min(v),
                "calls": len(v)} for k, v in times.items()}


def new_calls(f, X, y, W):
    return {"unweighted_mse": lambda: f.SR_weighted_loss(X, y),
            "huber_K1": lambda: f.SR_weighted_loss(X, y, W[0], "huber", 1.0),
            "huber_K2": lambda: f.SR_weighted_loss(X, y, W[:2], "huber", 1.0),
            "huber_K8": lambda: f.SR_weighted_loss(X, y, W, "huber", 1.0),
            "linear_scaling": lambda: f.SR_scaled_fitness(X, y),
            "sr_fitness": lambda: f.SR_fitness(X, y)}


def ratios(r):
    k1, k2, k8 = (r[k]["median_ms"] for k in ("huber_K1", "huber_K2", "huber_K8"))
    r["second_column_over_full_call"] = (k2 - k1) / k1
    r["eight_columns_over_one"] = (k8 - k1) / k1
    r["unweighted_over_linear_scaling"] = r["unweighted_mse"]["median_ms"] / r["linear_scaling"]["median_ms"]
    r["unweighted_over_sr_fitness"] = r["unweighted_mse"]["median_ms"] / r["sr_fitness"]["median_ms"]
    r["unweighted_within_linear_scaling"] = (r["unweighted_mse"]["median_ms"] <= r["linear_scaling"]["median_ms"]
                                             + r["unweighted_mse"]["spread_ms"] + r["linear_scaling"]["spread_ms"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-headline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weighted_loss_bench.json"))
    args = ap.parse_args()
    assert args.calls >= 20, "median and spread over at least 20 calls"
    from evogp_amd.tree import Forest, GenerateDescriptor

    dev = torch.device("cuda:0")
    X, y, W = dataset(dev)
    desc = GenerateDescriptor(max_tree_len=64, input_len=10, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=6,
                              const_samples=[-1, 0, 1])
    keys = torch.tensor([42, 0], dtype=torch.uint32, device=dev)
    result = {"device": torch.cuda.get_device_name(0), "rows": 1024, "var_len": 10, "gp_len": 64, "timing": "one event pair per call",
              "spread": "median - min"}

    def composition(f, w):   # what a user had before: the (pop, D) squared errors, then float64 torch
        E = f.SR_case_errors(X, y, True)
        return (E.to(torch.float64) * w.to(torch.float64)[None, :]).sum(1) / w.to(torch.float64).sum()

    f = Forest.random_generate(100_000, desc, keys=keys)
    calls = new_calls(f, X, y, W)
    calls["mse_K1"] = lambda: f.SR_weighted_loss(X, y, W[0])
    calls["case_errors_plus_torch_float64"] = lambda: composition(f, W[0])
    r = measure(calls, args.calls, args.warmup)
    r["pop"] = f.pop_size
    ratios(r)
    comp, new = r["case_errors_plus_torch_float64"], r["mse_K1"]
    r["composition_over_weighted"] = comp["median_ms"] / new["median_ms"]
    r["weighted_beats_composition"] = new["median_ms"] < comp["median_ms"] - comp["spread_ms"] - new["spread_ms"]
    r["huber_K1_beats_composition"] = r["huber_K1"]["median_ms"] < comp["median_ms"] - comp["spread_ms"] - r["huber_K1"]["spread_ms"]
    got, want = f.SR_weighted_loss(X, y, W[0]), composition(f, W[0]).to(torch.float32)
    fin = torch.isfinite(got) & torch.isfinite(want)
    r["nan_trees"] = int(torch.isnan(got).sum())
    r["nan_trees_composition"] = int(torch.isnan(want).sum())   # (0 * NaN: a tree undefined on a row without weight is lost here)
    r["max_rel_diff_to_composition"] = float(((got[fin] - want[fin]).abs() / want[fin].abs().clamp(min=1e-30)).max())
    plain = f.SR_fitness(X, y)
    both = torch.isfinite(plain) & torch.isfinite(f.SR_weighted_loss(X, y))
    r["max_rel_diff_unweighted_to_sr_fitness"] = float(((f.SR_weighted_loss(X, y)[both] - plain[both]).abs() / plain[both].abs().clamp(min=1e-30)).max())
    result["configs1"] = r
    print("configs1", json.dumps(r), flush=True)
    del f, calls
    torch.cuda.empty_cache()

    if not args.no_headline:
        f = Forest.random_generate(1_000_000, desc, keys=keys)
        r = measure(new_calls(f, X, y, W), args.calls, args.warmup)
        r["pop"] = f.pop_size
        ratios(r)
        result["headline"] = r
        print("headline", json.dumps(r), flush=True)
        del f
        torch.cuda.empty_cache()

    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
