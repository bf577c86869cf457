"""Cost of weighted linear scaling (csrc/sr_wscale.hip, Forest.SR_weighted_scaled_fitness) next to what stands around it:
tree_SR_linear_scaling (the same interpreter skeleton, unweighted, fitted on every row), the two separate passes a user could make
before -- tree_SR_linear_scaling plus tree_SR_weighted_loss with two weight rows: two interpretations of the trees, and still no
held-out score of the SCALED model -- and the composition that does give it: batch_forward plus the float64 torch twin of the problem's
torch mode, which writes and rereads the (pop, D) predictions.  One device-event pair around EVERY call after warm-up, the calls of all
kinds alternating in the same process; median, min, max and the spread (median - min) over --calls calls (>= 20).  Prints one JSON object
and writes it to --out (default profiles/weighted_scaling_bench.json).

  configs1   100 k trees x 1024 rows, 10 variables, gp_len 64, + - * /           (BASELINE configs[1]); every call
  headline   1 M trees x 1024 rows, same descriptor                            (bench.py's headline forest); no composition there:
                                                                                 its float64 intermediates alone are tens of GB

No time is fixed in advance.  What is reported:
  (a) "two_rows_below_two_passes": the K = 2 call (a training and a validation row) lies below tree_SR_linear_scaling plus the K = 2
      tree_SR_weighted_loss by more than the spreads of the three; "two_rows_over_two_passes" is the ratio;
  (b) "unweighted_over_linear_scaling": the call without weights over tree_SR_linear_scaling;
  (c) "second_row_over_one", "eight_rows_over_one": (K = 2 minus K = 1) over K = 1 and (K = 8 minus K = 1) over K = 1;
  (d) "composition_over_two_rows": batch_forward plus float64 torch over the K = 2 call (configs1 only)."""
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
    W = rng.uniform(0.5, 2, (8, 1024)).astype(np.float32)
    W[rng.random((8, 1024)) < 0.3] = 0
    m = rng.random(1024) < 0.3   # rows 0 and 1: a training row and its complement, as SymbolicRegression builds them
    W[1] = np.where(m, np.float32(1), np.float32(0))
    W[0] = np.where(m, np.float32(0), W[0] + np.float32(0.5))
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


def two_passes(f, X, y, W2):
    f.SR_scaled_fitness(X, y)
    return f.SR_weighted_loss(X, y, W2)


def new_calls(f, X, y, W):
    return {"scaling_none": lambda: f.SR_weighted_scaled_fitness(X, y),
            "scaling_K1": lambda: f.SR_weighted_scaled_fitness(X, y, W[0]),
            "scaling_K2": lambda: f.SR_weighted_scaled_fitness(X, y, W[:2]),
            "scaling_K8": lambda: f.SR_weighted_scaled_fitness(X, y, W),
            "linear_scaling": lambda: f.SR_scaled_fitness(X, y),
            "weighted_loss_K2": lambda: f.SR_weighted_loss(X, y, W[:2]),
            "linear_scaling_plus_weighted_loss_K2": lambda: two_passes(f, X, y, W[:2])}


def ratios(r):
    k0, k1, k2, k8 = (r[k]["median_ms"] for k in ("scaling_none", "scaling_K1", "scaling_K2", "scaling_K8"))
    both = r["linear_scaling_plus_weighted_loss_K2"]
    r["second_row_over_one"] = (k2 - k1) / k1
    r["eight_rows_over_one"] = (k8 - k1) / k1
    r["unweighted_over_linear_scaling"] = k0 / r["linear_scaling"]["median_ms"]
    r["two_rows_over_two_passes"] = k2 / both["median_ms"]
    r["two_rows_below_two_passes"] = k2 < both["median_ms"] - both["spread_ms"] - r["scaling_K2"]["spread_ms"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-headline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weighted_scaling_bench.json"))
    args = ap.parse_args()
    assert args.calls >= 20, "median and spread over at least 20 calls"
    from evogp_amd.problem import SymbolicRegression
    from evogp_amd.tree import Forest, GenerateDescriptor

    dev = torch.device("cuda:0")
    X, y, W = dataset(dev)
    desc = GenerateDescriptor(max_tree_len=64, input_len=10, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=6,
                              const_samples=[-1, 0, 1])
    keys = torch.tensor([42, 0], dtype=torch.uint32, device=dev)
    result = {"device": torch.cuda.get_device_name(0), "rows": 1024, "var_len": 10, "gp_len": 64, "timing": "one event pair per call",
              "spread": "median - min"}
    # the composition: the problem's own torch mode (batch_forward, then the definition in float64 torch) on the same two rows
    twin = SymbolicRegression(datapoints=X, labels=y, linear_scaling=True, scaling_loss="problem", sample_weights=W[0] + W[1],
                              validation_mask=W[1] != 0, execute_mode="torch")
    assert torch.equal(twin._loss_weights, W[:2])

    f = Forest.random_generate(100_000, desc, keys=keys)
    calls = new_calls(f, X, y, W)
    calls["batch_forward_plus_torch_float64"] = lambda: twin.scaled_fitness(f)
    r = measure(calls, args.calls, args.warmup)
    r["pop"] = f.pop_size
    ratios(r)
    r["composition_over_two_rows"] = r["batch_forward_plus_torch_float64"]["median_ms"] / r["scaling_K2"]["median_ms"]
    loss, slope, icpt = f.SR_weighted_scaled_fitness(X, y, W[:2])
    tl, ts, ti = twin.scaled_fitness(f)
    tl = torch.stack([tl, twin.last_validation_loss], dim=1)
    fin = torch.isfinite(loss) & torch.isfinite(tl)
    r["nan_trees"] = int(torch.isnan(slope).sum())
    r["nan_trees_composition"] = int(torch.isnan(ts).sum())
    r["max_rel_diff_to_composition"] = float(((loss[fin] - tl[fin]).abs() / tl[fin].abs().clamp(min=1e-30)).max())
    plain = f.SR_scaled_fitness(X, y)[0]
    none = f.SR_weighted_scaled_fitness(X, y)[0]
    both = torch.isfinite(plain) & torch.isfinite(none)
    r["max_rel_diff_unweighted_to_linear_scaling"] = float(((none[both] - plain[both]).abs() / plain[both].abs().clamp(min=1e-30)).max())
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
