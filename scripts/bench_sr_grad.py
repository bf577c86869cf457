"""Cost of the constant-gradient pass (tree_SR_gradient) next to the fitness pass (tree_SR_fitness) on the same forest, in the
same process, alternating the two; and of Forest.optimize_constants(steps=10) at configs[1]'s size.  Device events around each
call after warm-up; prints one JSON object (and writes it to --out when given).

  configs1   100 k trees x 1024 rows, 10 variables, gp_len 64, + - * /           (BASELINE configs[1])
  headline   1 M trees x 1024 rows, same descriptor                            (bench.py's headline forest)
  transc     100 k trees x 1024 rows, + - * / sin cos exp log
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
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="comma-separated subset of configs1,headline,transc,optimize")
    args = ap.parse_args()
    from evogp_amd.tree import Forest, GenerateDescriptor

    dev = torch.device("cuda:0")
    X, y = dataset(dev)
    cases = {
        "configs1": (100_000, ["+", "-", "*", "/"]),
        "headline": (1_000_000, ["+", "-", "*", "/"]),
        "transc": (100_000, ["+", "-", "*", "/", "sin", "cos", "exp", "log"]),
    }
    only = set(args.only.split(",")) if args.only else set(cases) | {"optimize"}
    result = {"device": torch.cuda.get_device_name(0), "rows": 1024, "var_len": 10, "gp_len": 64}
    for name, (pop, funcs) in cases.items():
        if name not in only:
            continue
        desc = GenerateDescriptor(max_tree_len=64, input_len=10, output_len=1, using_funcs=funcs, max_layer_cnt=6, const_samples=[-1, 0, 1])
        f = Forest.random_generate(pop, desc, keys=torch.tensor([42, 0], dtype=torch.uint32, device=dev))
        fit = lambda: f.SR_fitness(X, y)             # noqa: E731
        grad = lambda: f.SR_gradient(X, y)           # noqa: E731
        fit(), grad()
        torch.cuda.synchronize()
        tf, tg = [], []
        for _ in range(args.rounds):                 # alternating, same process
            tf.append(timed(fit, args.reps))
            tg.append(timed(grad, args.reps))
        nodes = int(f.batch_subtree_size[:, 0].clamp(min=0).sum())
        result[name] = {"pop": pop, "funcs": funcs, "live_nodes": nodes, "fitness_ms": min(tf), "gradient_ms": min(tg),
                        "ratio": min(tg) / min(tf), "fitness_ms_all": tf, "gradient_ms_all": tg,
                        "gradient_node_rows_per_s": nodes * 1024 / (min(tg) * 1e-3)}
        print(name, json.dumps(result[name]), flush=True)
        del f
        torch.cuda.empty_cache()
    if "optimize" in only:
        desc = GenerateDescriptor(max_tree_len=64, input_len=10, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=6,
                                  const_samples=[-1, 0, 1])
        f = Forest.random_generate(100_000, desc, keys=torch.tensor([42, 0], dtype=torch.uint32, device=dev))
        f.optimize_constants(X, y, steps=10)
        torch.cuda.synchronize()
        t = timed(lambda: f.optimize_constants(X, y, steps=10), 2)
        before = f.SR_fitness(X, y)
        _, after = f.optimize_constants(X, y, steps=10)
        fin = torch.isfinite(before) & torch.isfinite(after)
        result["optimize_configs1"] = {"pop": 100_000, "steps": 10, "ms": t, "mean_loss_before": float(before[fin].mean()),
                                       "mean_loss_after": float(after[fin].mean()), "improved_share": float((after[fin] < before[fin]).float().mean())}
        print("optimize", json.dumps(result["optimize_configs1"]), flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
