"""The input-gradient passes (csrc/sr_xgrad.hip) next to what they are the same two walks as, and next to what they replace, on the
configs[1] forest (100 k trees x 1024 rows, 10 variables, gp_len 64, + - * /, the forest of scripts/bench_sr_grad.py) and on the 1 M
forest, in one process, alternating after warm-up:

  * tree_SR_derivative_loss (fused: no (pop, D) array) for V = 1, 3 and 8 requested variables, with labels and bounds;
  * tree_SR_input_gradient (materialising pred and dpred) for V = 1;
  * tree_SR_gradient, the constant gradient: the expectation is that the fused loss costs about one such launch;
  * the finite-difference route the ops replace: 2 V calls of Forest.batch_forward on X +- h e_v plus float64 torch reductions over the
    (pop, D) matrices (V = 1; also V = 3 on the 100 k forest).

Device events around each call.  Prints one JSON object and writes it to --out (default profiles/input_gradients_bench.json).  The
ratios are recorded, not asserted."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.bench_sr_grad import dataset, timed  # noqa: E402


def finite_differences(forest, X, y, dy, wrt, h=1e-3):
    """the route without a kernel: loss columns (pop, 1 + V) from 2 V + 1 batch_forward calls, float64 reductions"""
    p0 = forest.batch_forward(X)[:, :, 0].double()
    cols = [((p0 - y.double()[None, :, 0]) ** 2).mean(1)]
    for k, v in enumerate(wrt):
        e = torch.zeros_like(X)
        e[:, v] = h
        g = (forest.batch_forward(X + e)[:, :, 0].double() - forest.batch_forward(X - e)[:, :, 0].double()) / (2 * h)
        cols.append(((g - dy.double()[None, :, k]) ** 2).mean(1))
    return torch.stack(cols, 1).float()


def measure(pop, X, y, reps, rounds, fd_vars):
    from evogp_amd.tree import Forest, GenerateDescriptor

    dev = X.device
    desc = GenerateDescriptor(max_tree_len=64, input_len=10, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=6,
                              const_samples=[-1, 0, 1])
    f = Forest.random_generate(pop, desc, keys=torch.tensor([42, 0], dtype=torch.uint32, device=dev))
    value, ntype, size = f._tensors()
    D = X.shape[0]
    hip = torch.ops.evogp_hip
    wrts = {1: [3], 3: [3, 0, 7], 8: [3, 0, 7, 1, 9, 2, 5, 4]}
    dys = {V: torch.randn(D, V, device=dev) for V in wrts}
    lo = {V: torch.full((V,), -1.0, device=dev) for V in wrts}
    hi = {V: torch.full((V,), 1.0, device=dev) for V in wrts}
    calls = {"gradient": lambda: hip.tree_SR_gradient(pop, D, 64, 10, 1, True, value, ntype, size, X, y)}
    for V, wrt in wrts.items():
        calls[f"derivative_loss_v{V}"] = (lambda V=V, wrt=wrt: hip.tree_SR_derivative_loss(value, ntype, size, X, y, dys[V], wrt, lo[V], hi[V]))
    calls["input_gradient_v1"] = lambda: hip.tree_SR_input_gradient(value, ntype, size, X, wrts[1])
    for V in fd_vars:
        calls[f"finite_differences_v{V}"] = (lambda V=V: finite_differences(f, X, y, dys[V], wrts[V]))
    for fn in calls.values():   # warm-up
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(rounds):   # alternating, same process
        for k, fn in calls.items():
            times[k].append(timed(fn, 1 if k.startswith("finite") else reps))
    best = {k: min(v) for k, v in times.items()}
    return {"pop": pop, "rows": D, "var_len": 10, "gp_len": 64, "ms": best, "ms_all": times,
            "ratio_to_gradient": {k: best[k] / best["gradient"] for k in calls if k != "gradient"}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pops", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "input_gradients_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    X, y = dataset(dev)
    result = {"device": torch.cuda.get_device_name(0),
              "forests": [measure(pop, X, y, args.reps, args.rounds, (1, 3) if pop <= 100_000 else (1,)) for pop in args.pops]}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
