"""The second-derivative passes (csrc/sr_hessian.hip) next to the route they replace and next to the per-interpretation yardstick, on the
configs[1] forest (100 k trees x 1024 rows, 10 variables, gp_len 64, + - * /, the forest of scripts/bench_sr_grad.py) and on the 1 M
forest, in one process, alternating after warm-up:

  * tree_SR_derivative_loss with pair codes (fused: no (pop, D) array) for P = 1, 3 and 8 pairs, with labels and bounds;
  * tree_SR_input_gradient with pair codes (materialising pred and the P second derivatives) for P = 1, 3 and 8 (the 1 M forest: P = 1);
  * the finite-difference route: two tree_SR_input_gradient calls with a plain wrt on X +- h e_b and the float32 difference of their
    dpred (P = 1) -- the op of the parent commit, unchanged here;
  * tree_SR_linear_scaling on the same forest: one plain register-stack interpretation of every tree on every row.

Device events around each call.  Prints one JSON object and writes it to --out (default profiles/hessian_bench.json).  The ratios are
recorded, not asserted."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.bench_sr_grad import dataset, timed  # noqa: E402

PAIR = 1 << 30
PAIRS = {1: [(3, 3)], 3: [(3, 3), (0, 3), (0, 7)], 8: [(3, 3), (0, 3), (0, 7), (1, 1), (2, 9), (5, 5), (4, 6), (0, 0)]}


def measure(pop, X, y, reps, rounds):
    from evogp_amd.tree import Forest, GenerateDescriptor

    dev = X.device
    desc = GenerateDescriptor(max_tree_len=64, input_len=10, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=6,
                              const_samples=[-1, 0, 1])
    f = Forest.random_generate(pop, desc, keys=torch.tensor([42, 0], dtype=torch.uint32, device=dev))
    value, ntype, size = f._tensors()
    D = X.shape[0]
    hip = torch.ops.evogp_hip
    codes = {P: [PAIR | a << 15 | b for a, b in q] for P, q in PAIRS.items()}
    d2 = {P: torch.randn(D, P, device=dev) for P in PAIRS}
    lo = {P: torch.zeros(P, device=dev) for P in PAIRS}
    hi = {P: torch.full((P,), float("inf"), device=dev) for P in PAIRS}
    e = torch.zeros_like(X)
    e[:, 3] = 1e-3
    Xp, Xm = X + e, X - e

    def finite_difference():
        up, down = hip.tree_SR_input_gradient(value, ntype, size, Xp, [3])[1], hip.tree_SR_input_gradient(value, ntype, size, Xm, [3])[1]
        return (up - down) / 2e-3

    calls = {"linear_scaling": lambda: hip.tree_SR_linear_scaling(pop, D, 64, 10, 1, value, ntype, size, X, y),
             "finite_difference_p1": finite_difference}
    for P in PAIRS:
        calls[f"curvature_loss_p{P}"] = (lambda P=P: hip.tree_SR_derivative_loss(value, ntype, size, X, y, d2[P], codes[P], lo[P], hi[P]))
        if P == 1 or pop <= 100_000:   # (the 1 M forest materialises 4 GiB per array: one pair there)
            calls[f"input_hessian_p{P}"] = (lambda P=P: hip.tree_SR_input_gradient(value, ntype, size, X, codes[P]))
    for fn in calls.values():   # warm-up
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(rounds):   # alternating, same process
        for k, fn in calls.items():
            times[k].append(timed(fn, reps))
    best = {k: min(v) for k, v in times.items()}
    return {"pop": pop, "rows": D, "var_len": 10, "gp_len": 64, "ms": best, "ms_all": times,
            "ratio_to_linear_scaling": {k: best[k] / best["linear_scaling"] for k in calls if k != "linear_scaling"},
            "ratio_to_finite_difference": {k: best[k] / best["finite_difference_p1"] for k in calls if k.endswith("_p1")}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pops", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hessian_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    X, y = dataset(dev)
    result = {"device": torch.cuda.get_device_name(0), "forests": [measure(pop, X, y, args.reps, args.rounds) for pop in args.pops]}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
