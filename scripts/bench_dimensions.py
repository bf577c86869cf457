"""Cost of dimensional analysis (csrc/sr_dims.hip, Forest.SR_dimensions) next to the interval pass (tree_intervals) on the same forest
in the same process: both are one-lane-per-tree walks over the live nodes with no dataset, the dimension pass walks twice (up, then
down for the consistent trees) and writes 4 K + 1 bytes per node where the interval pass writes 9.
One device-event pair around EVERY call after warm-up, the calls alternating; median, min and max over --calls calls (>= 20).  Prints
one JSON object and writes it to --out (default profiles/dimensions_bench.json).

  configs1   100 k trees, 10 variables, gp_len 64, + - * /           (BASELINE configs[1])
  headline   1 M trees, same descriptor                             (bench.py's headline forest)

``tree_dimensions_op_K3`` / ``_K8`` are the operator on units that are already on the device, i.e. the kernel, with 3 and with 8 base
dimensions; ``SR_dimensions_K3`` is the Forest method (it converts the units on the host and copies them to the device on every call).
The variables' units are drawn from {-1, 0, 1}^K with a fixed seed; the label is that of x0 * x1.  Also written: the share of the
trees that are dimensionally consistent, with the root held to the label and with the root free.  No threshold: nothing is gated."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_linear_scaling import measure  # noqa: E402

DEN = 25200


def units_of(K, var_len=10):
    rng = np.random.default_rng(100 + K)
    var = rng.integers(-1, 2, (var_len, K))
    return var, var[0] + var[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-headline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dimensions_bench.json"))
    args = ap.parse_args()
    assert args.calls >= 20, "median and min over at least 20 calls"
    from evogp_amd.tree import Forest, GenerateDescriptor

    dev = torch.device("cuda:0")
    desc = GenerateDescriptor(max_tree_len=64, input_len=10, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=6,
                              const_samples=[-1, 0, 1])
    keys = torch.tensor([42, 0], dtype=torch.uint32, device=dev)
    lower, upper = torch.full((10,), -1.0, device=dev), torch.full((10,), 1.0, device=dev)
    result = {"device": torch.cuda.get_device_name(0), "var_len": 10, "gp_len": 64, "timing": "one event pair per call"}
    on_dev = {}
    for K in (3, 8):
        var, label = units_of(K)
        on_dev[K] = (torch.tensor(var * DEN, dtype=torch.int32, device=dev), torch.tensor(label * DEN, dtype=torch.int32, device=dev))
    var3, label3 = (a.tolist() for a in units_of(3))

    for name, pop in (("configs1", 100_000),) + (() if args.no_headline else (("headline", 1_000_000),)):
        f = Forest.random_generate(pop, desc, keys=keys)
        calls = {"tree_intervals_op": lambda: torch.ops.evogp_hip.tree_intervals(*f._tensors(), lower, upper),
                 "tree_dimensions_op_K3": lambda: torch.ops.evogp_hip.tree_dimensions(*f._tensors(), *on_dev[3], True),
                 "tree_dimensions_op_K8": lambda: torch.ops.evogp_hip.tree_dimensions(*f._tensors(), *on_dev[8], True),
                 "SR_dimensions_K3": lambda: f.SR_dimensions(var3, label3)}
        r = measure(calls, args.calls, args.warmup)
        r["pop"] = f.pop_size
        r["mean_tree_len"] = float(f.batch_subtree_size[:, 0].float().mean())
        for K in (3, 8):
            r[f"dimensions_K{K}_over_intervals"] = r[f"tree_dimensions_op_K{K}"]["median_ms"] / r["tree_intervals_op"]["median_ms"]
            for root, check in (("label", True), ("free_root", False)):
                viol = torch.ops.evogp_hip.tree_dimensions(*f._tensors(), *on_dev[K], check)[2]
                r[f"consistent_share_K{K}_{root}"] = float((viol == 0).float().mean())
                r[f"malformed_K{K}"] = int((viol < 0).sum())
        result[name] = r
        print(name, json.dumps(r), flush=True)
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
