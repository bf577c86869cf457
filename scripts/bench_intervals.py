"""Cost of the interval pass (csrc/sr_interval.hip, Forest.SR_intervals) next to SR_fitness on the same forest and next to
SR_subtree_errors, the cheapest existing call that produces a (pop, L) result: that one does O(nodes x rows) work where the interval
pass does O(nodes), so an interval pass that is not faster is wrong, not slow.
One device-event pair around EVERY call after warm-up, the calls alternating in the same process; median, min and max over --calls
calls (>= 20).  Prints one JSON object and writes it to --out (default profiles/intervals_bench.json).

  configs1   100 k trees x 1024 rows, 10 variables, gp_len 64, + - * /           (BASELINE configs[1])
  headline   1 M trees, same descriptor                                         (bench.py's headline forest); no SR_subtree_errors there

``SR_intervals`` is the Forest method (it checks the box on the host and copies it to the device on every call); ``tree_intervals_op``
is the operator on a box that is already on the device, i.e. the kernel.  Also written: the share of the trees that are safe on the
box [-1, 1]^var_len and on the dataset's own box.

Ready when, at configs1, the median of SR_intervals lies below the median of SR_subtree_errors ("ready").  The ratio to SR_fitness is
reported, not gated."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_linear_scaling import dataset, measure  # noqa: E402


def shares(f, X):
    lo, hi, flags = f.SR_intervals(-1.0, 1.0)
    unit = f.safe_mask(-1.0, 1.0)
    data = f.safe_mask(X.min(0).values, X.max(0).values)
    return {"safe_share_unit_box": float(unit.float().mean()), "safe_share_data_box": float(data.float().mean()),
            "may_nan_share_unit_box": float(((flags[:, 0] & 1) != 0).float().mean()),
            "unbounded_share_unit_box": float((((flags[:, 0] & 1) == 0) & ~(torch.isfinite(lo[:, 0]) & torch.isfinite(hi[:, 0]))).float().mean()),
            "malformed": int(((flags[:, 0] & 2) != 0).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-headline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "intervals_bench.json"))
    args = ap.parse_args()
    assert args.calls >= 20, "median and min over at least 20 calls"
    from evogp_amd.tree import Forest, GenerateDescriptor

    dev = torch.device("cuda:0")
    X, y = dataset(dev)
    desc = GenerateDescriptor(max_tree_len=64, input_len=10, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=6,
                              const_samples=[-1, 0, 1])
    keys = torch.tensor([42, 0], dtype=torch.uint32, device=dev)
    lower, upper = torch.full((10,), -1.0, device=dev), torch.full((10,), 1.0, device=dev)
    result = {"device": torch.cuda.get_device_name(0), "rows": 1024, "var_len": 10, "gp_len": 64, "timing": "one event pair per call"}

    def calls_of(f, with_subtree):
        c = {"SR_intervals": lambda: f.SR_intervals(-1.0, 1.0),
             "tree_intervals_op": lambda: torch.ops.evogp_hip.tree_intervals(*f._tensors(), lower, upper),
             "sr_fitness": lambda: f.SR_fitness(X, y)}
        if with_subtree:
            c["sr_subtree_errors"] = lambda: f.SR_subtree_errors(X, y)
        return c

    for name, pop in (("configs1", 100_000),) + (() if args.no_headline else (("headline", 1_000_000),)):
        f = Forest.random_generate(pop, desc, keys=keys)
        r = measure(calls_of(f, name == "configs1"), args.calls, args.warmup)
        r["pop"] = f.pop_size
        r["mean_tree_len"] = float(f.batch_subtree_size[:, 0].float().mean())
        r["intervals_over_sr_fitness"] = r["SR_intervals"]["median_ms"] / r["sr_fitness"]["median_ms"]
        if name == "configs1":
            r["subtree_errors_over_intervals"] = r["sr_subtree_errors"]["median_ms"] / r["SR_intervals"]["median_ms"]
            r["ready"] = r["SR_intervals"]["median_ms"] < r["sr_subtree_errors"]["median_ms"]
        r.update(shares(f, X))
        result[name] = r
        print(name, json.dumps(r), flush=True)
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
