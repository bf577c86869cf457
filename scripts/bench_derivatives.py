"""Cost of the derivative bounds (csrc/sr_deriv.hip, Forest.SR_derivative_intervals) for K = 1 and K = 4 requested variables next to
SR_intervals on the same forest and next to SR_subtree_errors, the only other call that learns something about every subtree: that one
does O(nodes x rows) work where the two launches here do O(nodes) and O(K x nodes), so a derivative pass that is not faster is wrong,
not slow.
One device-event pair around EVERY call after warm-up, the calls alternating in the same process; median, min and max over --calls
calls (>= 20).  Prints one JSON object and writes it to --out (default profiles/derivative_bounds_bench.json).

  configs1   100 k trees x 1024 rows, 10 variables, gp_len 64, + - * /           (BASELINE configs[1])
  headline   1 M trees, same descriptor                                         (bench.py's headline forest); no SR_subtree_errors there

Also written: the share of the fresh forest that is provably nondecreasing in x0 on [-1, 1]^10 (``monotone_mask``), next to the share
that is safe there, and the share whose root depends on x0 at all.

Ready when, at configs1, the median of the K = 1 call lies below the median of SR_subtree_errors ("ready").  The ratio to SR_intervals
is reported, not gated."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_linear_scaling import dataset, measure  # noqa: E402


def shares(f):
    dlo, dhi, dfl = f.SR_derivative_intervals(-1.0, 1.0, wrt=[0])
    root = dfl[0, :, 0]
    up = f.monotone_mask(-1.0, 1.0, {0: 1})
    depends = (root & 4) != 0
    return {"nondecreasing_in_x0_share_unit_box": float(up.float().mean()),
            "nondecreasing_and_depends_on_x0_share": float((up & depends).float().mean()),
            "safe_share_unit_box": float(f.safe_mask(-1.0, 1.0).float().mean()),
            "depends_on_x0_share": float(depends.float().mean()),
            "jump_share": float(((root & 1) != 0).float().mean()),
            "finite_bounds_share": float((torch.isfinite(dlo[0, :, 0]) & torch.isfinite(dhi[0, :, 0])).float().mean()),
            "malformed": int(((root & 2) != 0).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-headline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "derivative_bounds_bench.json"))
    args = ap.parse_args()
    assert args.calls >= 20, "median and min over at least 20 calls"
    from evogp_amd.tree import Forest, GenerateDescriptor

    dev = torch.device("cuda:0")
    X, y = dataset(dev)
    desc = GenerateDescriptor(max_tree_len=64, input_len=10, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=6,
                              const_samples=[-1, 0, 1])
    keys = torch.tensor([42, 0], dtype=torch.uint32, device=dev)
    result = {"device": torch.cuda.get_device_name(0), "rows": 1024, "var_len": 10, "gp_len": 64, "timing": "one event pair per call"}

    def calls_of(f, with_subtree):
        c = {"SR_derivative_intervals_k1": lambda: f.SR_derivative_intervals(-1.0, 1.0, wrt=[0]),
             "SR_derivative_intervals_k4": lambda: f.SR_derivative_intervals(-1.0, 1.0, wrt=[0, 1, 2, 3]),
             "SR_intervals": lambda: f.SR_intervals(-1.0, 1.0)}
        if with_subtree:
            c["sr_subtree_errors"] = lambda: f.SR_subtree_errors(X, y)
        return c

    for name, pop in (("configs1", 100_000),) + (() if args.no_headline else (("headline", 1_000_000),)):
        f = Forest.random_generate(pop, desc, keys=keys)
        r = measure(calls_of(f, name == "configs1"), args.calls, args.warmup)
        r["pop"] = f.pop_size
        r["mean_tree_len"] = float(f.batch_subtree_size[:, 0].float().mean())
        r["k1_over_intervals"] = r["SR_derivative_intervals_k1"]["median_ms"] / r["SR_intervals"]["median_ms"]
        r["k4_over_k1"] = r["SR_derivative_intervals_k4"]["median_ms"] / r["SR_derivative_intervals_k1"]["median_ms"]
        if name == "configs1":
            r["subtree_errors_over_k1"] = r["sr_subtree_errors"]["median_ms"] / r["SR_derivative_intervals_k1"]["median_ms"]
            r["ready"] = r["SR_derivative_intervals_k1"]["median_ms"] < r["sr_subtree_errors"]["median_ms"]
        r.update(shares(f))
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
