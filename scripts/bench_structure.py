"""Cost of the structural pass (csrc/sr_structure.hip, Forest.SR_structure) next to dimensional analysis (tree_dimensions, K = 3) and the
interval pass (tree_intervals) on the same forest in the same process: all three are one-lane-per-tree walks over the live nodes with
no dataset.  The structural pass walks twice (up, then down for the depths) and writes 9 + R bytes per node, the dimension pass 4 K + 1
and the interval pass 9.
One device-event pair around EVERY call after warm-up, the calls alternating; median, min and max over --calls calls (>= 20).  Prints
one JSON object and writes it to --out (default profiles/structure_bench.json).

  configs1   100 k trees, 10 variables, gp_len 64, + - * /           (BASELINE configs[1])
  headline   1 M trees, same descriptor                             (bench.py's headline forest)

``tree_structure_op_R0`` / ``_R2`` / ``_R8`` are the operator on tables that are already on the device, i.e. the kernel, with no rule,
two and eight nesting rules (over + - * /, so that every rule counts on these forests), a depth and a complexity limit;
``SR_structure_R2`` is the Forest method (it parses the dictionaries on the host and copies the tables to the device on every call).
Also written: the share of a fresh + - * / sin cos forest (100 k trees, same descriptor otherwise) that passes "no sine or cosine
inside a sine or a cosine" with max_depth=6, and under each of the two limits alone.  No threshold: nothing is gated; the two sibling
kernels are the yardstick."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_linear_scaling import measure  # noqa: E402

NESTED = {0: None,
          2: {"*": {"*": 2}, "/": {"/": 1}},
          8: {"*": {"*": 2, "/": 1, "+": 3}, "/": {"/": 1, "*": 2, "-": 3}, "+": {"*": 4}, "-": {"/": 4}}}
COSTS = {"/": 2, "const": 2}
NO_NESTED_TRIG = {"sin": {"sin": 0, "cos": 0}, "cos": {"sin": 0, "cos": 0}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-headline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "structure_bench.json"))
    args = ap.parse_args()
    assert args.calls >= 20, "median and min over at least 20 calls"
    from evogp_amd.tree import Forest, GenerateDescriptor
    from evogp_amd.tree.utils import parse_structure

    dev = torch.device("cuda:0")
    desc = GenerateDescriptor(max_tree_len=64, input_len=10, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=6,
                              const_samples=[-1, 0, 1])
    keys = torch.tensor([42, 0], dtype=torch.uint32, device=dev)
    lower, upper = torch.full((10,), -1.0, device=dev), torch.full((10,), 1.0, device=dev)
    var_units = torch.randint(-1, 2, (10, 3), generator=torch.Generator().manual_seed(103)).to(torch.int32).to(dev) * 25200
    label_units = (var_units[0] + var_units[1]).contiguous()
    result = {"device": torch.cuda.get_device_name(0), "var_len": 10, "gp_len": 64, "timing": "one event pair per call",
              "max_depth": 6, "max_complexity": 40, "complexity_of": COSTS, "nested": {str(k): v for k, v in NESTED.items()}}

    def words(x, shape):
        return torch.tensor([v - (1 << 32) if v >= 1 << 31 else v for v in x], dtype=torch.int32).reshape(shape).to(dev)

    on_dev = {}
    for R, nested in NESTED.items():
        cost, oplim, rules = parse_structure(COSTS, nested, {"/": (-1, 5)})
        assert len(rules) == R
        on_dev[R] = (words(cost, (32,)), words([x for row in oplim for x in row], (32, 3)), words([r[0] for r in rules], (R,)),
                     words([r[1] for r in rules], (R,)), words([r[2] for r in rules], (R,)), 6, 40)

    for name, pop in (("configs1", 100_000),) + (() if args.no_headline else (("headline", 1_000_000),)):
        f = Forest.random_generate(pop, desc, keys=keys)
        calls = {"tree_intervals_op": lambda: torch.ops.evogp_hip.tree_intervals(*f._tensors(), lower, upper),
                 "tree_dimensions_op_K3": lambda: torch.ops.evogp_hip.tree_dimensions(*f._tensors(), var_units, label_units, True),
                 "tree_structure_op_R0": lambda: torch.ops.evogp_hip.tree_structure(*f._tensors(), *on_dev[0]),
                 "tree_structure_op_R2": lambda: torch.ops.evogp_hip.tree_structure(*f._tensors(), *on_dev[2]),
                 "tree_structure_op_R8": lambda: torch.ops.evogp_hip.tree_structure(*f._tensors(), *on_dev[8]),
                 "SR_structure_R2": lambda: f.SR_structure(COSTS, NESTED[2], {"/": (-1, 5)}, 6, 40)}
        r = measure(calls, args.calls, args.warmup)
        r["pop"] = f.pop_size
        r["mean_tree_len"] = float(f.batch_subtree_size[:, 0].float().mean())
        for R in NESTED:
            for other, short in (("tree_dimensions_op_K3", "dimensions_K3"), ("tree_intervals_op", "intervals")):
                r[f"structure_R{R}_over_{short}"] = r[f"tree_structure_op_R{R}"]["median_ms"] / r[other]["median_ms"]
            viol = torch.ops.evogp_hip.tree_structure(*f._tensors(), *on_dev[R])[5]
            r[f"pass_share_R{R}"] = float((viol == 0).float().mean())
            r[f"malformed_R{R}"] = int((viol < 0).sum())
        result[name] = r
        print(name, json.dumps(r), flush=True)
        del f
        torch.cuda.empty_cache()

    trig = Forest.random_generate(100_000, desc.update(using_funcs=["+", "-", "*", "/", "sin", "cos"]), keys=keys)
    height = trig.SR_structure()[1][:, 0]
    result["trig_forest"] = {
        "pop": trig.pop_size, "using_funcs": ["+", "-", "*", "/", "sin", "cos"], "mean_tree_len": float(trig.batch_subtree_size[:, 0].float().mean()),
        "max_height": int(height.max()),
        "pass_share_no_nested_trig_max_depth_6": float(trig.structure_mask(nested_constraints=NO_NESTED_TRIG, max_depth=6).float().mean()),
        "pass_share_no_nested_trig": float(trig.structure_mask(nested_constraints=NO_NESTED_TRIG).float().mean()),
        "pass_share_max_depth_6": float(trig.structure_mask(max_depth=6).float().mean()),
    }
    print("trig_forest", json.dumps(result["trig_forest"]), flush=True)

    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
