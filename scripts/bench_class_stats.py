"""Cost of the classification statistics (csrc/cls_stats.hip, Forest.class_stats) at BASELINE configs[3]'s shape -- classifier trees with
10 outputs, gp_len 128, sklearn digits 1797 x 64 -- at 200 k and at 20 k trees, for G = 1, 2 and 8 row splits, next to

  argmax_count            tree_batch_argmax_count as Classification.evaluate calls it (compiled programs, the END_CLS handler);
  argmax_count_tile_group the same op with EVOGP_TC_CLASSIFY=0: the tile-group kernel class_stats is built from, so the fair ratio.  The
                          switch is read once per process, so this figure comes from a CHILD process started with it, which times
                          class_stats (G = 1) next to it again -- the ratio is taken inside that child;
  torch_route             what a user did before: batch_forward in blocks of 1 GiB, torch.nn.functional.cross_entropy per row, arg-max
                          and a scatter_add confusion count;
  accuracy_path           Classification.evaluate itself; with --parent-root DIR (a built checkout of the parent commit) it is re-measured
                          in child processes alternating between this tree and the parent's, three each.

One device-event pair around EVERY call after warm-up, the kinds alternating; median, min, max and spread (median - min) over --calls
calls.  No time and no ratio is fixed in advance; the ratios and the interpreter rate (live nodes x rows per second: the kernel is under
the instruction-issue roof of the wave-uniform interpreter, its memory traffic is the forest once per row tile) are reported as measured.
Prints one JSON object and writes it to --out (default profiles/class_stats_bench.json)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def digits(dev):
    from sklearn import datasets   # the offline toy set Classification(dataset="digits") loads

    X, y = datasets.load_digits(return_X_y=True)
    return torch.tensor(X, dtype=torch.float32, device=dev), torch.tensor(y, dtype=torch.int32, device=dev)


def forest_of(pop, dev):
    from evogp_amd.tree import Forest, GenerateDescriptor

    desc = GenerateDescriptor(max_tree_len=128, input_len=64, output_len=10, using_funcs=["+", "-", "*", "/"], max_layer_cnt=6, const_samples=[-1, 0, 1])
    return Forest.random_generate(pop, desc, keys=torch.tensor([42, 0], dtype=torch.uint32, device=dev))


def argmax_count(f, X, y):
    return torch.ops.evogp_hip.tree_batch_argmax_count(f.pop_size, X.shape[0], f.max_tree_len, f.input_len, f.output_len, *f._tensors(), X, y)


def torch_route(f, X, y, block_bytes=1 << 30):
    import torch.nn.functional as F

    D, C = X.shape[0], f.output_len
    step = max(1, block_bytes // (4 * D * C))
    yl = y.to(torch.int64)
    out = []
    for i in range(0, f.pop_size, step):
        o = f[i:i + step].batch_forward(X)
        n = o.shape[0]
        loss = F.cross_entropy(o.reshape(-1, C), yl.repeat(n), reduction="none").view(n, D).mean(1)
        pred = o.argmax(2)
        predicted = torch.zeros(n, C, dtype=torch.int32, device=o.device).scatter_add_(1, pred, torch.ones_like(pred, dtype=torch.int32))
        hits = torch.zeros(n, C, dtype=torch.int32, device=o.device).scatter_add_(1, pred, (pred == yl[None, :]).to(torch.int32))
        out.append((hits, predicted, loss))
    return out


def child(args, env=None, root=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--calls", str(args.calls), "--warmup", str(args.warmup), "--out", ""]
    r = subprocess.run(cmd + (["--root", root] if root else []) + ["--child"], env=dict(os.environ, **(env or {})), capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"child failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pops", type=int, nargs="*", default=[200_000, 20_000])
    ap.add_argument("--root", default=HERE, help="the checkout whose evogp_amd is measured")
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit: re-measure the accuracy path against it")
    ap.add_argument("--child", action="store_true", help="(internal) argmax_count, the accuracy path and, where the tree has it, class_stats G = 1")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "class_stats_bench.json"))
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    import evogp_amd  # noqa: F401
    from evogp_amd.problem import Classification

    dev = torch.device("cuda:0")
    X, y = digits(dev)
    has_op = hasattr(torch.ops.evogp_hip, "tree_batch_class_stats")
    result = {"device": torch.cuda.get_device_name(0), "rows": X.shape[0], "var_len": 64, "out_len": 10, "gp_len": 128,
              "timing": "one event pair per call", "spread": "median - min", "tc_classify": os.environ.get("EVOGP_TC_CLASSIFY", "default")}
    rng = np.random.default_rng(7)
    g2 = torch.from_numpy((rng.random(X.shape[0]) < 0.3)).to(dev)
    g8 = torch.from_numpy(rng.integers(0, 8, X.shape[0]).astype(np.int32)).to(dev)
    for pop in args.pops:
        f = forest_of(pop, dev)
        prob = Classification(datapoints=X, labels=y.to(torch.float32))
        calls = {"argmax_count": lambda: argmax_count(f, X, y), "accuracy_path": lambda: prob.evaluate(f)}
        if has_op:
            calls["class_stats_G1"] = lambda: f.class_stats(X, y)
        if not args.child:
            calls["class_stats_G2"] = lambda: f.class_stats(X, y, g2)
            calls["class_stats_G8"] = lambda: f.class_stats(X, y, g8, 8)
            calls["torch_route"] = lambda: torch_route(f, X, y)
        r = measure(calls, args.calls, args.warmup)
        r["pop"] = pop
        node_rows = float(f.batch_subtree_size[:, 0].to(torch.int64).sum()) * X.shape[0]
        r["live_nodes_x_rows"] = node_rows
        if has_op:
            r["class_stats_G1_over_argmax_count"] = r["class_stats_G1"]["median_ms"] / r["argmax_count"]["median_ms"]
            r["class_stats_G1_G_node_rows_per_s"] = node_rows / r["class_stats_G1"]["median_ms"] / 1e6
            r["argmax_count_G_node_rows_per_s"] = node_rows / r["argmax_count"]["median_ms"] / 1e6
        if not args.child:
            g1 = r["class_stats_G1"]
            r["second_split_over_one"] = (r["class_stats_G2"]["median_ms"] - g1["median_ms"]) / g1["median_ms"]
            r["eight_splits_over_one"] = (r["class_stats_G8"]["median_ms"] - g1["median_ms"]) / g1["median_ms"]
            r["torch_route_over_class_stats_G1"] = r["torch_route"]["median_ms"] / g1["median_ms"]
            r["class_stats_beats_torch_route"] = g1["median_ms"] < r["torch_route"]["median_ms"] - r["torch_route"]["spread_ms"] - g1["spread_ms"]
            # the same answers: counts equal, losses within the float32 route's rounding
            hits, predicted, loss = f.class_stats(X, y)
            th = torch.cat([a for a, _, _ in torch_route(f, X, y)])
            r["hits_differ_from_raw_argmax_trees"] = int((hits[:, 0] != th).any(1).sum())   # (near-ties and NaN rows: torch's raw arg-max is not the rule)
            r["nan_loss_trees"] = int(torch.isnan(loss).sum())
        result[f"pop_{pop}"] = r
        print(f"pop_{pop}", json.dumps(r), flush=True)
        del f, calls
        torch.cuda.empty_cache()
    if not args.child:
        tile = child(args, env={"EVOGP_TC_CLASSIFY": "0"})
        result["tile_group_child"] = tile
        for pop in args.pops:
            result[f"pop_{pop}"]["class_stats_G1_over_argmax_count_tile_group"] = tile[f"pop_{pop}"]["class_stats_G1_over_argmax_count"]
        if args.parent_root:
            runs = {"this": [], "parent": []}
            for _ in range(3):                    # alternating processes
                runs["this"].append(child(args))
                runs["parent"].append(child(args, root=args.parent_root))
            acc = {}
            for pop in args.pops:
                for k, v in runs.items():
                    acc[f"pop_{pop}_{k}_median_ms"] = [x[f"pop_{pop}"]["accuracy_path"]["median_ms"] for x in v]
                a, b = statistics.median(acc[f"pop_{pop}_this_median_ms"]), statistics.median(acc[f"pop_{pop}_parent_median_ms"])
                acc[f"pop_{pop}_this_over_parent"] = a / b
            result["accuracy_path_vs_parent"] = acc
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
