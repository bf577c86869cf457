"""Cost of multi-gene fitness (csrc/sr_genes.hip, Forest.SR_gene_fitness) next to the composition a user had before -- batch_forward plus
the float64 torch normal equations (SymbolicRegression(multigene=True, execute_mode="torch")), which writes and rereads the (pop, D, G)
outputs -- and next to SR_fitness on the same forest (G separate targets: the labels repeated G times).
One device-event pair around EVERY call after warm-up, the calls of the three kinds alternating in the same process; median, min and
max over --calls calls (>= 20).  Prints one JSON object and writes it to --out (default profiles/genes_bench.json).

  g4, g8     100 k trees x 1024 rows, 10 variables, gp_len 64, + - * /, output_len 4 and 8; all three
  headline   1 M trees x 1024 rows, output_len 4; no composition there: its outputs alone are 16 GB

Ready when, at 100 k, the median of the new call lies below the composition's median by more than the composition's own
min-to-median spread ("ready"), for both output_len.  The ratio to SR_fitness is reported, not gated."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_linear_scaling import dataset, measure  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-headline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "genes_bench.json"))
    args = ap.parse_args()
    assert args.calls >= 20, "median and min over at least 20 calls"
    from evogp_amd.problem import SymbolicRegression
    from evogp_amd.tree import Forest, GenerateDescriptor

    dev = torch.device("cuda:0")
    X, y = dataset(dev)
    keys = torch.tensor([42, 0], dtype=torch.uint32, device=dev)
    composed = SymbolicRegression(datapoints=X, labels=y, multigene=True, execute_mode="torch")
    result = {"device": torch.cuda.get_device_name(0), "rows": 1024, "var_len": 10, "gp_len": 64, "timing": "one event pair per call"}

    def forest(pop, G):
        desc = GenerateDescriptor(max_tree_len=64, input_len=10, output_len=G, using_funcs=["+", "-", "*", "/"], max_layer_cnt=6,
                                  const_samples=[-1, 0, 1])
        return Forest.random_generate(pop, desc, keys=keys), y.expand(-1, G).contiguous()

    for G in (4, 8):
        f, yG = forest(100_000, G)
        r = measure({"gene_fitness": lambda: f.SR_gene_fitness(X, y), "sr_fitness": lambda: f.SR_fitness(X, yG),
                     "batch_forward_plus_torch_float64": lambda: composed.gene_model(f)}, args.calls, args.warmup)
        comp, new = r["batch_forward_plus_torch_float64"], r["gene_fitness"]
        r["pop"], r["output_len"] = f.pop_size, G
        r["gene_over_sr_fitness"] = new["median_ms"] / r["sr_fitness"]["median_ms"]
        r["composition_over_gene"] = comp["median_ms"] / new["median_ms"]
        r["composition_spread_ms"] = comp["median_ms"] - comp["min_ms"]
        r["ready"] = new["median_ms"] < comp["median_ms"] - r["composition_spread_ms"]
        loss, coef = f.SR_gene_fitness(X, y)
        tl, _ = composed.gene_model(f)
        fin = torch.isfinite(loss) & torch.isfinite(tl)
        r["nan_trees"] = int(torch.isnan(loss).sum())
        r["nan_masks_equal"] = bool(torch.equal(torch.isnan(loss), torch.isnan(tl)))
        syy_D = float(y.double().var(unbiased=False))
        r["max_abs_diff_to_composition_over_syy"] = float((loss[fin] - tl[fin]).abs().max()) / syy_D
        r["share_within_1e-6_syy"] = float(((loss[fin] - tl[fin]).abs() <= 1e-6 * syy_D).double().mean())
        r["mean_kept_genes"] = float((coef[fin][:, 1:] != 0).sum(1).double().mean())
        r["median_loss"] = float(loss[fin].double().median())
        result[f"g{G}"] = r
        print(f"g{G}", json.dumps(r), flush=True)
        del f
        torch.cuda.empty_cache()

    if not args.no_headline:
        f, yG = forest(1_000_000, 4)
        r = measure({"gene_fitness": lambda: f.SR_gene_fitness(X, y), "sr_fitness": lambda: f.SR_fitness(X, yG)}, args.calls, args.warmup)
        r["pop"], r["output_len"] = f.pop_size, 4
        r["gene_over_sr_fitness"] = r["gene_fitness"]["median_ms"] / r["sr_fitness"]["median_ms"]
        result["headline"] = r
        print("headline", json.dumps(r), flush=True)
        del f
        torch.cuda.empty_cache()

    result["ready"] = result["g4"]["ready"] and result["g8"]["ready"]
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
