"""Cost of the semantic neighbourhoods (csrc/sr_neigh.hip; Forest.SR_neighbours) next to the only route a user had before it: the n x n
matrix of SR_gram and torch.topk on it.  Device events around every call after a warm-up call, medians of --reps repetitions, all in
ONE process; writes one JSON object to --out (profiles/neighbours_bench.json) and prints it.  No time is fixed in advance.

A fresh + - * / forest (gp_len 64, 10 variables, the benchmark's generator settings), k = 15 and one radius; per shape (n trees, D rows):
  neighbours_ms    tree_SR_neighbours, the whole call
  panel_ms, norm_ms, strip_ms, merge_ms   one stage alone (evogp_hip_debug_sr_neighbours(1 / 2 / 4 / 8)) on what the call before left
  gram_topk_ms     n <= 8192: tree_SR_gram without residuals, d2 = N_i + N_j - 2 G on the (n, n) matrix, the diagonal and the unusable
                   columns set to +inf, torch.topk(k, largest=False) and the count within the radius
  gram_matrix_ms   n <= 8192: SR_gram's matrix kernels alone (evogp_hip_debug_sr_gram(2)), the upper triangle
  strip_flops      2 n^2 D / strip time: the useful float64 operations of the full square per second;  gram_flops: n (n + 1) D / matrix time
  share_of_peak    strip_flops over --peak (the float64 matrix peak of the device, 78.6e12 for an MI355X)
  same             n <= 8192: dist2 equals the n x n route's values bit for bit (the two share the order of summation)
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_gram import data  # noqa: E402
from bench_semantics import times  # noqa: E402

SHAPES = [(1024, 1024), (4096, 1024), (8192, 1024), (32768, 1024), (100000, 1024), (8192, 65536)]
K = 15


def measure(forest, n, D, reps, peak):
    from evogp_amd import _lib
    ops = torch.ops.evogp_hip
    v, t, s = forest[:n]._tensors()
    X, _ = data(D, v.device)
    index = torch.arange(n, dtype=torch.int32, device=v.device)
    norm = ops.tree_SR_neighbours(v, t, s, X, index[:min(n, 4096)], 1, torch.zeros(0, dtype=torch.float64, device=v.device))[3]
    radius2 = torch.nanmedian(norm).reshape(1) * 0.01   # a tenth of the median norm as a distance
    call = lambda: ops.tree_SR_neighbours(v, t, s, X, index, K, radius2)   # noqa: E731

    out = {"n": n, "rows": D, "k": K, "neighbours_ms": times(call, reps)}
    for name, stages in (("panel_ms", 1), ("norm_ms", 2), ("strip_ms", 4), ("merge_ms", 8)):
        assert _lib.lib.evogp_hip_debug_sr_neighbours(stages) == 0
        out[name] = times(call, reps)
    assert _lib.lib.evogp_hip_debug_sr_neighbours(15) == 0
    out["strip_flops"] = 2.0 * n * n * D / (out["strip_ms"]["median"] * 1e-3)
    out["share_of_peak"] = out["strip_flops"] / peak
    dist2, _, count, _, usable = call()
    out["usable"] = int(usable.sum())
    out["mean_count"] = float(count[usable].double().mean())
    line = f"# n={n} D={D}: neighbours {out['neighbours_ms']['median']:.3f} ms (panel {out['panel_ms']['median']:.3f}, norm {out['norm_ms']['median']:.3f}, " \
           f"strip {out['strip_ms']['median']:.3f}, merge {out['merge_ms']['median']:.3f}), strip {out['strip_flops'] / 1e12:.2f} TFLOP/s"
    if n <= 8192 and n * D <= 1 << 26:   # the n x n route (SR_gram's cap; its slab loop is not what is compared at 65536 rows)
        def by_gram():
            G, _, use = ops.tree_SR_gram(v, t, s, X, None, index, False)
            N = torch.diagonal(G)
            d2 = torch.clamp_min((N[:, None] + N[None, :]) - 2.0 * G, 0.0)
            d2 = torch.where(use[None, :] & ~torch.eye(n, dtype=torch.bool, device=G.device), d2, float("inf"))
            return torch.topk(d2, K, dim=1, largest=False, sorted=True)[0], (d2 <= radius2).sum(1)
        out["gram_topk_ms"] = times(by_gram, reps)
        assert _lib.lib.evogp_hip_debug_sr_gram(2) == 0
        out["gram_matrix_ms"] = times(lambda: ops.tree_SR_gram(v, t, s, X, None, index, False), reps)
        assert _lib.lib.evogp_hip_debug_sr_gram(3) == 0
        out["gram_flops"] = n * (n + 1) * D / (out["gram_matrix_ms"]["median"] * 1e-3)
        want, want_count = by_gram()
        out["same"] = bool(torch.equal(dist2[usable], want[usable]) and torch.equal(count[usable, 0].long(), want_count[usable]))
        line += f"; gram + topk {out['gram_topk_ms']['median']:.3f} ms, gram matrix {out['gram_matrix_ms']['median']:.3f} ms, same {out['same']}"
    print(line, file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--peak", type=float, default=78.6e12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neighbours_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_neighbours.py measures on the device: no GPU found")
    from evogp_amd.tree import Forest, GenerateDescriptor
    d = GenerateDescriptor(max_tree_len=64, input_len=10, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=5, const_samples=[-1, 0, 1, 2])
    forest = Forest.random_generate(max(n for n, _ in SHAPES), d, keys=torch.tensor([1, 2], dtype=torch.uint32, device="cuda"))
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "f64_matrix_peak": args.peak, "shapes": []}
    for n, D in SHAPES:
        result["shapes"].append(measure(forest, n, D, args.reps, args.peak))
        with open(args.out, "w") as f:   # (kept up to date shape by shape)
            f.write(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
