"""Cost of the population Gram matrix (csrc/sr_gram.hip; Forest.SR_gram) next to what a user had before it.  Device events around every
call after a warm-up call, medians of --reps repetitions, all in ONE process; writes one JSON object to --out
(profiles/gram_bench.json) and prints it.  No time is fixed in advance.

A fresh + - * / forest (gp_len 64, 10 variables, the benchmark's generator settings); per shape (n trees, D rows):
  gram_ms          tree_SR_gram, the whole call (residuals on)
  panel_ms         the panel kernels alone (evogp_hip_debug_sr_gram(1)): every tree interpreted once, float32 predictions to the workspace
  matrix_ms        the matrix kernels alone (evogp_hip_debug_sr_gram(2)) on the panel the call before left in the workspace
  torch_ms         batch_forward + .double() + (R @ R.T) and the two lin products: the same numbers through an (n, D) float64 copy and BLAS
  scaling_ms       tree_SR_linear_scaling on the same n trees: the cost of one interpretation per tree
  matrix_flops     n (n + 1) D / matrix time: the useful float64 operations of the upper triangle per second
  share_of_peak    matrix_flops over --peak (the float64 matrix peak of the device, 78.6e12 for an MI355X)
  max_rel_diff     the largest |G - G_torch| / sqrt(G_ii G_jj) over the finite words: what reordering the sum costs, for the record
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_semantics import times  # noqa: E402

SHAPES = [(256, 1024), (1024, 1024), (4096, 1024), (8192, 1024), (1024, 65536)]


def data(D, device):
    g = torch.Generator().manual_seed(1234)
    X = (torch.rand((D, 10), generator=g) * 10 - 5).to(device)
    y = (X[:, 0] * X[:, 1] + X[:, 2] * X[:, 3] - X[:, 4] + 0.5 * X[:, 5] ** 2).contiguous()
    return X, y


def measure(forest, n, D, reps, peak):
    from evogp_amd import _lib
    ops = torch.ops.evogp_hip
    sub = forest[:n]
    v, t, s = sub._tensors()
    X, y = data(D, v.device)
    index = torch.arange(n, dtype=torch.int32, device=v.device)
    call = lambda: ops.tree_SR_gram(v, t, s, X, y, index, True)   # noqa: E731

    def by_torch():
        R = sub.batch_forward(X)[:, :, 0].double() - y.double()[None, :]
        return R @ R.T, torch.stack([R.sum(1), R @ y.double()], 1)

    out = {"n": n, "rows": D, "gram_ms": times(call, reps)}
    for name, stages in (("panel_ms", 1), ("matrix_ms", 2)):
        assert _lib.lib.evogp_hip_debug_sr_gram(stages) == 0
        out[name] = times(call, reps)
    assert _lib.lib.evogp_hip_debug_sr_gram(3) == 0
    out["torch_ms"] = times(by_torch, reps)
    out["scaling_ms"] = times(lambda: ops.tree_SR_linear_scaling(n, D, v.shape[1], 10, 1, v, t, s, X, y[:, None].contiguous()), reps)
    out["matrix_flops"] = n * (n + 1) * D / (out["matrix_ms"]["median"] * 1e-3)
    out["share_of_peak"] = out["matrix_flops"] / peak
    G, _, usable = call()
    Gt = by_torch()[0]
    d = torch.sqrt(torch.diagonal(G)[:, None] * torch.diagonal(G)[None, :])
    ok = usable[:, None] & usable[None, :] & (d > 0)
    out["usable"] = int(usable.sum())
    out["max_rel_diff"] = float(((G - Gt).abs() / d)[ok].max()) if bool(ok.any()) else None
    print(f"# n={n} D={D}: gram {out['gram_ms']['median']:.3f} ms (panel {out['panel_ms']['median']:.3f}, matrix {out['matrix_ms']['median']:.3f}), "
          f"torch {out['torch_ms']['median']:.3f} ms, scaling {out['scaling_ms']['median']:.3f} ms, {out['matrix_flops'] / 1e12:.2f} TFLOP/s", file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--peak", type=float, default=78.6e12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gram_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_gram.py measures on the device: no GPU found")
    from evogp_amd.tree import Forest, GenerateDescriptor
    d = GenerateDescriptor(max_tree_len=64, input_len=10, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=5, const_samples=[-1, 0, 1, 2])
    forest = Forest.random_generate(8192, d, keys=torch.tensor([1, 2], dtype=torch.uint32, device="cuda"))
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "f64_matrix_peak": args.peak,
              "shapes": [measure(forest, n, D, args.reps, args.peak) for n, D in SHAPES]}
    text = json.dumps(result, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
