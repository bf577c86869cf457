"""Cost of rank-based fitness (csrc/sr_rank.hip; Forest.SR_spearman, RankFitness): the fused Spearman call next to the interpretation
without the sort (tree_SR_linear_scaling on the same forest and rows) and next to batch_forward + torch.argsort on a slice that fits in
memory.  Device events around every call after a warm-up call, medians of --reps repetitions, all in ONE process on ONE forest; writes one
JSON object to --out (profiles/rank_bench.json) and prints it.  No time is fixed in advance.

Shapes: "configs1" is configs[1] (100 k trees x 1024 rows, 10 variables, gp_len 64, + - * /) as ONE segment, the small build (a wave
sorts a tree alone); "panel" is --panel-segments segments of --panel-rows rows (256 x 3000: the large build, the workgroup sorts 4096
elements per tree and segment) on the first --panel-pop trees of the same forest.
  spearman_ms      tree_SR_rank_stats, fused sums only, on prepared payload and segments (what RankFitness.evaluate launches)
  scaling_ms       tree_SR_linear_scaling: one interpretation per tree and row, three float64 sums
  sort_share       1 - scaling_ms / spearman_ms: the part of the call the interpretation does not explain
  torch_ms         batch_forward + argsort(argsort) + a float64 correlation per segment on --slice trees, and the same slice through the op
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


def torch_spearman(forest, X, y, G, n):
    """Spearman per segment from the materialised predictions: ordinal ranks by two argsorts (no mid-ranks: the cheaper variant)"""
    P = forest.batch_forward(X)[:, :, 0].reshape(forest.pop_size, G, n)
    r = torch.argsort(torch.argsort(P, dim=2), dim=2).double()
    q = torch.argsort(torch.argsort(y.reshape(G, n), dim=1), dim=1).double()
    r, q = r - r.mean(2, keepdim=True), q - q.mean(1, keepdim=True)
    return ((r * q).sum(2) / torch.sqrt((r * r).sum(2) * (q * q).sum(1))).mean(1)


def measure(forest, X, y, G, n, reps, slice_):
    from evogp_amd.tree.forest import rank_segments

    ops = torch.ops.evogp_hip
    v, t, s = forest._tensors()
    pop, L = v.shape
    ids = torch.arange(G, device=X.device).repeat_interleave(n) if G > 1 else None
    segs = rank_segments(ids, G * n, X.device)
    r2 = ops.rank_rows(y, None, segs.seg_start, segs.max_segment)[0]
    out = {"pop": pop, "rows": G * n, "segments": G, "rows_per_segment": n}
    out["spearman_ms"] = times(lambda: forest._rank_call(X, r2, segs, "spearman", "fused"), reps)
    out["scaling_ms"] = times(lambda: ops.tree_SR_linear_scaling(pop, G * n, L, X.shape[1], 1, v, t, s, X, y[:, None].contiguous()), reps)
    out["sort_share"] = 1.0 - out["scaling_ms"]["median"] / out["spearman_ms"]["median"]
    status = forest._rank_call(X, r2, segs, "spearman", "fused")[3]
    out["unusable_share"] = float((status != 0).double().mean())
    sub = forest[:slice_]
    out["slice"] = {"trees": slice_, "torch_ms": times(lambda: torch_spearman(sub, X, y, G, n), reps),
                    "spearman_ms": times(lambda: sub._rank_call(X, r2, segs, "spearman", "fused"), reps)}
    print(f"# {pop} trees x {G} x {n} rows: spearman {out['spearman_ms']['median']:.3f} ms, scaling {out['scaling_ms']['median']:.3f} ms, "
          f"slice of {slice_}: torch {out['slice']['torch_ms']['median']:.3f} ms, op {out['slice']['spearman_ms']['median']:.3f} ms",
          file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pop", type=int, default=100_000)
    ap.add_argument("--panel-pop", type=int, default=4096)
    ap.add_argument("--panel-segments", type=int, default=256)
    ap.add_argument("--panel-rows", type=int, default=3000)
    ap.add_argument("--slice", type=int, default=2048)
    ap.add_argument("--panel-slice", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_rank.py measures on a GPU; there is no fallback"
    import evogp_amd  # noqa: F401
    from evogp_amd.tree import Forest, GenerateDescriptor

    dev = torch.device("cuda")
    desc = GenerateDescriptor(max_tree_len=64, input_len=10, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=6,
                              const_samples=[-1, 0, 1])
    forest = Forest.random_generate(args.pop, desc, keys=torch.tensor([42, 0], dtype=torch.uint32, device=dev))
    gen = torch.Generator(device=dev).manual_seed(1234)

    def data(rows):
        X = torch.rand(rows, 10, device=dev, generator=gen) * 10 - 5
        return X, (X[:, 0] * X[:, 1] + X[:, 2] * X[:, 3] - X[:, 4] + 0.5 * X[:, 5] ** 2).contiguous()

    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "mean_tree_len": float(forest.batch_subtree_size[:, 0].float().mean())}
    res["configs1"] = measure(forest, *data(1024), 1, 1024, args.reps, args.slice)
    G, n = args.panel_segments, args.panel_rows
    res["panel"] = measure(forest[:args.panel_pop], *data(G * n), G, n, args.reps, args.panel_slice)
    res["notes"] = ["times are device-event medians of one process; min and max are next to them",
                    "fused sums against the numpy restatement (tests/test_gpu_rank.py): worst error / bound 0 on every case, bit-equal; "
                    "the test asserts equality",
                    "the torch route ranks ordinally (no mid-ranks): it does less than the op"]
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
