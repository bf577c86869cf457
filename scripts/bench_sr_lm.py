"""Levenberg-Marquardt against the descent on the configs[1] forest (100 k trees x 1024 rows, 10 variables, gp_len 64, + - * /, the
forest of tests/test_gpu_sr_grad.py::test_optimize_constants_configs1_forest): the cost of one normal-equation launch
(tree_SR_normal_eq) next to one gradient launch (tree_SR_gradient) on the same forest, in the same process, alternating the two;
the cost of one step launch of each method; and the median loss after 1, 2, 5 and 10 steps of Forest.optimize_constants with each
method.  Device events around each call after warm-up; prints one JSON object (and writes it to --out when given)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.bench_sr_grad import dataset, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pop", type=int, default=100_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from evogp_amd.tree import Forest, GenerateDescriptor

    dev = torch.device("cuda:0")
    X, y = dataset(dev)
    desc = GenerateDescriptor(max_tree_len=64, input_len=10, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=6,
                              const_samples=[-1, 0, 1])
    f = Forest.random_generate(args.pop, desc, keys=torch.tensor([42, 0], dtype=torch.uint32, device=dev))
    value, ntype, size = f._tensors()
    shape = (args.pop, 1024, 64, 10, 1)
    grad = lambda: torch.ops.evogp_hip.tree_SR_gradient(*shape, True, value, ntype, size, X, y)   # noqa: E731
    neq = lambda: torch.ops.evogp_hip.tree_SR_normal_eq(*shape, value, ntype, size, X, y)         # noqa: E731
    fit = lambda: f.SR_fitness(X, y)                                                              # noqa: E731
    (loss, g), (loss_n, normal) = grad(), neq()
    fit()
    torch.cuda.synchronize()
    tg, tn, tf = [], [], []
    for _ in range(args.rounds):                 # alternating, same process
        tg.append(timed(grad, args.reps))
        tn.append(timed(neq, args.reps))
        tf.append(timed(fit, args.reps))
    # the step launches (propose only: the state is left as it is)
    cand = torch.empty_like(value)
    v2 = value.clone()
    h = torch.full((args.pop,), 0.1, device=dev)
    lam = torch.full((args.pop,), 1e-3, device=dev)
    d_step = lambda: torch.ops.evogp_hip.tree_SR_const_step(2, 1, v2, ntype, size, cand, loss, g, loss, g, h)            # noqa: E731
    l_step = lambda: torch.ops.evogp_hip.tree_SR_lm_step(2, v2, ntype, size, cand, loss_n, normal, loss_n, normal, lam)  # noqa: E731
    d_step(), l_step()
    torch.cuda.synchronize()
    td, tl = timed(d_step, args.reps), timed(l_step, args.reps)
    nodes = int(f.batch_subtree_size[:, 0].clamp(min=0).sum())
    nconst = ((ntype == 1) & (torch.arange(64, device=dev)[None, :] < size[:, :1])).sum(1)
    result = {"device": torch.cuda.get_device_name(0), "pop": args.pop, "rows": 1024, "var_len": 10, "gp_len": 64, "live_nodes": nodes,
              "mean_constants": float(nconst.float().mean()), "share_more_than_8_constants": float((nconst > 8).float().mean()),
              "fitness_ms": min(tf), "gradient_ms": min(tg), "normal_eq_ms": min(tn), "normal_eq_over_gradient": min(tn) / min(tg),
              "gradient_ms_all": tg, "normal_eq_ms_all": tn,
              "descent_step_ms": td, "lm_step_ms": tl}
    before = loss.clone()
    fin0 = torch.isfinite(before)
    # the two kernels sum the squared residuals in the same order: the same loss bits wherever the loss is a number
    result["loss_bits_equal_gradient"] = bool(torch.equal(torch.isnan(loss), torch.isnan(loss_n)) and
                                              torch.equal(loss[~torch.isnan(loss)].view(torch.int32), loss_n[~torch.isnan(loss)].view(torch.int32)))
    result["median_loss_before"] = float(before[fin0].median())
    curves = {}
    for method in ("descent", "lm"):
        curves[method] = {}
        for steps in (1, 2, 5, 10):
            _, after = f.optimize_constants(X, y, steps=steps, method=method)
            fin = fin0 & torch.isfinite(after)
            curves[method][str(steps)] = {"median_loss": float(after[fin].median()), "improved_share": float((after[fin] < before[fin]).float().mean())}
        f.optimize_constants(X, y, steps=10, method=method)
        torch.cuda.synchronize()
        curves[method]["ms_10_steps"] = timed(lambda: f.optimize_constants(X, y, steps=10, method=method), 2)
    result["after_steps"] = curves
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
