"""Cost of simulation fitness (csrc/sr_simulate.hip; Forest.SR_simulation_loss) next to the only route a user had before it: Forest.forward
once per (trajectory, step, stage) with the scheme's update in torch between two launches.  Device events around every call after a
warm-up call, medians of --reps repetitions, all in ONE process; writes one JSON object to --out (profiles/simulate_bench.json) and
prints it.  No time is fixed in advance.

A fresh + - * / forest of --pop trees (gp_len 64, S = 2 states, U = 1 input, two outputs), B = 64 trajectories of T = 128 steps; per scheme:
  loss_ms          tree_SR_simulation_loss, the whole call
  stepping_ms      the forward + torch route on --slice trajectories of --slice-steps steps, SCALED by (B T) / (slice trajectories x slice
                   steps): the route's launches are the same at every (b, t), so the scaling is a multiplication; `scaled` says so
  ns_per_eval      loss_ms over pop x B x T x stages tree evaluations
and once, on the same trees read as single-output trees over D = B T rows:
  scaling_ms       tree_SR_linear_scaling, and its ns per tree evaluation: the same interpreter without the dependent chain
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

S, U, B, T = 2, 1, 64, 128
STAGES = {"map": 1, "euler": 1, "rk4": 4}


def stepping(forest, x0, u, scheme, dt):
    """the route that exists: one forward launch per (trajectory, step, stage), the update in torch"""
    pop = forest.pop_size
    h2, h6 = dt * 0.5, dt / 6.0
    for b in range(x0.shape[0]):
        x = x0[b].expand(pop, S).contiguous()
        for t in range(u.shape[1]):
            ub = u[b, t].expand(pop, U)
            f = lambda s: forest.forward(torch.cat([s, ub], 1))  # noqa: E731
            if scheme == "map":
                x = f(x)
            elif scheme == "euler":
                x = x + dt * f(x)
            else:
                k1 = f(x)
                k2 = f(x + h2 * k1)
                k3 = f(x + h2 * k2)
                k4 = f(x + dt * k3)
                x = x + h6 * (((k1 + 2 * k2) + 2 * k3) + k4)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pop", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--slice", type=int, default=2)
    ap.add_argument("--slice-steps", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simulate_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_simulate.py measures on the device: no GPU found")
    from evogp_amd.tree import Forest, GenerateDescriptor
    keys = torch.tensor([1, 2], dtype=torch.uint32, device="cuda")
    desc = dict(max_tree_len=64, input_len=S + U, using_funcs=["+", "-", "*", "/"], max_layer_cnt=5, const_samples=[-1, 0, 1, 2])
    forest = Forest.random_generate(args.pop, GenerateDescriptor(output_len=S, **desc), keys=keys)
    single = Forest.random_generate(args.pop, GenerateDescriptor(output_len=1, **desc), keys=keys)
    g = torch.Generator(device="cuda").manual_seed(3)
    x0 = torch.rand((B, S), device="cuda", generator=g) + 0.5
    u = torch.rand((B, T, U), device="cuda", generator=g) + 0.5
    target = torch.rand((B, T, S), device="cuda", generator=g) + 0.5
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "pop": args.pop, "states": S, "inputs": U, "trajectories": B,
              "steps": T, "schemes": {}}
    for scheme, stages in STAGES.items():
        loss = times(lambda: forest.SR_simulation_loss(x0, u, target, scheme, 0.01), args.reps)
        step = times(lambda: stepping(forest, x0[:args.slice], u[:args.slice, :args.slice_steps], scheme, 0.01), max(2, args.reps // 3))
        scale = (B * T) / (args.slice * args.slice_steps)
        alive = int(torch.isfinite(forest.SR_simulation_loss(x0, u, target, scheme, 0.01)).all(1).sum())
        result["schemes"][scheme] = {
            "loss_ms": loss, "stepping_ms": {k: v * scale for k, v in step.items()}, "scaled": f"x{scale:g} from {args.slice} trajectories of {args.slice_steps} steps",
            "ns_per_eval": loss["median"] * 1e6 / (args.pop * B * T * stages), "trees_alive": alive}
        print(f"# {scheme}: loss {loss['median']:.3f} ms, stepping (scaled) {step['median'] * scale:.1f} ms, {alive} trees alive", file=sys.stderr, flush=True)
    X = torch.rand((B * T, S + U), device="cuda", generator=g) + 0.5
    y = torch.rand((B * T, 1), device="cuda", generator=g)
    v, t, s = single._tensors()
    scaling = times(lambda: torch.ops.evogp_hip.tree_SR_linear_scaling(args.pop, B * T, 64, S + U, 1, v, t, s, X, y), args.reps)
    one = times(lambda: single.SR_simulation_loss(x0[:, :1], u.expand(B, T, 2).contiguous(), target[:, :, :1].contiguous(), "map", 0.01), args.reps)
    result["scaling_ms"] = scaling
    result["scaling_ns_per_eval"] = scaling["median"] * 1e6 / (args.pop * B * T)
    result["single_output_map_ms"] = one
    result["single_output_map_ns_per_eval"] = one["median"] * 1e6 / (args.pop * B * T)
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
