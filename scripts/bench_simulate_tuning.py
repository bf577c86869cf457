"""Cost of the Gauss-Newton model under simulation fitness (csrc/sr_simulate_sens.hip; Forest.SR_simulation_normal_equations) next to the
fitness it models (Forest.SR_simulation_loss) on the SAME forest and shape, and of three Levenberg-Marquardt steps end to end
(Forest.optimize_simulation_constants).  One warm-up call, medians of --reps repetitions, all in ONE process; writes one JSON object to
--out (profiles/simulate_tuning_bench.json).  --resources FILE also writes the compiler's resource report of the kernel file
(profiles/simulate_tuning_resources.txt; needs hipcc, no GPU).

  loss_ms          tree_SR_simulation_loss, the whole call
  normal_eq_ms     tree_SR_simulation_normal_eq, the whole call; ratio = normal_eq / loss (expected about 1 + 3 ceil(nc / 4) interpretations' worth)
  tune3_ms         optimize_simulation_constants(steps=3): four evaluations and four step launches
"""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

S, U, B, T = 2, 1, 64, 128


def resources(path):
    """the compiler's report of csrc/sr_simulate_sens.hip, one line per kernel"""
    csrc = os.path.join(ROOT, "evogp_amd", "csrc")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-mllvm",
           "-structurizecfg-skip-uniform-regions=true", "-Rpass-analysis=kernel-resource-usage", "-c", "sr_simulate_sens.hip", "-o", os.devnull]
    log = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True, check=True).stderr
    demangle = lambda n: subprocess.run(["c++filt", n], capture_output=True, text=True).stdout.strip() or n  # noqa: E731
    field = lambda block, name: re.search(name + r"[^:]*: (\d+)", block).group(1)  # noqa: E731
    lines = ["csrc/sr_simulate_sens.hip, hipcc --offload-arch=gfx950 -O3 -ffp-contract=off with the flags of the Makefile's UNI_SRCS group "
             "(-Rpass-analysis=kernel-resource-usage).",
             "sr_sim_sens_kernel<VL, KIND, BUILD>: VL words of the [state | u] tuple; KIND 0 one state, 1 several states, 2 narx; BUILD 0 LEAN, "
             "1 FULL (4 tangents per interpretation), 2 DEEP (1 tangent, the stack in the workspace).", ""]
    for block in log.split("Function Name: ")[1:]:
        name = demangle(block.split()[0]).split("(")[0].replace("void evogp::", "")
        lines.append(f"{name:<48} VGPR {field(block, 'VGPRs'):>3} AGPR {field(block, 'AGPRs'):>3} scratch {field(block, 'ScratchSize'):>5} B/lane  "
                     f"waves/SIMD {field(block, 'Occupancy')}  LDS {field(block, 'LDS Size'):>5} B")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pop", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simulate_tuning_bench.json"))
    ap.add_argument("--resources", default=None)
    args = ap.parse_args()
    if args.resources:
        resources(args.resources)
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_simulate_tuning.py measures on the device: no GPU found")
    from bench_semantics import times
    from evogp_amd.tree import Forest, GenerateDescriptor
    keys = torch.tensor([1, 2], dtype=torch.uint32, device="cuda")
    desc = GenerateDescriptor(max_tree_len=64, input_len=S + U, output_len=S, using_funcs=["+", "-", "*", "/"], max_layer_cnt=5,
                              const_samples=[-1, 0, 1, 2])
    forest = Forest.random_generate(args.pop, desc, keys=keys)
    g = torch.Generator(device="cuda").manual_seed(3)
    x0 = torch.rand((B, S), device="cuda", generator=g) + 0.5
    u = torch.rand((B, T, U), device="cuda", generator=g) + 0.5
    target = torch.rand((B, T, S), device="cuda", generator=g) + 0.5
    nc = (forest.SR_simulation_sensitivities(x0[:1], u[:1, :1], scheme="map")[2] >= 0).sum(1).float()
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "pop": args.pop, "states": S, "inputs": U, "trajectories": B,
              "steps": T, "mean_constants": float(nc.mean()), "mean_passes": float(torch.ceil(nc / 4).mean()), "schemes": {}}
    for scheme in ("map", "euler", "rk4"):
        loss = times(lambda: forest.SR_simulation_loss(x0, u, target, scheme, 0.01), args.reps)
        normal = times(lambda: forest.SR_simulation_normal_equations(x0, u, target, scheme, 0.01), args.reps)
        tune = times(lambda: forest.optimize_simulation_constants(x0, u, target, scheme, 0.01, steps=3), args.reps)
        result["schemes"][scheme] = {"loss_ms": loss, "normal_eq_ms": normal, "ratio": normal["median"] / loss["median"], "tune3_ms": tune}
        print(f"# {scheme}: loss {loss['median']:.3f} ms, normal equations {normal['median']:.3f} ms, 3 LM steps {tune['median']:.1f} ms",
              file=sys.stderr, flush=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
