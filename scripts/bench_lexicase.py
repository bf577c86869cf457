"""Cost of epsilon-lexicase selection (csrc/lexicase.hip, LexicaseSelection) at configs[1]'s size, stage by stage: the per-case errors
(tree_SR_case_errors), epsilon (lexicase_epsilon, torch.nanmedian), the clone classes, the first pools and the events
(evogp_hip_debug_lexicase stops the call after a stage; the differences of the timed calls are the stages).  Counts from the same hook:
clone classes, first-pool sizes, steps per event.  Context: TournamentSelection's counter-based launch and tree_SR_fitness on the same
forest.  Device events around each call after warm-up; prints one JSON object (and writes it to --out when given).

  fresh      100 k trees x 1024 rows, 10 variables, gp_len 64, + - * / (BASELINE configs[1]), Forest.random_generate
  evolved    the same forest after 30 generations under LexicaseSelection (DefaultCrossover, DefaultMutation 0.2)
  zero       Forest.zero_generate: one clone class
  down10     the fresh forest, downsample_rate 0.1 (102 rows)
  headline   1 M trees x 1024 rows, fresh (--headline)
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def dataset(device):
    rng = np.random.default_rng(1234)
    X = rng.uniform(-5, 5, (1024, 10)).astype(np.float32)
    y = (X[:, 0] * X[:, 1] + X[:, 2] * X[:, 3] - X[:, 4] + 0.5 * X[:, 5] ** 2).astype(np.float32)[:, None]
    return torch.from_numpy(X).to(device), torch.from_numpy(y).to(device)


def timed(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    fn()
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def measure(forest, X, y, reps, rate=1.0):
    from evogp_amd import _lib
    from evogp_amd.algorithm import LexicaseSelection, lexicase_epsilon

    L = _lib.lib
    pop = forest.pop_size
    sel = LexicaseSelection(X, y, downsample_rate=rate)
    rows = sel.rows(X.shape[0], X.device)
    Xs, ys = (X, y) if rows is None else (X[rows], y[rows])
    errors = forest.SR_case_errors(Xs, ys, use_MSE=False)
    E = errors.t().contiguous()
    eps = lexicase_epsilon(errors)
    select = lambda: torch.ops.evogp_hip.lexicase_select(E, eps, pop, sel.seed, 0)   # noqa: E731
    out = {"rows": int(E.shape[0])}
    out["case_errors_ms"] = timed(lambda: forest.SR_case_errors(Xs, ys, use_MSE=False), reps)
    out["epsilon_ms"] = timed(lambda: lexicase_epsilon(errors), reps)
    t = []
    for stop in (1, 2, 0):
        assert L.evogp_hip_debug_lexicase(None, stop) == 0
        t.append(timed(select, reps))
    out["classes_ms"], out["prep_ms"], out["events_ms"] = t[0], t[1] - t[0], t[2] - t[1]
    out["select_ms"] = t[2]
    counters = torch.zeros(8, dtype=torch.int64, device=X.device)
    assert L.evogp_hip_debug_lexicase(ctypes.c_void_p(counters.data_ptr()), 0) == 0
    select()
    torch.cuda.synchronize()
    assert L.evogp_hip_debug_lexicase(None, 0) == 0
    c = counters.cpu().tolist()
    out.update(classes=c[4], first_pool_mean=c[2] / max(c[5], 1), first_pool_max=c[3], steps_per_event=c[0] / max(c[1], 1))
    out["operator_ms"] = timed(lambda: sel(forest, torch.zeros(pop, device=X.device)), reps)   # errors + eps + select, whole call
    # context on the same forest
    fit = -forest.SR_fitness(X, y)
    out["sr_fitness_ms"] = timed(lambda: forest.SR_fitness(X, y), reps)
    out["tournament7_ms"] = timed(lambda: torch.ops.evogp_hip.tournament_select(fit, pop, 7, 1, 0), reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--generations", type=int, default=30)
    ap.add_argument("--headline", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from evogp_amd.algorithm import DefaultCrossover, DefaultMutation, GeneticProgramming, LexicaseSelection
    from evogp_amd.tree import Forest, GenerateDescriptor

    dev = torch.device("cuda:0")
    X, y = dataset(dev)
    desc = GenerateDescriptor(max_tree_len=64, input_len=10, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=6,
                              const_samples=[-1, 0, 1])
    keys = torch.tensor([42, 0], dtype=torch.uint32, device=dev)
    result = {"device": torch.cuda.get_device_name(0), "pop": 100_000, "rows": 1024, "gp_len": 64, "epsilon": "auto (MAD)",
              "loss": "absolute", "events": "pop"}
    fresh = Forest.random_generate(100_000, desc, keys=keys)
    result["fresh"] = measure(fresh, X, y, args.reps)
    result["down10"] = measure(fresh, X, y, args.reps, rate=0.1)
    result["zero"] = measure(Forest.zero_generate(100_000, 64, 10, 1), X, y, args.reps)
    torch.manual_seed(0)
    algo = GeneticProgramming(fresh, DefaultCrossover(), DefaultMutation(0.2, desc), LexicaseSelection(X, y))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(args.generations):
        algo.step(-algo.forest.SR_fitness(X, y))
    ev[1].record()
    ev[1].synchronize()
    result["generation_ms"] = ev[0].elapsed_time(ev[1]) / max(args.generations, 1)
    result["evolved"] = measure(algo.forest, X, y, args.reps)
    result["evolved"]["generations"] = args.generations
    if args.headline:
        del algo, fresh
        torch.cuda.empty_cache()
        big = Forest.random_generate(1_000_000, desc, keys=keys)
        result["headline"] = measure(big, X, y, max(1, args.reps // 2))
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
