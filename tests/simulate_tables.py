"""TEST-ONLY: the rows of evogp_hip::tree_SR_simulate and evogp_hip::tree_SR_simulation_loss (csrc/sr_simulate.hip) in the
forest-invariance table (tests/forest_invariance.py) and in the binding-contract table (tests/test_gpu_binding_contract.py).  Imported by
tests/test_simulate_ref.py and tests/test_gpu_simulate.py, so the rows exist under ``-m gpu`` and ``-m "not gpu"`` alike.

The adapter reads the table's cases as simulations: a single-output forest is a one-state law (rk4) and a NARX forecaster of two lags, a
forest of 4 outputs on 3 variables a 4-state autonomous system.  The ops take at most 32 variables: the forest of 40 is simulated with 32
(an index past them reads the last one, as every kernel clamps it).  70 trajectories (a full tile and a ragged one) of 3 steps."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forest_invariance as FI  # noqa: E402
import test_gpu_binding_contract as BC  # noqa: E402

SIMULATE, LOSS = "evogp_hip::tree_SR_simulate", "evogp_hip::tree_SR_simulation_loss"
F64 = torch.float64
B, T = 70, 3


def _systems(s):
    v = min(s["var_len"], 32)
    return [(0, s["out_len"]), (2, s["out_len"])] if s["out_len"] > 1 else [(2, 1), (3, 2 if v > 2 else 1)]


def _inputs(s, S, device):
    X = s["X"]
    v = max(min(s["var_len"], 32), S)
    U = v - S
    rows = (np.arange(B)[:, None] + np.arange(T)[None, :]) % len(X)
    x0 = np.ascontiguousarray(np.resize(X[:B, :min(S, X.shape[1])], (B, S)))
    u = np.ascontiguousarray(X[rows][:, :, X.shape[1] - U:] if U else np.zeros((B, T, 0), np.float32))
    return FI._d(x0, device), FI._d(u, device)


def _simulate(f, s, p, device):
    fd, out = FI._f(f, device), ()
    for scheme, S in _systems(s):
        out += FI._o(FI.hip.tree_SR_simulate(*fd, *_inputs(s, S, device), scheme, 0.1))
    return out


def _loss(f, s, p, device):
    fd, out = FI._f(f, device), ()
    for scheme, S in _systems(s):
        x0, u = _inputs(s, S, device)
        target = torch.full((B, T) if scheme == 3 else (B, T, S), 0.75, device=device)
        out += FI._o(FI.hip.tree_SR_simulation_loss(*fd, x0, u, target, scheme, 0.1))
    return out


FI.TABLE[SIMULATE] = FI._row(_simulate, out="any", finite=0)
FI.TABLE[LOSS] = FI._row(_loss, out="any", finite=0)

ROWS = {
    SIMULATE: lambda: dict(
        args=BC._forest() + [BC._f("x0", BC.D, 1), BC._f("u", BC.D, 3, 1), ("scheme", 2), ("dt", 0.1)],
        outs=[((BC.POP, BC.D, 3, 1), BC.F32)], scalars={"scheme": (-1, 4)},
        also=[("no inputs", {"u": torch.zeros((BC.D, 3, 0), device="cuda")}, [((BC.POP, BC.D, 3, 1), BC.F32)])]),
    LOSS: lambda: dict(
        args=BC._forest() + [BC._f("x0", BC.D, 1), BC._f("u", BC.D, 3, 1), BC._f("target", BC.D, 3, 1), ("scheme", 1), ("dt", 0.1)],
        outs=[((BC.POP, 1), F64)], scalars={"scheme": (-1, 4)},
        also=[("narx", {"x0": BC._f("x0", BC.D, 2)[1], "u": torch.zeros((BC.D, 3, 0), device="cuda"), "target": BC._f("target", BC.D, 3)[1],
                        "scheme": 3}, [((BC.POP, 1), F64)])]),
}
BC.TABLE.update(ROWS)
