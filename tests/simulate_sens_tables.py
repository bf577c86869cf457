"""TEST-ONLY: the rows of evogp_hip::tree_SR_simulation_sensitivities and evogp_hip::tree_SR_simulation_normal_eq
(csrc/sr_simulate_sens.hip) in the forest-invariance table (tests/forest_invariance.py) and in the binding-contract table
(tests/test_gpu_binding_contract.py), on tests/simulate_tables.py's reading of the table's cases as simulations.  Imported by
tests/test_simulate_sens_ref.py and tests/test_gpu_simulate_sens.py, so the rows exist under ``-m gpu`` and ``-m "not gpu"`` alike."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forest_invariance as FI  # noqa: E402
import simulate_tables as ST  # noqa: E402
import test_gpu_binding_contract as BC  # noqa: E402

SENS, NORMAL = "evogp_hip::tree_SR_simulation_sensitivities", "evogp_hip::tree_SR_simulation_normal_eq"
F32, F64 = torch.float32, torch.float64
B, T = ST.B, ST.T


def _sens(f, s, p, device):
    fd, out = FI._f(f, device), ()
    for scheme, S in ST._systems(s):
        out += FI._o(FI.hip.tree_SR_simulation_sensitivities(*fd, *ST._inputs(s, S, device), scheme, 0.1))
    return out


def _normal(f, s, p, device):
    fd, out = FI._f(f, device), ()
    for scheme, S in ST._systems(s):
        x0, u = ST._inputs(s, S, device)
        SC = 1 if scheme == 3 else S
        target = torch.full((B, T) if scheme == 3 else (B, T, S), 0.75, device=device)
        weight = torch.linspace(0.5, 1.5, SC, device=device)
        out += FI._o(FI.hip.tree_SR_simulation_normal_eq(*fd, x0, u, target, weight, scheme, 0.1))
    return out


FI.TABLE[SENS] = FI._row(_sens, out="any", finite=0)
FI.TABLE[NORMAL] = FI._row(_normal, out="any", finite=0)

ROWS = {
    SENS: lambda: dict(
        args=BC._forest() + [BC._f("x0", BC.D, 1), BC._f("u", BC.D, 3, 1), ("scheme", 2), ("dt", 0.1)],
        outs=[((BC.POP, BC.D, 3, 1), F32), ((BC.POP, BC.D, 3, 1, 8), F32)], scalars={"scheme": (-1, 4)},
        also=[("no inputs", {"u": torch.zeros((BC.D, 3, 0), device="cuda")}, [((BC.POP, BC.D, 3, 1), F32), ((BC.POP, BC.D, 3, 1, 8), F32)])]),
    NORMAL: lambda: dict(
        args=BC._forest() + [BC._f("x0", BC.D, 1), BC._f("u", BC.D, 3, 1), BC._f("target", BC.D, 3, 1), BC._f("state_weight", 1), ("scheme", 1),
                             ("dt", 0.1)],
        outs=[((BC.POP, 1), F64), ((BC.POP,), F32), ((BC.POP, 44), F32)], scalars={"scheme": (-1, 4)},
        also=[("narx", {"x0": BC._f("x0", BC.D, 2)[1], "u": torch.zeros((BC.D, 3, 0), device="cuda"), "target": BC._f("target", BC.D, 3)[1],
                        "scheme": 3}, [((BC.POP, 1), F64), ((BC.POP,), F32), ((BC.POP, 44), F32)])]),
}
BC.TABLE.update(ROWS)
