"""TEST-ONLY: the rows of the two input-gradient ops (csrc/sr_xgrad.hip) in the forest-invariance table (tests/forest_invariance.py) and
in the binding-contract table (tests/test_gpu_binding_contract.py).  Imported by tests/test_input_grad_host.py and
tests/test_gpu_input_grad.py, so the rows exist under ``-m gpu`` and ``-m "not gpu"`` alike (collection imports every module)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forest_invariance as FI  # noqa: E402
import test_gpu_binding_contract as BC  # noqa: E402

GRAD, LOSS = "evogp_hip::tree_SR_input_gradient", "evogp_hip::tree_SR_derivative_loss"


def _wrt(s):
    return [s["var_len"] - 1, 0]   # (not in order)


def _gradient(f, s, p, device):
    return FI._o(FI.hip.tree_SR_input_gradient(*FI._f(f, device), FI._d(s["X"], device), _wrt(s)))


def _loss(f, s, p, device):
    """with labels and finite bounds, then with neither"""
    fd, X, y = FI._f(f, device), FI._d(s["X"], device), FI._d(s["y"], device)
    dy = FI._d(np.stack([-s["X"][:, -1], 3.0 * s["X"][:, 0]], 1).astype(np.float32), device)
    lo, hi = FI._d(np.array([-1.0, 0.0], np.float32), device), FI._d(np.array([0.5, 4.0], np.float32), device)
    return FI._o(FI.hip.tree_SR_derivative_loss(*fd, X, y, dy, _wrt(s), lo, hi)) + FI._o(FI.hip.tree_SR_derivative_loss(*fd, X, y, None, _wrt(s), None, None))


FI.TABLE[GRAD] = FI._row(_gradient, cpu=("cpu_xgrad_ops",), axes=(0, 1), finite=0)
FI.TABLE[LOSS] = FI._row(_loss, cpu=("cpu_xgrad_ops",), finite=0)


def _data():
    return [BC._f("variables", BC.D, BC.V)]


_WRT_FAULTS = ([], [0, 0], [BC.V], [-1], list(range(9)))
_LOSS_OUT = [((BC.POP, 2), BC.F32), ((BC.POP, 1), BC.I32)]
BC.TABLE[GRAD] = lambda: dict(args=BC._forest() + _data() + [("wrt", [1, 0])], outs=[((BC.POP, BC.D), BC.F32), ((2, BC.POP, BC.D), BC.F32)],
                              scalars={"wrt": _WRT_FAULTS}, also=[("one variable", {"wrt": [1]}, [((BC.POP, BC.D), BC.F32), ((1, BC.POP, BC.D), BC.F32)])])
BC.TABLE[LOSS] = lambda: dict(
    args=BC._forest() + _data() + [BC._f("labels", BC.D, 1), BC._f("dlabels", BC.D, 1), ("wrt", [1]), BC._f("dmin", 1), BC._f("dmax", 1)],
    outs=_LOSS_OUT, scalars={"wrt": _WRT_FAULTS},
    also=[("no derivative labels", {"dlabels": None}, _LOSS_OUT), ("no bounds", {"dmin": None, "dmax": None}, _LOSS_OUT),
          ("a lower bound alone", {"dmax": None}, _LOSS_OUT), ("nothing optional", {"dlabels": None, "dmin": None, "dmax": None}, _LOSS_OUT)])
