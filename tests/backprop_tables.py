"""TEST-ONLY: the rows of the two semantic-backpropagation ops (csrc/sr_backprop.hip) in the forest-invariance table
(tests/forest_invariance.py) and in the binding-contract table (tests/test_gpu_binding_contract.py).  Imported by
tests/test_backprop_host.py and tests/test_gpu_backprop.py, so the rows exist under ``-m gpu`` and ``-m "not gpu"`` alike (collection
imports every module)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forest_invariance as FI  # noqa: E402
import test_gpu_binding_contract as BC  # noqa: E402

DESIRED, MATCH = "evogp_hip::tree_SR_desired", "evogp_hip::tree_SR_backprop_match"


def _pos(f, p):
    """a node of every tree from its raw word; every other tree the root (whose rows are all REQUIRED)"""
    pos = FI._node(p["mut_word"], f[2])
    return np.where((p["mut_word"] % 2 == 0) & (pos >= 0), 0, pos).astype(np.int32)


def _library(s):
    """the variables, a product, the labels and a row that is not finite"""
    X = s["X"]
    bad = X[:, 0].copy()
    bad[::7] = np.inf
    return np.ascontiguousarray(np.concatenate([X.T, (X[:, 0] * X[:, -1])[None], s["y"].T, bad[None]]).astype(np.float32))


def _desired(f, s, p, device):
    return FI._o(FI.hip.tree_SR_desired(*FI._f(f, device), FI._d(s["X"], device), FI._d(s["y"], device), FI._d(_pos(f, p), device)))


def _match(f, s, p, device):
    return FI._o(FI.hip.tree_SR_backprop_match(*FI._f(f, device), FI._d(s["X"], device), FI._d(s["y"], device), FI._d(_pos(f, p), device),
                                               FI._d(_library(s), device)))


FI.TABLE[DESIRED] = FI._row(_desired, cpu=("cpu_backprop_ops",))
FI.TABLE[MATCH] = FI._row(_match, cpu=("cpu_backprop_ops",), finite=3)


def _args():
    return BC._forest() + [BC._f("variables", BC.D, BC.V), BC._f("labels", BC.D, 1), BC._i("pos", BC.POP)]


_DESIRED_OUT = [((BC.POP, BC.D), BC.F32), ((BC.POP, BC.D), BC.U8), ((BC.POP,), BC.I32)]
_MATCH_OUT = [((BC.POP,), BC.I32), ((BC.POP, 3), torch.float64), ((BC.POP,), BC.F32), ((BC.POP,), torch.float64), ((BC.POP, 3), BC.I32),
              ((BC.POP,), BC.I32)]


def _flat_labels():
    return {"labels": BC._f("labels", BC.D)[1]}


BC.TABLE[DESIRED] = lambda: dict(args=_args(), outs=_DESIRED_OUT, also=[("labels of shape (D,)", _flat_labels(), _DESIRED_OUT)])
BC.TABLE[MATCH] = lambda: dict(
    args=_args() + [BC._f("lib", 3, BC.D)], outs=_MATCH_OUT,
    tensors={"lib": [("without a row", torch.zeros((0, BC.D))), ("of 1025 rows", torch.zeros((1025, BC.D))), ("of another D", torch.zeros((3, BC.D + 1)))]},
    also=[("labels of shape (D,)", _flat_labels(), _MATCH_OUT),
          ("a library of 1024 rows", {"lib": BC._f("lib", 1024, BC.D)[1]}, _MATCH_OUT[:1] + [((BC.POP, 1024), torch.float64)] + _MATCH_OUT[2:])])
