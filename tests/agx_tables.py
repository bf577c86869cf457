"""TEST-ONLY: the rows of the two midpoint ops (csrc/sr_backprop.hip with MID; approximately geometric semantic crossover) in the
forest-invariance table (tests/forest_invariance.py) and in the binding-contract table (tests/test_gpu_binding_contract.py).  Imported
by tests/test_agx_host.py and tests/test_gpu_agx.py, so the rows exist under ``-m gpu`` and ``-m "not gpu"`` alike (collection imports
every module).  The mates are the case's shared ``donors`` forest (stale tails included), the mate of a tree a per-tree word."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import backprop_tables as BT  # noqa: E402
import forest_invariance as FI  # noqa: E402
import test_gpu_binding_contract as BC  # noqa: E402

DESIRED_MID, AGX_MATCH = "evogp_hip::tree_SR_desired_mid", "evogp_hip::tree_SR_agx_match"


def _mate(s, p):
    return (p["mut_word"] % s["donors"][0].shape[0]).astype(np.int32)


def _head(f, s, p, device):
    return (*FI._f(f, device), *FI._f(s["donors"], device), FI._d(s["X"], device), FI._d(BT._pos(f, p), device), FI._d(_mate(s, p), device))


def _desired_mid(f, s, p, device):
    return FI._o(FI.hip.tree_SR_desired_mid(*_head(f, s, p, device)))


def _agx_match(f, s, p, device):
    return FI._o(FI.hip.tree_SR_agx_match(*_head(f, s, p, device), FI._d(BT._library(s), device)))


FI.TABLE[DESIRED_MID] = FI._row(_desired_mid, cpu=("cpu_agx_ops",))
FI.TABLE[AGX_MATCH] = FI._row(_agx_match, cpu=("cpu_agx_ops",), finite=3)

N_MATES = 3
_MATE_NAMES = ("mate_value", "mate_type", "mate_size")


def _args():
    return (BC._forest() + BC._forest(N_MATES, BC.L, _MATE_NAMES) + [BC._f("variables", BC.D, BC.V), BC._i("pos", BC.POP), BC._i("mate", BC.POP)])


def _mate_faults():
    """a mate forest without a row, and of another row width"""
    return {"mate_value": [("without a row", torch.zeros((0, BC.L))), ("of another width", torch.zeros((N_MATES, BC.L + 1)))]}


def _five_mates():
    return dict(BC._forest(5, BC.L, _MATE_NAMES))


BC.TABLE[DESIRED_MID] = lambda: dict(args=_args(), outs=BT._DESIRED_OUT, tensors=_mate_faults(),
                                     also=[("five mates", _five_mates(), BT._DESIRED_OUT)])
BC.TABLE[AGX_MATCH] = lambda: dict(
    args=_args() + [BC._f("lib", 3, BC.D)], outs=BT._MATCH_OUT,
    tensors={**_mate_faults(), "lib": [("without a row", torch.zeros((0, BC.D))), ("of 1025 rows", torch.zeros((1025, BC.D))),
                                       ("of another D", torch.zeros((3, BC.D + 1)))]},
    also=[("five mates", _five_mates(), BT._MATCH_OUT),
          ("a library of 1024 rows", {"lib": BC._f("lib", 1024, BC.D)[1]}, BT._MATCH_OUT[:1] + [((BC.POP, 1024), torch.float64)] + BT._MATCH_OUT[2:])])
