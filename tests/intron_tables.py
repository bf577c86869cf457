"""TEST-ONLY: the rows of evogp_hip::tree_SR_subtree_introns and evogp_hip::tree_remove_introns (csrc/sr_introns.hip) in the
forest-invariance table (tests/forest_invariance.py) and in the binding-contract table (tests/test_gpu_binding_contract.py).  Imported by
tests/test_intron_host.py and tests/test_gpu_introns.py, so the rows exist under ``-m gpu`` and ``-m "not gpu"`` alike (collection imports
every module).  The intron op is a per-tree op whose call computes the signatures inside, as the semantic classes compute their hash: no
word of an output row may depend on a dead word, on the order of the rows or on the population the tree stands in.  The rewrite is a
rewriter with zero tails that copies malformed rows; its call derives ``rep`` through the first op on the case's X."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forest_invariance as FI  # noqa: E402
import test_gpu_binding_contract as BC  # noqa: E402

INTRONS = "evogp_hip::tree_SR_subtree_introns"
REWRITE = "evogp_hip::tree_remove_introns"


def _rep(f, s, device):
    fd, X = FI._f(f, device), FI._d(s["X"], device)
    sig = FI.hip.tree_SR_subtree_signatures(*FI._head(f, s), *fd, X)
    return fd, FI.hip.tree_SR_subtree_introns(*FI._head(f, s), *fd, X, sig)


def _introns(f, s, p, device):
    return FI._o(_rep(f, s, device)[1])


def _remove(f, s, p, device):
    fd, rep = _rep(f, s, device)
    return FI._o(FI.hip.tree_remove_introns(*fd, rep))


FI.TABLE[INTRONS] = FI._row(_introns, cpu=("cpu_intron_ops",))
FI.TABLE[REWRITE] = FI._row(_remove, "rewriter", cpu=("cpu_intron_ops",), tails=FI.ZERO3, copied=FI._malformed_rows,
                            cite=FI.H + ": evogp_hip_remove_introns, '[new_len, gp_len) is zero in all three arrays'; 'A malformed row is "
                            "copied as it is'")

ROWS = {
    INTRONS: lambda: dict(args=BC._data_head(use_mse=False) + BC._forest() + [BC._f("variables", BC.D, BC.V),
                                                                               ("sig", torch.ones((BC.POP, BC.L), dtype=BC.I64, device="cuda"))],
                          outs=[((BC.POP, BC.L), BC.I16)], scalars=dict(BC.SIZES, out_len=(2,))),
    REWRITE: lambda: dict(args=BC._forest() + [("rep", torch.zeros((BC.POP, BC.L), dtype=BC.I16, device="cuda"))],
                          outs=BC.FOREST_OUT + [((BC.POP,), BC.I32)]),
}
BC.TABLE.update(ROWS)
