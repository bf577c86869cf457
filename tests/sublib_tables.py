"""TEST-ONLY: the rows of evogp_hip::tree_SR_subtree_signatures and evogp_hip::subtree_library_select (csrc/sr_subtree_sig.hip) in the
forest-invariance table (tests/forest_invariance.py) and in the binding-contract table (tests/test_gpu_binding_contract.py).  Imported by
tests/test_sublib_host.py and tests/test_gpu_sublib.py, so the rows exist under ``-m gpu`` and ``-m "not gpu"`` alike (collection imports
every module).  The signatures are a per-tree op: no word of an output row may depend on a dead word, on the order of the rows or on the
population the tree stands in, malformed rows and stale tails included.  The selection takes no forest."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forest_invariance as FI  # noqa: E402
import test_gpu_binding_contract as BC  # noqa: E402

SIGNATURES = "evogp_hip::tree_SR_subtree_signatures"
SELECT = "evogp_hip::subtree_library_select"

FI.TABLE[SIGNATURES] = FI._row(FI._data_op(FI.hip.tree_SR_subtree_signatures, y=None), cpu=("cpu_sublib_ops",))
FI.EXEMPT[SELECT] = "takes no forest: a matrix of signatures and one of sizes"

K = 5
ROWS = {
    SIGNATURES: lambda: dict(args=BC._data_head(use_mse=False) + BC._forest() + [BC._f("variables", BC.D, BC.V)],
                             outs=[((BC.POP, BC.L), BC.I64)], scalars=dict(BC.SIZES, out_len=(2,))),
    SELECT: lambda: dict(
        args=[("sig", torch.ones((BC.POP, BC.L), dtype=BC.I64, device="cuda")), ("size", torch.ones((BC.POP, BC.L), dtype=BC.I16, device="cuda")),
              ("min_size", 1), ("max_size", BC.L), ("k", K)],
        outs=[((K,), BC.I32), ((K,), BC.I32), ((1,), BC.I32)], scalars={"k": (0, 1025), "min_size": (0,), "max_size": (0,)},
        tensors={"size": [("of another shape", torch.ones((BC.POP, BC.L + 1), dtype=BC.I16))]},
        also=[("the largest k", {"k": 1024}, [((1024,), BC.I32), ((1024,), BC.I32), ((1,), BC.I32)])]),
}
BC.TABLE.update(ROWS)
