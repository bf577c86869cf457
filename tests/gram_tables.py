"""TEST-ONLY: the row of evogp_hip::tree_SR_gram (csrc/sr_gram.hip) in the forest-invariance table (tests/forest_invariance.py) and in the
binding-contract table (tests/test_gpu_binding_contract.py).  Imported by tests/test_gram_host.py and tests/test_gpu_gram.py, so the rows
exist under ``-m gpu`` and ``-m "not gpu"`` alike (collection imports every module).

The op's matrix relates every tree to every other, so the invariants are stated on what belongs to ONE tree: with index = every tree,
the diagonal of G, the lin words and the usable flag, with residuals and without labels.  Row t is then a function of tree t and the
dataset: no word of it may depend on a dead word, on the order of the rows or on the population the tree stands in."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forest_invariance as FI  # noqa: E402
import test_gpu_binding_contract as BC  # noqa: E402

GRAM = "evogp_hip::tree_SR_gram"
F64 = torch.float64


def _gram(f, s, p, device):
    fd, X, y = FI._f(f, device), FI._d(s["X"], device), FI._d(s["y1"], device)
    t = torch.arange(f[0].shape[0], dtype=torch.int32, device=device)
    G, lin, usable = FI.hip.tree_SR_gram(*fd, X, y, t, True)
    G0, lin0, _ = FI.hip.tree_SR_gram(*fd, X, None, t, False)
    return FI._o((torch.diagonal(G).contiguous(), lin, usable, torch.diagonal(G0).contiguous(), lin0))


FI.TABLE[GRAM] = FI._row(_gram, finite=0)

ROWS = {
    GRAM: lambda: dict(
        args=BC._forest() + [BC._f("variables", BC.D, BC.V), BC._f("labels", BC.D), BC._i("index", 5), ("residuals", True)],
        outs=[((5, 5), F64), ((5, 2), F64), ((5,), torch.bool)],
        also=[("no labels", {"labels": None, "residuals": False}, [((5, 5), F64), ((5, 2), F64), ((5,), torch.bool)]),
              ("no trees", {"index": BC._i("index", 0)[1]}, [((0, 0), F64), ((0, 2), F64), ((0,), torch.bool)])]),
}
BC.TABLE.update(ROWS)
