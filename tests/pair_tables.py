"""TEST-ONLY: the row of evogp_hip::tree_SR_pair_moments (csrc/sr_pair.hip) in the forest-invariance table (tests/forest_invariance.py)
and in the binding-contract table (tests/test_gpu_binding_contract.py).  Imported by tests/test_pair_host.py and tests/test_gpu_pairs.py,
so the rows exist under ``-m gpu`` and ``-m "not gpu"`` alike (collection imports every module).

The op is indexed by EVENTS, so the events of a case are built from tree indices and the invariants are stated per tree: event t has tree
t as its first tree, once against three fixed trees of the case's shared donor forest (another population, with labels) and once against
itself (no mates forest, no labels).  Row t of every output is then a function of tree t, the donors and the dataset: no word of it may
depend on a dead word, on the order of the rows or on the population the tree stands in."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forest_invariance as FI  # noqa: E402
import test_gpu_binding_contract as BC  # noqa: E402

PAIRS = "evogp_hip::tree_SR_pair_moments"
F64 = torch.float64


def _pairs(f, s, p, device):
    fd, X, y = FI._f(f, device), FI._d(s["X"], device), FI._d(s["y1"], device)
    donors = FI._f(s["donors"], device)
    pop, nd = f[0].shape[0], s["donors"][0].shape[0]
    t = torch.arange(pop, dtype=torch.int32, device=device)
    against = torch.tensor([0, nd // 2, nd - 1], dtype=torch.int32, device=device)[None, :].expand(pop, 3).contiguous()
    own, mom = FI.hip.tree_SR_pair_moments(*fd, *donors, X, y, t, against)
    own0, self_ = FI.hip.tree_SR_pair_moments(*fd, *fd, X, None, t, t[:, None].contiguous())
    return FI._o((own, mom, own0, self_))


FI.TABLE[PAIRS] = FI._row(_pairs, cpu=("cpu_pair_ops",), finite=0)

ROWS = {
    PAIRS: lambda: dict(
        args=BC._forest() + BC._forest(3, 16, ("mate_value", "mate_type", "mate_size"))
        + [BC._f("variables", BC.D, BC.V), BC._f("labels", BC.D), BC._i("first", 5), BC._i("candidates", 5, 2)],
        outs=[((5,), F64), ((5, 2, 3), F64)],
        also=[("no labels", {"labels": None}, [((5,), F64), ((5, 2, 3), F64)]),
              ("no events", {"first": BC._i("first", 0)[1], "candidates": BC._i("candidates", 0, 2)[1]}, [((0,), F64), ((0, 2, 3), F64)])]),
}
BC.TABLE.update(ROWS)
