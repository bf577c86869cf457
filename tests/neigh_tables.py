"""TEST-ONLY: the row of evogp_hip::tree_SR_neighbours (csrc/sr_neigh.hip) in the forest-invariance table (tests/forest_invariance.py) and in
the binding-contract table (tests/test_gpu_binding_contract.py).  Imported by tests/test_neigh_host.py and tests/test_gpu_neigh.py, so the
rows exist under ``-m gpu`` and ``-m "not gpu"`` alike (collection imports every module).

A tree's neighbours are other trees, so the invariants are stated on what belongs to ONE tree: with index = every tree, ``norm`` and
``usable``; and ``dist2``, ``neighbour`` and ``count`` of a call on the tree ALONE (no neighbour: +inf, -1 and 0, or NaN, -1 and 0)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forest_invariance as FI  # noqa: E402
import test_gpu_binding_contract as BC  # noqa: E402

NEIGH = "evogp_hip::tree_SR_neighbours"
F64, I32 = torch.float64, torch.int32
BC.WRONG.setdefault(F64, torch.float32)   # (the first op with a float64 input)


def _neigh(f, s, p, device):
    fd, X = FI._f(f, device), FI._d(s["X"], device)
    t = torch.arange(f[0].shape[0], dtype=I32, device=device)
    r2 = torch.tensor([1.0], dtype=F64, device=device)
    norm, usable = FI.hip.tree_SR_neighbours(*fd, X, t, 3, r2)[3:]
    alone = [FI.hip.tree_SR_neighbours(*fd, X, t[i:i + 1], 3, r2)[:3] for i in range(t.numel())]
    return FI._o((norm, usable) + tuple(torch.cat(c) for c in zip(*alone)))


FI.TABLE[NEIGH] = FI._row(_neigh, finite=0)


def _outs(n, k, r):
    return [((n, k), F64), ((n, k), I32), ((n, r), I32), ((n,), F64), ((n,), torch.bool)]


ROWS = {
    NEIGH: lambda: dict(
        args=BC._forest() + [BC._f("variables", BC.D, BC.V), BC._i("index", 5), ("k", 3), ("radius2", torch.full((2,), 0.5, dtype=F64, device="cuda"))],
        outs=_outs(5, 3, 2), scalars={"k": (0, 17)},
        also=[("no radii", {"radius2": torch.zeros(0, dtype=F64, device="cuda")}, _outs(5, 3, 0)),
              ("no trees", {"index": BC._i("index", 0)[1]}, _outs(0, 3, 2))]),
}
BC.TABLE.update(ROWS)
