"""TEST-ONLY: the rows of the two rank ops (csrc/sr_rank.hip) in the forest-invariance and binding-contract tables, whose coverage tests want
every registered op listed; imported by both rank test modules.  Two segments, a small payload: tree t's outputs depend on tree t alone."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forest_invariance as FI  # noqa: E402
import test_gpu_binding_contract as BC  # noqa: E402

RANK, ROWS_OP = "evogp_hip::tree_SR_rank_stats", "evogp_hip::rank_rows"
F64, I64 = torch.float64, torch.int64


def _rank(f, s, p, device):
    D = s["D"]
    seg = FI._d(np.array([0, D // 3, D], np.int32), device)
    payload = FI._d((np.arange(D) % 7).astype(np.int32), device)
    return FI._o(FI.hip.tree_SR_rank_stats(*FI._f(f, device), FI._d(s["X"], device), payload, seg, D - D // 3, 0, True, True, True))


FI.TABLE[RANK] = FI._row(_rank)
FI.EXEMPT[ROWS_OP] = "takes no forest: a vector of labels"
_seg = lambda: ("seg_start", torch.tensor([0, 3, BC.D], dtype=torch.int32, device="cuda"))  # noqa: E731
ROWS = {
    RANK: lambda: dict(
        args=BC._forest() + [BC._f("variables", BC.D, BC.V), BC._i("payload", BC.D), _seg(), ("max_segment", 5), ("metric", 1),
                             ("want_words", True), ("want_fused", True), ("want_scores", True)],
        outs=[((BC.POP, 2, 2), I64), ((BC.POP, 3), F64), ((BC.POP, 2), F64), ((BC.POP,), BC.U8)],
        scalars={"max_segment": (0, 9, 8193), "metric": (2, -1)}),
    ROWS_OP: lambda: dict(args=[BC._f("values", BC.D), BC._i("payload", BC.D), _seg(), ("max_segment", 5)],
                          outs=[((BC.D,), BC.I32), ((2, 2), I64), ((2,), BC.I32)], scalars={"max_segment": (0, 9)}),
}
BC.TABLE.update(ROWS)
