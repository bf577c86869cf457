"""TEST-ONLY: the rows of evogp_hip::tree_batch_class_stats (csrc/cls_stats.hip) in the forest-invariance table
(tests/forest_invariance.py) and in the binding-contract table (tests/test_gpu_binding_contract.py).  Imported by tests/test_cls_host.py
and tests/test_gpu_class_stats.py, so the rows exist under ``-m gpu`` and ``-m "not gpu"`` alike (collection imports every module).
The invariance call splits the rows three ways -- not counted, split 0, split 1 -- so every output column and the skipped rows take part:
bit-equal float64 losses under a permuted or sliced population are the claim that the sum order depends on the tree and D alone."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forest_invariance as FI  # noqa: E402
import test_gpu_binding_contract as BC  # noqa: E402

CLASS_STATS = "evogp_hip::tree_batch_class_stats"


def _groups(s, device):
    return FI._d((np.arange(s["D"]) % 3 - 1).astype(np.int32), device)


FI.TABLE[CLASS_STATS] = FI._row(FI._data_op(FI.hip.tree_batch_class_stats, y="cls", tail=(_groups, 2)), out="multi", cpu=("cpu_cls_ops",))

G8 = 8
_OUT = lambda G: [((BC.POP, G, 2), BC.I32), ((BC.POP, G, 2), BC.I32), ((BC.POP, G), torch.float64)]  # noqa: E731

BC.TABLE[CLASS_STATS] = lambda: dict(
    args=BC._data_head(2, use_mse=False) + BC._forest() + [BC._f("variables", BC.D, BC.V), BC._i("labels", BC.D), BC._i("groups", BC.D), ("n_groups", 2)],
    outs=_OUT(2), scalars=dict(BC.SIZES, out_len=(1, 17), n_groups=(0, 9)),
    tensors={"groups": [("of another length", torch.zeros(BC.D + 1, dtype=BC.I32))]},
    also=[("eight splits", {"n_groups": G8}, _OUT(G8)), ("no groups", {"groups": None, "n_groups": 1}, _OUT(1))])
