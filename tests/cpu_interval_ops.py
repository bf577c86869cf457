"""TEST-ONLY: a CPU implementation of torch.ops.evogp_hip.tree_intervals backed by the numpy restatement (tests/interval_ref.py), so
that the host logic of Forest.SR_intervals / safe_mask and SymbolicRegression(interval_check=) can be exercised without a GPU.  The
product registers no CPU implementation.  ``calls`` counts the invocations."""
import torch

import evogp_amd  # noqa: F401  (defines the schemas)
import interval_ref as IR

_done = False
calls = {"tree_intervals": 0}


def _np(t):
    return t.detach().cpu().numpy()


def register():
    global _done
    if _done:
        return
    _done = True

    def tree_intervals(v, t, s, lower, upper):
        calls["tree_intervals"] += 1
        return tuple(torch.from_numpy(a) for a in IR.forest_intervals(_np(v), _np(t), _np(s), _np(lower), _np(upper)))

    torch.library.impl("evogp_hip::tree_intervals", "CPU")(tree_intervals)
