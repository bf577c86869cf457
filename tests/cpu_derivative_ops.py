"""TEST-ONLY: a CPU implementation of torch.ops.evogp_hip.tree_derivative_intervals backed by the numpy restatement
(tests/derivative_ref.py), so that the host logic of Forest.SR_derivative_intervals / monotone_mask and SymbolicRegression(monotonic=)
can be exercised without a GPU.  The product registers no CPU implementation.  ``calls`` counts the invocations."""
import torch

import evogp_amd  # noqa: F401  (defines the schemas)
import derivative_ref as DR

_done = False
calls = {"tree_derivative_intervals": 0}


def _np(t):
    return t.detach().cpu().numpy()


def register():
    global _done
    if _done:
        return
    _done = True

    def tree_derivative_intervals(v, t, s, lower, upper, wrt):
        calls["tree_derivative_intervals"] += 1
        assert wrt.dtype == torch.int32 and wrt.dim() == 1
        return tuple(torch.from_numpy(a) for a in DR.forest_derivative_intervals(_np(v), _np(t), _np(s), _np(lower), _np(upper), _np(wrt)))

    torch.library.impl("evogp_hip::tree_derivative_intervals", "CPU")(tree_derivative_intervals)
