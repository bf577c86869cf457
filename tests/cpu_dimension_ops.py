"""TEST-ONLY: a CPU implementation of torch.ops.evogp_hip.tree_dimensions backed by the integer restatement (tests/dimension_ref.py), so
that the host logic of Forest.SR_dimensions / dimension_mask and SymbolicRegression(input_units=) can be exercised without a GPU.  The
product registers no CPU implementation.  ``calls`` counts the invocations, ``last`` keeps the arguments of the latest one."""
import torch

import evogp_amd  # noqa: F401  (defines the schemas)
import dimension_ref as DR

_done = False
calls = {"tree_dimensions": 0}
last = {}


def _np(t):
    return t.detach().cpu().numpy()


def register():
    global _done
    if _done:
        return
    _done = True

    def tree_dimensions(v, t, s, var_units, label_units, check_root):
        calls["tree_dimensions"] += 1
        last.update(var_units=_np(var_units).copy(), label_units=_np(label_units).copy(), check_root=bool(check_root))
        assert var_units.dtype == torch.int32 and label_units.dtype == torch.int32
        return tuple(torch.from_numpy(a) for a in DR.forest_dimensions(_np(v), _np(t), _np(s), _np(var_units), _np(label_units), check_root))

    torch.library.impl("evogp_hip::tree_dimensions", "CPU")(tree_dimensions)
