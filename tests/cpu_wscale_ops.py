"""TEST-ONLY: a CPU implementation of torch.ops.evogp_hip.tree_SR_weighted_scaling backed by the numpy restatement
(tests/weighted_scaling_ref.py) on the CPU oracle's predictions, so that the host logic of Forest.SR_weighted_scaled_fitness,
SymbolicRegression(linear_scaling=True, scaling_loss="problem", ...) and StandardPipeline can be exercised without a GPU.  The product
registers no CPU implementation.  ``calls`` counts the invocations, ``last`` keeps the weights of the latest one."""
import numpy as np
import torch

import evogp_amd  # noqa: F401  (defines the schemas)
import weighted_scaling_ref as WS
from cpu_scale_ops import predictions

_done = False
calls = {"weighted_scaling": 0}
last = {}


def _np(t):
    return t.detach().cpu().numpy()


def register():
    global _done
    if _done:
        return
    _done = True

    def weighted_scaling(pop, D, L, vl, ol, v, t, s, X, y, weights):
        assert ol == 1 and (weights is None or (weights.dim() == 2 and weights.dtype == torch.float32 and weights.is_contiguous()))
        calls["weighted_scaling"] += 1
        last.update(weights=None if weights is None else weights.clone())
        ref = WS.scaling(predictions(_np(v), _np(t), _np(s), _np(X)), _np(y), None if weights is None else _np(weights))
        with np.errstate(over="ignore"):
            coef = np.stack([ref["a"], ref["b"]], axis=1).astype(np.float32)
            return torch.from_numpy(ref["loss"].astype(np.float32)), torch.from_numpy(coef)

    torch.library.impl("evogp_hip::tree_SR_weighted_scaling", "CPU")(weighted_scaling)
