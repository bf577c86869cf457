"""TEST-ONLY: a CPU implementation of torch.ops.evogp_hip.tree_SR_weighted_loss backed by the numpy restatement
(tests/weighted_loss_ref.py) on the CPU oracle's predictions, so that the host logic of Forest.SR_weighted_loss,
SymbolicRegression(loss=, sample_weights=, validation_mask=) and StandardPipeline can be exercised without a GPU.  The product
registers no CPU implementation.  ``calls`` counts the invocations, ``last`` keeps the weights and the kind of the latest one."""
import numpy as np
import torch

import evogp_amd  # noqa: F401  (defines the schemas)
import weighted_loss_ref as WL
from cpu_scale_ops import predictions

_done = False
calls = {"weighted_loss": 0}
last = {}
_NAMES = {v: k for k, v in WL.KINDS.items()}


def _np(t):
    return t.detach().cpu().numpy()


def register():
    global _done
    if _done:
        return
    _done = True

    def weighted_loss(pop, D, L, vl, ol, v, t, s, X, y, weights, kind, param):
        assert ol == 1 and (weights is None or (weights.dim() == 2 and weights.dtype == torch.float32 and weights.is_contiguous()))
        calls["weighted_loss"] += 1
        last.update(weights=None if weights is None else weights.clone(), kind=_NAMES[kind], param=param)
        P = predictions(_np(v), _np(t), _np(s), _np(X))
        return torch.from_numpy(WL.weighted_loss(P, _np(y), None if weights is None else _np(weights), _NAMES[kind], param))

    torch.library.impl("evogp_hip::tree_SR_weighted_loss", "CPU")(weighted_loss)
