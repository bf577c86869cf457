"""TEST-ONLY: CPU implementations of torch.ops.evogp_hip.tree_SR_weighted_gradient / tree_SR_weighted_normal_eq backed by the float64
numpy reference (tests/weighted_grad_ref.py), so that the host logic of Forest.SR_gradient / SR_normal_equations /
optimize_constants(weights=, loss=, param=) and SymbolicRegression(const_opt_loss="problem") can be exercised without a GPU.  The
product registers no CPU implementation.  ``calls`` counts the invocations, ``last`` keeps the arguments of the latest one."""
import numpy as np
import torch

import evogp_amd  # noqa: F401  (defines the schemas)
import weighted_grad_ref as WG
import weighted_loss_ref as WL

_done = False
calls = {"weighted_gradient": 0, "weighted_normal_eq": 0}
last = {}
_NAMES = {v: k for k, v in WL.KINDS.items()}


def _np(t):
    return t.detach().cpu().numpy()


def _weights(weights, D):
    assert weights is None or (weights.shape == (D,) and weights.dtype == torch.float32 and weights.is_contiguous())
    return None if weights is None else _np(weights)


def register():
    global _done
    if _done:
        return
    _done = True

    def weighted_gradient(pop, D, L, vl, ol, v, t, s, X, y, weights, kind, param):
        assert ol == 1
        calls["weighted_gradient"] += 1
        last.update(weights=None if weights is None else weights.clone(), kind=_NAMES[kind], param=param)
        prm = param if _NAMES[kind] in ("huber", "pinball") else None
        loss, grad, _ = WG.forest_wgrad(_np(v), _np(t), _np(s), _np(X), _np(y), _weights(weights, D), _NAMES[kind], prm)
        return torch.from_numpy(loss.astype(np.float32)), torch.from_numpy(grad.astype(np.float32))

    def weighted_normal_eq(pop, D, L, vl, ol, v, t, s, X, y, weights):
        assert ol == 1
        calls["weighted_normal_eq"] += 1
        last.update(weights=None if weights is None else weights.clone(), kind="mse", param=0.0)
        loss, normal, _ = WG.forest_wnormal_eq(_np(v), _np(t), _np(s), _np(X), _np(y), _weights(weights, D))
        return torch.from_numpy(loss.astype(np.float32)), torch.from_numpy(normal.astype(np.float32))

    torch.library.impl("evogp_hip::tree_SR_weighted_gradient", "CPU")(weighted_gradient)
    torch.library.impl("evogp_hip::tree_SR_weighted_normal_eq", "CPU")(weighted_normal_eq)
