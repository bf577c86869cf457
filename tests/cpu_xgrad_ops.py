"""TEST-ONLY: CPU implementations of torch.ops.evogp_hip.tree_SR_input_gradient / tree_SR_derivative_loss backed by the float64 numpy
restatement (tests/input_grad_ref.py), so that the host logic of Forest.SR_input_gradients / SR_derivative_loss and of
SymbolicRegression(derivative_labels=, sampled_monotonic=) can be exercised without a GPU.  The product registers no CPU implementation."""
import numpy as np
import torch

import evogp_amd  # noqa: F401  (defines the schemas)
import input_grad_ref as XR

_done = False
calls = {"input_gradient": 0, "derivative_loss": 0}


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def register():
    global _done
    if _done:
        return
    _done = True

    def input_gradient(v, t, s, X, wrt):
        calls["input_gradient"] += 1
        pred, d, _ = XR.forest_xgrad(_np(v), _np(t), _np(s), _np(X), list(wrt))
        with np.errstate(all="ignore"):
            return torch.from_numpy(pred.astype(np.float32)), torch.from_numpy(d.astype(np.float32))

    def derivative_loss(v, t, s, X, y, dlabels, wrt, dmin, dmax):
        calls["derivative_loss"] += 1
        loss, viol = XR.derivative_loss(_np(v), _np(t), _np(s), _np(X), _np(y), _np(dlabels), list(wrt), _np(dmin), _np(dmax))
        with np.errstate(all="ignore"):
            return torch.from_numpy(loss.astype(np.float32)), torch.from_numpy(viol)

    torch.library.impl("evogp_hip::tree_SR_input_gradient", "CPU")(input_gradient)
    torch.library.impl("evogp_hip::tree_SR_derivative_loss", "CPU")(derivative_loss)
