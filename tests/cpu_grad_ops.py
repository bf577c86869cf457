"""TEST-ONLY: CPU implementations of torch.ops.evogp_hip.tree_SR_gradient / tree_SR_const_step backed by the float64 numpy
reference (tests/sr_grad_ref.py), so that the host logic of Forest.optimize_constants, SymbolicRegression.optimize and
StandardPipeline can be exercised without a GPU.  The product registers no CPU implementation."""
import numpy as np
import torch

import evogp_amd  # noqa: F401  (defines the schemas)
import sr_grad_ref

_done = False


def _np(t):
    return t.detach().cpu().numpy()


def register():
    global _done
    if _done:
        return
    _done = True

    def gradient(pop, D, L, vl, ol, mse, v, t, s, X, y):
        loss, grad, _ = sr_grad_ref.forest_grad(_np(v), _np(t), _np(s), _np(X), _np(y), mse)
        return torch.from_numpy(loss.astype(np.float32)), torch.from_numpy(grad.astype(np.float32))

    def const_step(phase, out_len, value, t, s, cand, loss, grad, loss_c, grad_c, step):
        arrs = [value.numpy(), _np(t), _np(s), cand.numpy(), loss.numpy(), grad.numpy(), _np(loss_c), _np(grad_c), step.numpy()]
        sr_grad_ref.const_step(*arrs, out_len, phase)   # (in place on the tensors' own memory)

    torch.library.impl("evogp_hip::tree_SR_gradient", "CPU")(gradient)
    torch.library.impl("evogp_hip::tree_SR_const_step", "CPU")(const_step)
