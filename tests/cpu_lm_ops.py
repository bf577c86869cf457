"""TEST-ONLY: CPU implementations of torch.ops.evogp_hip.tree_SR_normal_eq / tree_SR_lm_step backed by the float64 numpy reference
(tests/sr_lm_ref.py), so that the host logic of Forest.optimize_constants(method="lm"), Forest.SR_normal_equations and
SymbolicRegression(const_opt_method="lm") can be exercised without a GPU.  The product registers no CPU implementation."""
import numpy as np
import torch

import evogp_amd  # noqa: F401  (defines the schemas)
import sr_lm_ref

_done = False
calls = {"normal_eq": 0, "lm_step": 0}   # launches seen, for the tests of the launch counts


def _np(t):
    return t.detach().cpu().numpy()


def register():
    global _done
    if _done:
        return
    _done = True

    def normal_eq(pop, D, L, vl, ol, v, t, s, X, y):
        calls["normal_eq"] += 1
        with np.errstate(all="ignore"):
            loss, normal, _ = sr_lm_ref.forest_normal_eq(_np(v), _np(t), _np(s), _np(X), _np(y))
            return torch.from_numpy(loss.astype(np.float32)), torch.from_numpy(normal.astype(np.float32))

    def lm_step(phase, value, t, s, cand, loss, normal, loss_c, normal_c, damping):
        calls["lm_step"] += 1
        arrs = [value.numpy(), _np(t), _np(s), cand.numpy(), loss.numpy(), normal.numpy(), _np(loss_c), _np(normal_c), damping.numpy()]
        sr_lm_ref.lm_step(*arrs, phase)   # (in place on the tensors' own memory)

    torch.library.impl("evogp_hip::tree_SR_normal_eq", "CPU")(normal_eq)
    torch.library.impl("evogp_hip::tree_SR_lm_step", "CPU")(lm_step)
