"""TEST-ONLY: CPU implementations of torch.ops.evogp_hip.tree_SR_linear_scaling / tree_wrap_linear backed by the numpy restatement
(tests/linear_scaling_ref.py) on the CPU oracle's predictions, so that the host logic of Forest.SR_scaled_fitness / apply_scaling,
SymbolicRegression(linear_scaling=) and StandardPipeline can be exercised without a GPU.  The product registers no CPU
implementation.  ``calls`` counts the invocations of each."""
import numpy as np
import torch

import evogp_amd  # noqa: F401  (defines the schemas)
import linear_scaling_ref as LS
from oracle.pyoracle import Oracle
from subtree_ref import live_len, well_formed

_O = Oracle("port")
_done = False
calls = {"linear_scaling": 0, "wrap_linear": 0}


def _np(t):
    return t.detach().cpu().numpy()


def predictions(v, t, s, X):
    """(pop, D) float32: the oracle's batch evaluation, NaN rows for malformed trees"""
    bad = np.array([not well_formed(t[r], live_len(s[r], v.shape[1])) for r in range(v.shape[0])])
    v, t, s = v.copy(), t.copy(), s.copy()
    v[bad, 0], t[bad, 0], s[bad, 0] = 0.0, LS.T_CONST, 1   # (the oracle is not asked to evaluate a malformed row)
    P = _O.batch_evaluate(v, t, s, X, 1)[:, :, 0].copy()
    P[bad] = np.nan
    return P


def register():
    global _done
    if _done:
        return
    _done = True

    def linear_scaling(pop, D, L, vl, ol, v, t, s, X, y):
        assert ol == 1
        calls["linear_scaling"] += 1
        ref = LS.scaling(predictions(_np(v), _np(t), _np(s), _np(X)), _np(y))
        with np.errstate(over="ignore"):
            coef = np.stack([ref["a"], ref["b"]], axis=1).astype(np.float32)
            return torch.from_numpy(ref["loss"].astype(np.float32)), torch.from_numpy(coef)

    def wrap_linear(out_len, v, t, s, coef):
        calls["wrap_linear"] += 1
        return tuple(torch.from_numpy(a) for a in LS.wrap_rows(_np(v), _np(t), _np(s), _np(coef), out_len))

    torch.library.impl("evogp_hip::tree_SR_linear_scaling", "CPU")(linear_scaling)
    torch.library.impl("evogp_hip::tree_wrap_linear", "CPU")(wrap_linear)
