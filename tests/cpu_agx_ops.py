"""TEST-ONLY: CPU implementations of torch.ops.evogp_hip.tree_SR_desired_mid / tree_SR_agx_match backed by the numpy restatement
(tests/agx_ref.py, float32 values as the device computes them, the match in float64), so that the host logic of
Forest.SR_midpoint_semantics / SR_midpoint_match and of ApproxGeometricCrossover can be exercised without a GPU.  The product registers
no CPU implementation."""
import numpy as np
import torch

import evogp_amd  # noqa: F401  (defines the schemas)
import agx_ref as AR
import backprop_ref as BR

_done = False
calls = {"desired": 0, "match": 0}


def _np(t):
    return t.detach().cpu().numpy()


def _checked(v, t, s, mv, mt, ms, X, pos, mate):
    pop, L = v.shape
    assert mv.dim() == 2 and mv.shape[1] == L and mv.shape[0] >= 1 and mt.shape == mv.shape == ms.shape
    assert v.dtype == mv.dtype == torch.float32 and t.dtype == mt.dtype == s.dtype == ms.dtype == torch.int16
    assert pos.shape == (pop,) == mate.shape and pos.dtype == torch.int32 == mate.dtype and X.dtype == torch.float32 and X.dim() == 2


def register():
    global _done
    if _done:
        return
    _done = True

    def desired(v, t, s, mv, mt, ms, X, pos, mate):
        calls["desired"] += 1
        _checked(v, t, s, mv, mt, ms, X, pos, mate)
        d, state, status = AR.forest_desired_mid(*map(_np, (v, t, s, mv, mt, ms, X, pos, mate)), np.float32)
        return torch.from_numpy(d), torch.from_numpy(state), torch.from_numpy(status)

    def match(v, t, s, mv, mt, ms, X, pos, mate, lib):
        calls["match"] += 1
        _checked(v, t, s, mv, mt, ms, X, pos, mate)
        assert lib.dim() == 2 and 1 <= lib.shape[0] <= 1024 and lib.shape[1] == X.shape[0] and lib.dtype == torch.float32
        d, state, status = AR.forest_desired_mid(*map(_np, (v, t, s, mv, mt, ms, X, pos, mate)), np.float32)
        best, dist, const, const_dist, counts = BR.match(d, state, status, _np(lib))
        return (torch.from_numpy(best), torch.from_numpy(dist), torch.from_numpy(const.astype(np.float32)), torch.from_numpy(const_dist),
                torch.from_numpy(counts), torch.from_numpy(status))

    torch.library.impl("evogp_hip::tree_SR_desired_mid", "CPU")(desired)
    torch.library.impl("evogp_hip::tree_SR_agx_match", "CPU")(match)
