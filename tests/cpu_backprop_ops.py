"""TEST-ONLY: CPU implementations of torch.ops.evogp_hip.tree_SR_desired / tree_SR_backprop_match backed by the numpy restatement
(tests/backprop_ref.py, float32 values as the device computes them, the match in float64), so that the host logic of
Forest.SR_desired_semantics / SR_backprop_match and of SemanticBackpropMutation can be exercised without a GPU.  The product registers no
CPU implementation."""
import numpy as np
import torch

import evogp_amd  # noqa: F401  (defines the schemas)
import backprop_ref as BR

_done = False
calls = {"desired": 0, "match": 0}


def _np(t):
    return t.detach().cpu().numpy()


def register():
    global _done
    if _done:
        return
    _done = True

    def desired(v, t, s, X, y, pos):
        calls["desired"] += 1
        d, state, status = BR.forest_desired(_np(v), _np(t), _np(s), _np(X), _np(y), _np(pos), np.float32)
        return torch.from_numpy(d), torch.from_numpy(state), torch.from_numpy(status)

    def match(v, t, s, X, y, pos, lib):
        calls["match"] += 1
        assert lib.dim() == 2 and 1 <= lib.shape[0] <= 1024 and lib.shape[1] == X.shape[0] and lib.dtype == torch.float32
        d, state, status = BR.forest_desired(_np(v), _np(t), _np(s), _np(X), _np(y), _np(pos), np.float32)
        best, dist, const, const_dist, counts = BR.match(d, state, status, _np(lib))
        return (torch.from_numpy(best), torch.from_numpy(dist), torch.from_numpy(const.astype(np.float32)), torch.from_numpy(const_dist),
                torch.from_numpy(counts), torch.from_numpy(status))

    torch.library.impl("evogp_hip::tree_SR_desired", "CPU")(desired)
    torch.library.impl("evogp_hip::tree_SR_backprop_match", "CPU")(match)
