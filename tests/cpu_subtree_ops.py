"""TEST-ONLY: CPU implementations of torch.ops.evogp_hip.tree_SR_subtree_errors / tree_prune backed by the numpy restatement
(tests/subtree_ref.py), so that the host logic of Forest.simplify, SymbolicRegression(simplify_every=) and StandardPipeline can be
exercised without a GPU.  The product registers no CPU implementation.  ``calls`` counts the invocations of each."""
import numpy as np
import torch

import evogp_amd  # noqa: F401  (defines the schemas)
import subtree_ref

_done = False
calls = {"subtree_errors": 0, "prune": 0}


def _np(t):
    return t.detach().cpu().numpy()


def register():
    global _done
    if _done:
        return
    _done = True

    def subtree_errors(pop, D, L, vl, ol, mse, v, t, s, X, y):
        assert ol == 1
        calls["subtree_errors"] += 1
        err, const = subtree_ref.forest_subtree_errors(_np(v), _np(t), _np(s), _np(X), _np(y), mse, np.float32)
        return torch.from_numpy(err.astype(np.float32)), torch.from_numpy(const)

    def prune(ol, hoist, fold, v, t, s, err, const):
        assert ol == 1
        calls["prune"] += 1
        return tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in
                     subtree_ref.prune_rows(_np(v), _np(t), _np(s), _np(err), _np(const), hoist, fold))

    torch.library.impl("evogp_hip::tree_SR_subtree_errors", "CPU")(subtree_errors)
    torch.library.impl("evogp_hip::tree_prune", "CPU")(prune)
