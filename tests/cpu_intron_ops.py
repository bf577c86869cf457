"""TEST-ONLY: CPU implementations of torch.ops.evogp_hip.tree_SR_subtree_introns / tree_remove_introns backed by the numpy restatement
(tests/intron_ref.py) on the CPU oracle's predictions of the extracted subtrees, so that the host logic of Forest.SR_subtree_introns /
remove_introns / simplify(introns=True), SymbolicRegression(intron_removal_every=) and the pipeline hook can be exercised without a GPU.
The product registers no CPU implementation.  ``calls`` counts the invocations of each.  The signatures come from cpu_sublib_ops, which
this module registers too."""
import numpy as np
import torch

import evogp_amd  # noqa: F401  (defines the schemas)
import cpu_sublib_ops
import intron_ref as IR
from oracle.pyoracle import Oracle

_done = False
calls = {"subtree_introns": 0, "remove_introns": 0}


def _np(t):
    return t.detach().cpu().numpy()


def register():
    global _done
    cpu_sublib_ops.register()
    if _done:
        return
    _done = True
    oracle = Oracle("port")

    def subtree_introns(pop, D, L, vl, ol, v, t, s, X, sig):
        calls["subtree_introns"] += 1
        assert ol == 1 and v.shape == t.shape == s.shape == sig.shape == (pop, L) and X.shape == (D, vl) and X.dtype == torch.float32
        assert sig.dtype == torch.int64
        f = (_np(v), _np(t), _np(s))
        rep = IR.forest_rep(f[1], f[2], _np(sig).view(np.uint64), IR.values_from(IR.oracle_evaluate(oracle, _np(X)), *f))
        return torch.from_numpy(rep)

    def remove_introns(v, t, s, rep):
        calls["remove_introns"] += 1
        assert v.shape == t.shape == s.shape == rep.shape and rep.dtype == torch.int16
        ov, ot, os_, removed = IR.rewrite(_np(v), _np(t), _np(s), _np(rep))
        return torch.from_numpy(ov), torch.from_numpy(ot), torch.from_numpy(os_), torch.from_numpy(removed)

    torch.library.impl("evogp_hip::tree_SR_subtree_introns", "CPU")(subtree_introns)
    torch.library.impl("evogp_hip::tree_remove_introns", "CPU")(remove_introns)
