"""TEST-ONLY: a CPU implementation of torch.ops.evogp_hip.tree_SR_pair_moments backed by the numpy restatement (tests/pair_ref.py) on the
CPU oracle's predictions, so that the host logic of Forest.SR_pair_moments / semantic_distance, SemanticMate, SemanticMateCrossover and
ApproxGeometricCrossover(mate=) can be exercised without a GPU.  The product registers no CPU implementation.  ``calls`` counts the
invocations."""
import numpy as np
import torch

import evogp_amd  # noqa: F401  (defines the schemas)
import pair_ref as PR
import semantic_ref as S
from oracle.pyoracle import Oracle

_done = False
calls = {"pair_moments": 0}


def _np(t):
    return t.detach().cpu().numpy()


def register():
    global _done
    if _done:
        return
    _done = True
    oracle = Oracle("port")

    def pair_moments(v, t, s, mv, mt, ms, X, labels, first, cand):
        calls["pair_moments"] += 1
        assert v.shape == t.shape == s.shape and mv.shape == mt.shape == ms.shape and X.dim() == 2 and X.dtype == torch.float32
        assert first.dtype == torch.int32 and cand.dtype == torch.int32 and cand.dim() == 2 and cand.shape[0] == first.shape[0]
        assert 1 <= cand.shape[1] <= 16 and (labels is None or (labels.shape == (X.shape[0],) and labels.dtype == torch.float32))
        Xn = _np(X)
        with np.errstate(all="ignore"):
            PA, fa = S.oracle_predictions(oracle, _np(v), _np(t), _np(s), Xn)
            same = mv.shape == v.shape and all(torch.equal(a, b) for a, b in ((v.view(torch.int32), mv.view(torch.int32)), (t, mt), (s, ms)))
            PB, fb = (PA, fa) if same else S.oracle_predictions(oracle, _np(mv), _np(mt), _np(ms), Xn)
            own, mom, _, _ = PR.pair_moments(PA, PR.usable(PA, fa), PB, PR.usable(PB, fb), None if labels is None else _np(labels),
                                             _np(first), _np(cand))
        return torch.from_numpy(own), torch.from_numpy(mom)

    torch.library.impl("evogp_hip::tree_SR_pair_moments", "CPU")(pair_moments)
