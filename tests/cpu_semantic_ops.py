"""TEST-ONLY: CPU implementations of torch.ops.evogp_hip.tree_SR_semantic_hash / tree_SR_semantic_classes backed by the numpy
restatement (tests/semantic_ref.py) on the CPU oracle's predictions, so that the host logic of Forest.semantic_hash /
semantic_classes / semantic_unique, SymbolicRegression(semantic_dedup=) and GeneticProgramming(duplicate_classes=) can be exercised
without a GPU.  The product registers no CPU implementation.  ``calls`` counts the invocations of each."""
import numpy as np
import torch

import evogp_amd  # noqa: F401  (defines the schemas)
import semantic_ref as S
from oracle.pyoracle import Oracle

_done = False
calls = {"semantic_hash": 0, "semantic_classes": 0}


def _np(t):
    return t.detach().cpu().numpy()


def register():
    global _done
    if _done:
        return
    _done = True
    oracle = Oracle("port")

    def check(pop, D, L, vl, ol, v, t, s, X):
        assert ol == 1 and v.shape == t.shape == s.shape == (pop, L) and X.shape == (D, vl) and X.dtype == torch.float32

    def semantic_hash(pop, D, L, vl, ol, v, t, s, X):
        calls["semantic_hash"] += 1
        check(pop, D, L, vl, ol, v, t, s, X)
        P, formed = S.oracle_predictions(oracle, _np(v), _np(t), _np(s), _np(X))
        return torch.from_numpy(S.signature(P, formed).view(np.int64))

    def semantic_classes(pop, D, L, vl, ol, v, t, s, X, h):
        calls["semantic_classes"] += 1
        check(pop, D, L, vl, ol, v, t, s, X)
        assert h.dtype == torch.int64 and h.shape == (pop,)
        P, formed = S.oracle_predictions(oracle, _np(v), _np(t), _np(s), _np(X))
        return torch.from_numpy(S.class_id(P, formed))

    torch.library.impl("evogp_hip::tree_SR_semantic_hash", "CPU")(semantic_hash)
    torch.library.impl("evogp_hip::tree_SR_semantic_classes", "CPU")(semantic_classes)
