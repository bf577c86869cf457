"""TEST-ONLY: CPU implementations of torch.ops.evogp_hip.tree_SR_gene_fitness / tree_SR_gene_moments backed by the numpy restatement
(tests/gene_ref.py) on the CPU oracle's multi-output evaluation, so that the host logic of Forest.SR_gene_fitness / SR_gene_moments /
gene_predict, SymbolicRegression(multigene=) and StandardPipeline.best_coef can be exercised without a GPU.  The product registers
no CPU implementation.  ``calls`` counts the invocations of each."""
import numpy as np
import torch

import evogp_amd  # noqa: F401  (defines the schemas)
import gene_ref as GR
from oracle.pyoracle import Oracle
from subtree_ref import live_len, well_formed

_O = Oracle("port")
_done = False
calls = {"gene_fitness": 0, "gene_moments": 0}
T_CONST = 1


def _np(t):
    return t.detach().cpu().numpy()


def outputs(v, t, s, X, G):
    """(pop, D, G) float32: the oracle's batch evaluation, NaN for malformed trees"""
    bad = np.array([not well_formed(t[r] & 0x7F if G > 1 else t[r], live_len(s[r], v.shape[1])) for r in range(v.shape[0])])
    v, t, s = v.copy(), t.copy(), s.copy()
    v[bad, 0], t[bad, 0], s[bad, 0] = 0.0, T_CONST, 1   # (the oracle is not asked to evaluate a malformed row)
    P = _O.batch_evaluate(v, t, s, X, G).copy()
    P[bad] = np.nan
    return P


def _fit(ol, v, t, s, X, y):
    ref = GR.fit(outputs(_np(v), _np(t), _np(s), _np(X), ol), _np(y))
    with np.errstate(over="ignore"):
        return ref, torch.from_numpy(ref["loss"].astype(np.float32)), torch.from_numpy(ref["coef"].astype(np.float32))


def register():
    global _done
    if _done:
        return
    _done = True

    def gene_fitness(pop, D, L, vl, ol, v, t, s, X, y):
        assert 1 <= ol <= GR.GENES_MAX and y.shape in ((D,), (D, 1))
        calls["gene_fitness"] += 1
        return _fit(ol, v, t, s, X, y)[1:]

    def gene_moments(pop, D, L, vl, ol, v, t, s, X, y):
        assert 1 <= ol <= GR.GENES_MAX and y.shape in ((D,), (D, 1))
        calls["gene_moments"] += 1
        ref, loss, coef = _fit(ol, v, t, s, X, y)
        return loss, coef, torch.from_numpy(GR.pack(ref["mean"], ref["C"], ref["c"]))

    torch.library.impl("evogp_hip::tree_SR_gene_fitness", "CPU")(gene_fitness)
    torch.library.impl("evogp_hip::tree_SR_gene_moments", "CPU")(gene_moments)
