"""Semantic mate selection (no counterpart in the reference): a geometric choice of the second parent for the geometric operators.

A crossover that moves an offspring towards a point between its parents gains little from a mate drawn uniformly: the error vectors of
two random trees mostly point the same way.  ``SemanticMate`` draws a handful of candidates per first parent and keeps the one whose
residual vector stands best to the first parent's, judged from three inner products per pair (``Forest.SR_pair_moments``,
csrc/sr_pair.hip) -- competent tournament selection (Pawlak & Krawiec 2018), angle-driven selection (Chen, Xue & Zhang
2019) and the blend error of geometric semantic GP with optimal mixing are all functions of those three numbers."""
from __future__ import annotations

import torch

from ..tree import Forest
from ..tree.forest import PAIR_MAX_CANDIDATES


def _midpoint(saa, sbb, sab, sdd):
    """the squared error norm of the midpoint of the two models: the point AGX aims at"""
    return (saa + 2.0 * sab + sbb) / 4.0


def _blend(saa, sbb, sab, sdd):
    """the squared error norm of the best model on the segment between the two"""
    zero = sdd == 0
    alpha = torch.where(zero, torch.zeros_like(sdd), ((sbb - sab) / torch.where(zero, torch.ones_like(sdd), sdd)).clamp(0.0, 1.0))
    return alpha * alpha * saa + 2.0 * alpha * (1.0 - alpha) * sab + (1.0 - alpha) * (1.0 - alpha) * sbb


def _angle(saa, sbb, sab, sdd):
    """the cosine between the two error vectors: the smallest cosine is the largest angle"""
    prod = saa * sbb
    zero = prod == 0
    return torch.where(zero, torch.ones_like(sab), sab / torch.sqrt(torch.where(zero, torch.ones_like(prod), prod)))


def _competent(saa, sbb, sab, sdd):
    """a mate that is good, semantically far from the first parent and at a similar distance from the target"""
    zero = sdd == 0
    score = torch.sqrt(sbb / torch.where(zero, torch.ones_like(sdd), sdd)) * (1.0 + (torch.sqrt(saa) - torch.sqrt(sbb)).abs())
    return torch.where(zero, torch.full_like(score, float("inf")), score)


CRITERIA = {"midpoint": _midpoint, "blend": _blend, "angle": _angle, "competent": _competent}


class SemanticMate:
    """``mate(parents, left) -> (right, score)``: for every first parent ``left[n]`` (indices into the Forest ``parents``) the best of
    ``candidates`` uniformly drawn trees of ``parents`` under ``criterion``, judged on ``datapoints`` / ``labels``.

    ``criterion``: with ``Saa = own`` and ``Sbb, Sab, Sdd = moments[..., 0..2]`` of ``Forest.SR_pair_moments``,
    ``"midpoint"`` ``(Saa + 2 Sab + Sbb) / 4``; ``"blend"`` ``a^2 Saa + 2 a (1 - a) Sab + (1 - a)^2 Sbb`` at ``a = clamp((Sbb - Sab) /
    Sdd, 0, 1)`` (0 where ``Sdd == 0``); ``"angle"`` ``Sab / sqrt(Saa Sbb)`` (1 where the product is 0); ``"competent"``
    ``sqrt(Sbb / Sdd) (1 + |sqrt(Saa) - sqrt(Sbb)|)`` (``+inf`` where ``Sdd == 0``); or a callable ``(own (n, 1), moments (n, M, 3)) ->
    (n, M)``.  Scores are float64, lower is better, an unusable pair (a NaN score) counts as ``+inf``; ties go to the lowest slot, and
    slot 0 is taken when every slot is ``+inf``.  ``labels=None`` judges the predictions themselves.  No host synchronisation."""

    def __init__(self, datapoints: torch.Tensor, labels=None, candidates: int = 8, criterion="midpoint"):
        if not isinstance(datapoints, torch.Tensor) or datapoints.dim() != 2 or datapoints.shape[0] == 0:
            raise ValueError(f"datapoints should be a (D, input_len) tensor, but got {tuple(getattr(datapoints, 'shape', ()))}")
        if isinstance(candidates, bool) or not isinstance(candidates, int) or not 1 <= candidates <= PAIR_MAX_CANDIDATES:
            raise ValueError(f"candidates should be an integer in [1, {PAIR_MAX_CANDIDATES}], but got {candidates!r}")
        if not callable(criterion) and criterion not in CRITERIA:
            raise ValueError(f"criterion should be one of {sorted(CRITERIA)} or a callable, but got {criterion!r}")
        if labels is not None:
            if not isinstance(labels, torch.Tensor) or labels.numel() != datapoints.shape[0] or labels.dim() > 2:
                raise ValueError(f"labels should be a ({datapoints.shape[0]},) tensor, but got {tuple(getattr(labels, 'shape', ()))}")
            labels = labels.reshape(-1).contiguous().to(torch.float32)
        self.datapoints = datapoints.contiguous().to(torch.float32)
        self.labels = labels
        self.candidates = candidates
        self.criterion = criterion

    def scores(self, own: torch.Tensor, moments: torch.Tensor) -> torch.Tensor:
        """(n, M) float64 from ``own`` (n,) and ``moments`` (n, M, 3); NaN -> +inf"""
        own = own[:, None]
        if callable(self.criterion):
            score = self.criterion(own, moments).to(torch.float64)
        else:
            score = CRITERIA[self.criterion](own, moments[..., 0], moments[..., 1], moments[..., 2])
        return torch.where(torch.isnan(score), torch.full_like(score, float("inf")), score)

    def choose(self, parents: Forest, left: torch.Tensor, cand: torch.Tensor):
        """``(right, score)`` for explicit candidates ``cand`` (n, M): ``right[n] = cand[n, argmin score[n]]``; deterministic"""
        own, moments = parents.SR_pair_moments(self.datapoints, self.labels, left, cand)
        score = self.scores(own, moments)
        slot = torch.argmin(score, dim=1, keepdim=True)   # (the first of equal minima: the lowest slot)
        return cand.gather(1, slot)[:, 0], score.gather(1, slot)[:, 0]

    def __call__(self, parents: Forest, left: torch.Tensor):
        cand = torch.randint(0, len(parents), (left.shape[0], self.candidates), dtype=torch.int32, device=left.device)
        return self.choose(parents, left, cand)
