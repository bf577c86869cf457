"""RankFitness — fitness that depends only on the ORDER of a tree's predictions: Spearman rank correlation with the labels (gplearn's
``metric="spearman"``, the rank IC of formulaic-alpha mining) or ROC-AUC of the tree as a binary scorer, per row segment and averaged
over the segments (no counterpart in the reference).  The sort runs inside the evaluation kernel (csrc/sr_rank.hip):
the (pop, D) predictions are never stored.  Larger is better; a tree that cannot be scored gets ``-inf``."""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from ..tree import Forest
from ..tree.forest import RANK_METRICS, check_tensor, rank_segments
from .base import BaseProblem


class RankFitness(BaseProblem):
    """``metric``: ``"spearman"`` (``labels`` any floats but NaN) or ``"auc"`` (``labels`` 0 / 1).  ``segments``: None (one segment,
    at most 8192 rows) or a ``(D,)`` integer tensor of group ids in any order, e.g. the date of a panel row or a held-out split: the
    score is taken within each group.  ``aggregate="mean"``: the mean score over the segments where it is defined; ``"icir"``: that mean
    divided by the (population) standard deviation of the segment scores; a variance below 64 eps x mean^2 (what rounding alone leaves
    of equal scores) counts as no spread.  ``absolute=True`` takes ``|.|`` of the result.  A tree that
    is malformed, predicts a NaN, has no defined segment or (``"icir"``) no spread scores ``-inf``.

    The payload, the segment table and the row permutation are prepared once here (this synchronises with the host); ``evaluate``
    launches the kernels and a few elementwise ops, nothing else."""

    def __init__(self, datapoints: Tensor, labels: Tensor, metric: str = "spearman", segments: Optional[Tensor] = None,
                 absolute: bool = False, aggregate: str = "mean"):
        if metric not in RANK_METRICS:
            raise ValueError(f"metric should be one of {list(RANK_METRICS)}, but got {metric!r}")
        if aggregate not in ("mean", "icir"):
            raise ValueError(f"aggregate should be 'mean' or 'icir', but got {aggregate!r}")
        if datapoints.dim() != 2 or datapoints.shape[0] < 1:
            raise ValueError(f"datapoints shape should be (D, input_len) with D >= 1, but got {tuple(datapoints.shape)}")
        labels = check_tensor(labels, datapoints.device)
        if labels.dim() == 2 and labels.shape[1] == 1:
            labels = labels[:, 0]
        if labels.shape != (datapoints.shape[0],):
            raise ValueError(f"labels shape should be ({datapoints.shape[0]},) or ({datapoints.shape[0]}, 1), but got {tuple(labels.shape)}")
        self.metric, self.absolute, self.aggregate = metric, absolute, aggregate
        self.segments = rank_segments(segments, datapoints.shape[0], datapoints.device)
        self.datapoints = self.segments.take(datapoints).contiguous().to(torch.float32)
        labels = self.segments.take(labels).contiguous()
        if metric == "auc":
            if not bool(((labels == 0) | (labels == 1)).all()):
                raise ValueError("metric 'auc' takes labels 0 and 1 only")
            self.payload = labels.to(torch.int32)
        else:
            r2, _, status = torch.ops.evogp_hip.rank_rows(labels.to(torch.float32), None, self.segments.seg_start, self.segments.max_segment)
            if bool(status.any()):
                raise ValueError("labels holds a NaN")
            self.payload = r2

    def evaluate(self, forest: Forest) -> Tensor:
        forest._single_output("RankFitness", ValueError)
        if forest.input_len != self.datapoints.shape[1]:
            raise ValueError(f"the forest takes {forest.input_len} inputs, but datapoints has {self.datapoints.shape[1]} columns")
        fused = forest._rank_call(self.datapoints, self.payload, self.segments, self.metric, "fused")[1]
        s, ss, count = fused[:, 0], fused[:, 1], fused[:, 2]
        score = s / count   # (0 / 0 and NaN / NaN: not finite, -inf below)
        if self.aggregate == "icir":
            var = ss / count - score * score   # (cancels: what is left of equal scores is rounding, a few eps of mean^2)
            var = torch.where(var > 64 * torch.finfo(torch.float64).eps * score * score, var, torch.zeros_like(var))
            score = score / torch.sqrt(var)   # (no spread: +-inf or NaN, -inf below)
        if self.absolute:
            score = torch.abs(score)
        return torch.where(torch.isfinite(score), score, torch.full_like(score, float("-inf"))).to(torch.float32)
