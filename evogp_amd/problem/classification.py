"""Classification — fitness = accuracy of every tree over a labelled dataset
(src/evogp/problem/classification.py:9-83).  ``multi_output=True``: the tree has one output per class and predicts the
arg-max of the soft-maxed outputs; ``multi_output=False``: the single output is rounded onto the label range.  The
outputs come from ``Forest.batch_forward`` — here the non-replicating batch op, so a population of
200 k trees on the 1797-point digits set does not have to be replicated 1797 times as in the reference — and are
reduced tree-block by tree-block so that the (pop, D, classes) tensor never exists in full.

Beyond the reference: ``metric`` picks the fitness among accuracy, balanced accuracy, macro-F1, the multi-class Matthews coefficient
and minus the soft-max cross-entropy, and ``validation_mask`` holds rows out -- all of them from ONE interpretation of the forest
(``Forest.class_stats``, csrc/cls_stats.hip): per tree, split and class the hits and the predictions, per tree and split the loss."""
from __future__ import annotations

import os
from typing import Optional

import torch
from torch import Tensor

from ..tree import Forest, default_device
from .base import BaseProblem

_SKLEARN = ("iris", "wine", "breast_cancer", "digits")
METRICS = ("accuracy", "balanced_accuracy", "f1_macro", "mcc", "cross_entropy")


class Classification(BaseProblem):
    def __init__(self, datapoints: Optional[Tensor] = None, labels: Optional[Tensor] = None,
                 dataset: Optional[str] = None, multi_output: bool = True, block_bytes: int = 1 << 30, metric: str = "accuracy",
                 validation_mask: Optional[Tensor] = None):
        """``metric``: one of ``METRICS``; the fitness is the metric, minus the loss for ``"cross_entropy"``: higher is better everywhere,
        NaN scores -inf.  ``validation_mask``: ``(D,)`` bool; ``evaluate`` scores the ``False`` rows, ``validation_scores`` the ``True`` rows
        of the same launch (``StandardPipeline(validation_patience=)`` follows them).  Both need ``multi_output=True`` and integral labels
        (``ValueError`` otherwise); with ``metric="accuracy"`` and no mask ``evaluate`` is the reference's accuracy as before."""
        if metric not in METRICS:
            raise ValueError(f"metric should be one of {METRICS}, but got {metric!r}")
        if not multi_output and (metric != "accuracy" or validation_mask is not None):
            raise ValueError("metric and validation_mask need multi_output=True: a single-output classifier has accuracy only")
        self.metric = metric
        self.multi_output = multi_output
        self.block_bytes = block_bytes
        if datapoints is not None and labels is not None:
            self.datapoints, self.labels = datapoints, labels
        else:
            assert dataset is not None, "dataset must be provided when datapoints and labels are not provided"
            self.datapoints, self.labels = self.generate_data(dataset)
        self.maximum = int(torch.max(self.labels))
        self.validation_mask = None
        if validation_mask is not None:
            mask = torch.as_tensor(validation_mask)
            if mask.dtype != torch.bool or mask.shape != (self.datapoints.shape[0],):
                raise ValueError(f"validation_mask should be a ({self.datapoints.shape[0]},) bool tensor, but got {mask.dtype}{tuple(mask.shape)}")
            self.validation_mask = mask.to(self.datapoints.device)
        if (metric != "accuracy" or validation_mask is not None) and self._int_labels() is None:
            raise ValueError("metric and validation_mask need integral labels")
        self._stats_cache = None
        self._support = {}

    @staticmethod
    def generate_data(dataset: str):
        assert dataset in _SKLEARN, "Invalid dataset"
        from sklearn import datasets  # offline toy sets only (classification.py:35-48)

        X, y = getattr(datasets, f"load_{dataset}")(return_X_y=True)
        dev = default_device()
        return (torch.tensor(X, dtype=torch.float32, device=dev), torch.tensor(y, dtype=torch.float32, device=dev))

    def transform(self, x: Tensor) -> Tensor:
        return torch.clamp(torch.round(x + self.maximum / 2), 0, self.maximum).squeeze(-1)

    def _accuracy(self, outputs: Tensor) -> Tensor:
        if not self.multi_output:
            pred = self.transform(outputs)
        else:
            eps = 1e-15
            pred = torch.argmax(torch.clip(torch.softmax(outputs, dim=2), eps, 1 - eps), dim=2)
        return torch.sum(pred == self.labels, dim=1, dtype=torch.float32) / self.labels.shape[0]

    def _int_labels(self):
        """int32 copy of the labels when every label is integral, else None (checked once: one host sync per problem)"""
        if not hasattr(self, "_labels_i32"):
            lab = self.labels
            ok = bool(torch.all(lab == torch.round(lab))) if lab.is_floating_point() else True
            self._labels_i32 = lab.to(torch.int32).contiguous() if ok else None
        return self._labels_i32

    # ---- the statistics behind every metric but the plain accuracy ---------------------------------
    def class_stats(self, forest: Forest):
        """``(hits, predicted, loss)`` of ``Forest.class_stats`` on this problem's data: one split without a ``validation_mask``, else
        split 0 = the training rows and split 1 = the held-out rows.  The last result is kept (keyed on the forest's tensors and their
        version counters), so ``validation_scores`` after ``evaluate`` costs no second launch."""
        if not self.multi_output:
            raise ValueError("class_stats needs multi_output=True")
        if self._int_labels() is None:
            raise ValueError("class_stats needs integral labels")
        key = forest._forest_key()
        if self._stats_cache is None or self._stats_cache[0] != key:
            self._stats_cache = (key, forest.class_stats(self.datapoints, self._int_labels(), self.validation_mask))
        return self._stats_cache[1]

    def _class_support(self, classes: int) -> Tensor:
        """float64 ``(splits, classes)``: the counted rows of every split by label (one bincount per problem and class count)"""
        if classes not in self._support:
            lab = self._int_labels().to(torch.int64)
            split = torch.zeros_like(lab) if self.validation_mask is None else self.validation_mask.to(lab.device).to(torch.int64)
            ok = (lab >= 0) & (lab < classes)
            G = 1 if self.validation_mask is None else 2
            self._support[classes] = torch.bincount((split * classes + lab)[ok], minlength=G * classes).reshape(G, classes).to(torch.float64)
        return self._support[classes]

    def _score(self, stats, split: int) -> Tensor:
        """float32 ``(pop,)``: the metric of every tree on one split, -inf where it is NaN (float64 arithmetic on the device)"""
        hits, predicted, loss = (a[:, split].to(torch.float64) for a in stats)
        support = self._class_support(hits.shape[1]).to(hits.device)[split]
        n, seen = support.sum(), support > 0
        if self.metric == "cross_entropy":
            out = -loss
        elif self.metric == "accuracy":
            out = hits.sum(1) / n
        elif self.metric == "balanced_accuracy":
            out = torch.where(seen, hits / support, torch.zeros_like(hits)).sum(1) / seen.sum()      # (a select, not a mask index: no host sync)
        elif self.metric == "f1_macro":
            out = torch.where(seen, 2.0 * hits / (support + predicted), torch.zeros_like(hits)).sum(1) / seen.sum()
        else:   # the multi-class Matthews coefficient: (c s - sum p_k t_k) / sqrt((s^2 - sum p_k^2)(s^2 - sum t_k^2)), 0 for a zero denominator
            cov = hits.sum(1) * n - (predicted * support).sum(1)
            den = torch.sqrt((n * n - (predicted * predicted).sum(1)) * (n * n - (support * support).sum()))
            out = torch.where(den == 0, torch.zeros_like(cov), cov / den)
        return torch.where(torch.isnan(out), torch.full_like(out, float("-inf")), out).to(torch.float32)

    def validation_scores(self, forest: Forest, fitness: Optional[Tensor] = None) -> Tensor:
        """float32 ``(pop,)``: the metric of every tree on the rows ``validation_mask`` holds out, -inf where it is NaN and wherever the
        training score is -inf.  ``fitness``: what ``evaluate(forest)`` has just returned (its launch is reused), or None."""
        if self.validation_mask is None:
            raise ValueError("this problem has no validation_mask")
        stats = self.class_stats(forest)
        train = self._score(stats, 0) if fitness is None else fitness
        out = self._score(stats, 1)
        return torch.where(train.to(out.device) == float("-inf"), torch.full_like(out, float("-inf")), out)

    def evaluate(self, forest: Forest) -> Tensor:
        if self.metric != "accuracy" or self.validation_mask is not None:
            return self._score(self.class_stats(forest), 0)
        D = self.datapoints.shape[0]
        if (self.multi_output and self.datapoints.is_cuda and 2 <= forest.output_len <= 16
                and forest.input_len * 256 <= 150 * 1024 and os.environ.get("EVOGP_FUSED_ACCURACY", "1") != "0"
                and self._int_labels() is not None):
            # fused epilogue: only the per-tree count of correct rows leaves the kernel (csrc/sr_tc.hip END_CLS, csrc/sr_wide.hip).
            # The kernel compares the arg-max with an int32 label: only taken for integral labels (a label like 1.5 never equals
            # a prediction in the reference's `pred == labels`, classification.py:62-75; a truncating cast would make it class 1).
            # The count EQUALS the reference's: argmax(clip(softmax(.))) is the raw arg-max except where an output in front of the
            # maximum is within ~1e-7 of it (their fp32 soft-max values may round to the same float, and torch returns the first);
            # trees with such a row are recounted with aten's soft-max arithmetic (csrc/interp.hpp argmax_as_torch).
            counts = torch.ops.evogp_hip.tree_batch_argmax_count(
                forest.pop_size, D, forest.max_tree_len, forest.input_len, forest.output_len, *forest._tensors(),
                self.datapoints.contiguous().to(torch.float32), self._int_labels())
            return counts.to(torch.float32) / D
        per_tree = 4 * D * max(forest.output_len, 1) * 3        # outputs + soft-max + clip temporaries
        step = max(1, min(forest.pop_size, self.block_bytes // per_tree))
        if step >= forest.pop_size:
            return self._accuracy(forest.batch_forward(self.datapoints))
        parts = [self._accuracy(forest[i:i + step].batch_forward(self.datapoints)) for i in range(0, forest.pop_size, step)]
        return torch.cat(parts)

    @property
    def problem_dim(self):
        return self.datapoints.shape[1]

    @property
    def solution_dim(self):
        return self.maximum + 1 if self.multi_output else 1
