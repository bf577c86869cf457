"""NichedFitness — a symbolic-regression fitness that rewards semantic diversity (no counterpart in the reference), from ONE pass of
``Forest.SR_neighbours`` over the whole population (csrc/sr_neigh.hip): no ``(pop, pop)`` matrix, no host synchronisation.

``mode="sharing"``: fitness sharing with a step kernel (Goldberg & Richardson 1987): a tree's loss is multiplied by its niche count,
``1 + (the number of other trees within distance radius of its prediction vector)``.  Semantic duplicates sit at distance exactly 0, so m
copies of one behaviour each carry m times the loss.
``mode="novelty"``: ``weight`` times the mean distance to the ``k`` nearest trees is added to the fitness (Lehman & Stanley 2011, with the
population as its own archive).
Larger is better, as everywhere; a tree the wrapped problem scores ``-inf`` stays at ``-inf``."""
from __future__ import annotations

import torch
from torch import Tensor

from ..tree import Forest
from ..tree.forest import novelty_from_dist2
from .base import BaseProblem
from .symbolic_regression import SymbolicRegression


def sharing_fitness(fitness: Tensor, count: Tensor) -> Tensor:
    """``fitness * (1 + count)``: the loss ``-fitness`` times the niche count, back as a fitness; ``-inf`` stays ``-inf``"""
    shared = fitness * (1 + count).to(fitness.dtype)
    return torch.where(fitness == float("-inf"), fitness, shared)


def novelty_fitness(fitness: Tensor, novelty: Tensor, weight: float) -> Tensor:
    """``fitness + weight * novelty``; ``-inf`` stays ``-inf``, and a tree without a novelty (NaN: unusable) keeps its fitness"""
    bonus = torch.where(torch.isnan(novelty), torch.zeros_like(novelty), novelty) * weight
    return torch.where(fitness == float("-inf"), fitness, fitness + bonus.to(fitness.dtype))


class NichedFitness(BaseProblem):
    """``problem``: a single-output ``SymbolicRegression``; its ``scores`` are the raw fitness and its datapoints the rows on which
    behaviours are compared.  ``radius`` (``"sharing"``): a distance between prediction vectors, i.e. ``sqrt(D)`` times a root-mean-square
    difference per row.  ``k`` (``"novelty"``): 1 .. 16 neighbours.  Populations of up to 131072 trees with ``pop * D <= 2^29``."""

    def __init__(self, problem: SymbolicRegression, mode: str = "sharing", radius: float = 0.0, k: int = 15, weight: float = 1.0):
        if not isinstance(problem, SymbolicRegression):
            raise ValueError(f"problem should be a SymbolicRegression, but got {type(problem).__name__}")
        if mode not in ("sharing", "novelty"):
            raise ValueError(f"mode should be 'sharing' or 'novelty', but got {mode!r}")
        if not float(radius) >= 0.0:
            raise ValueError(f"radius should be >= 0, but got {radius}")
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= 16:
            raise ValueError(f"k should be an integer in 1 .. 16, but got {k!r}")
        self.problem, self.mode, self.radius, self.k, self.weight = problem, mode, float(radius), k, float(weight)

    def evaluate(self, forest: Forest) -> Tensor:
        fitness = self.problem.scores(forest)
        if self.mode == "sharing":
            count = forest.SR_neighbours(self.problem.datapoints, None, 1, [self.radius])[2][:, 0]
            return sharing_fitness(fitness, count)
        return novelty_fitness(fitness, forest.semantic_novelty(self.problem.datapoints, self.k), self.weight)

    @property
    def problem_dim(self):
        return self.problem.problem_dim

    @property
    def solution_dim(self):
        return self.problem.solution_dim
