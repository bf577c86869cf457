"""CPU: the arithmetic on top of the neighbourhood op (csrc/sr_neigh.hip) -- novelty from ``dist2``, NichedFitness in both modes -- on
hand-made ``dist2`` / ``count`` tensors, and the ValueErrors of Forest.SR_neighbours and NichedFitness, raised before any op is called."""
import math
import os
import sys

import pytest
import torch

import evogp_amd  # noqa: F401  (defines the schemas)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import neigh_tables  # noqa: E402,F401  (the op's rows of the invariance and binding tables exist in every collection)

from evogp_amd.problem import NichedFitness, SymbolicRegression  # noqa: E402
from evogp_amd.tree import Forest  # noqa: E402
from evogp_amd.tree.forest import novelty_from_dist2  # noqa: E402

INF, NAN = math.inf, math.nan
DIST2 = torch.tensor([[0.0, 4.0, 9.0], [1.0, INF, INF], [INF, INF, INF], [NAN, NAN, NAN]], dtype=torch.float64)
NOVELTY = [5.0 / 3.0, 1.0, 0.0, NAN]   # three neighbours, one, none, an unusable tree


def _forest(pop=4, outs=1):
    value = torch.zeros((pop, 8))
    t = torch.ones((pop, 8), dtype=torch.int16)
    return Forest(2, outs, value, t, t.clone())


def test_novelty_is_the_mean_distance_over_the_finite_slots():
    got = novelty_from_dist2(DIST2)
    assert got.dtype == torch.float64 and torch.equal(torch.isnan(got), torch.tensor([False, False, False, True]))
    assert got[:3].tolist() == NOVELTY[:3]


@pytest.mark.parametrize("mode", ["sharing", "novelty"])
def test_niched_fitness_arithmetic(monkeypatch, mode):
    import evogp.problem
    assert evogp.problem.NichedFitness is NichedFitness
    fitness = torch.tensor([-2.0, -0.5, -INF, -INF])
    count = torch.tensor([[3], [0], [7], [0]], dtype=torch.int32)
    seen = {}

    def neighbours(self, inputs, index=None, k=15, radii=None):
        seen.update(k=k, radii=radii)
        return DIST2[:, :k], None, count, None, None
    monkeypatch.setattr(Forest, "SR_neighbours", neighbours)
    monkeypatch.setattr(SymbolicRegression, "scores", lambda self, forest: fitness)
    problem = SymbolicRegression(datapoints=torch.zeros((6, 2)), labels=torch.zeros((6, 1)), execute_mode="torch")
    out = NichedFitness(problem, mode, radius=0.25, k=3, weight=2.0).evaluate(_forest())
    if mode == "sharing":   # the loss times 1 + count
        assert out.tolist() == [-8.0, -0.5, -INF, -INF] and seen == dict(k=1, radii=[0.25])
    else:                   # the fitness plus weight times the novelty
        assert out.tolist() == pytest.approx([-2.0 + 2.0 * NOVELTY[0], 1.5, -INF, -INF], rel=1e-6) and seen["k"] == 3


def test_value_errors_come_before_any_op(monkeypatch):
    single, multi = _forest(), _forest(outs=2)
    X = torch.zeros((6, 2))

    def no_op(*a, **k):
        raise AssertionError("an op was called")
    monkeypatch.setattr(Forest, "_tensors", no_op)
    for forest, call in [
        (multi, lambda f: f.SR_neighbours(X)),
        (single, lambda f: f.SR_neighbours(X[:, :1])),
        (single, lambda f: f.SR_neighbours(X, k=0)),
        (single, lambda f: f.SR_neighbours(X, k=17)),
        (single, lambda f: f.SR_neighbours(X, k=2.0)),
        (single, lambda f: f.SR_neighbours(X, torch.zeros(0, dtype=torch.int32))),
        (single, lambda f: f.SR_neighbours(X, torch.zeros(131073, dtype=torch.int32))),
        (single, lambda f: f.SR_neighbours(torch.zeros((1 << 20, 2)), torch.zeros(513, dtype=torch.int32))),   # the resident panel
        (single, lambda f: f.SR_neighbours(X, torch.zeros(3))),
        (single, lambda f: f.SR_neighbours(X, radii=[-1.0])),
        (single, lambda f: f.SR_neighbours(X, radii=[NAN])),
        (single, lambda f: f.SR_neighbours(X, radii=[0.0] * 9)),
        (single, lambda f: f.SR_neighbours(X, radii=torch.zeros(2, dtype=torch.int32))),
        (single, lambda f: f.semantic_novelty(X, k=17)),
    ]:
        with pytest.raises(ValueError):
            call(forest)
    problem = SymbolicRegression(datapoints=X, labels=torch.zeros((6, 1)), execute_mode="torch")
    for bad in (dict(mode="crowding"), dict(radius=-1.0), dict(k=0), dict(problem=object())):
        with pytest.raises(ValueError):
            NichedFitness(**dict(dict(problem=problem), **bad))
