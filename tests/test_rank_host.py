"""CPU: the host logic of the rank statistics -- Forest.SR_rank_stats / SR_spearman / SR_auc and RankFitness -- on the test-only CPU ops of
tests/cpu_rank_ops.py: every ValueError before a launch, group ids in any order, the scoring rules of RankFitness (and the table rows)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cpu_rank_ops  # noqa: E402
import rank_tables  # noqa: E402,F401
import sr_grad_ref as R  # noqa: E402
from interval_cases import B, C, V, rows  # noqa: E402

cpu_rank_ops.register()

import evogp.problem  # noqa: E402
from evogp_amd.problem import RankFitness  # noqa: E402
from evogp_amd.tree import Forest  # noqa: E402

D = 24
TREE = B(R.F_ADD, B(R.F_MUL, V(0), V(1)), V(2))   # T = x0 x1 + x2
# 0: T   1: -T   2: a constant   3: NaN on every row   4: x0
PLANTED = [TREE, B(R.F_SUB, C(0.0), TREE), C(2.0), B(R.F_DIV, V(0), C(0.0)), V(0)]


def _forest(exprs=PLANTED, outputs=1):
    return Forest(3, outputs, *(torch.from_numpy(a) for a in rows(exprs, 16)))


def _data():
    rng = np.random.default_rng(11)
    X = rng.choice(np.setdiff1d(np.arange(-8, 9), [0]), (D, 3)).astype(np.float32)
    return torch.from_numpy(X), torch.from_numpy(X[:, 0] * X[:, 1] + X[:, 2])


IDS = torch.tensor([7, 7, 7, 7, 7, 7, 7, 7, -2, -2, -2, -2, -2, -2, -2, -2, 4, 4, 4, 4, 4, 4, 4, 4])


def test_every_value_error_comes_before_a_launch():
    X, y = _data()
    f, n0, q = _forest(), dict(cpu_rank_ops.calls), torch.arange(D)
    bad = [
        lambda: _forest(outputs=2).SR_spearman(X, y),                       # a multi-output forest
        lambda: f.SR_spearman(X[:, :2], y),                                 # a shape that does not fit
        lambda: f.SR_spearman(X, y[:5]),
        lambda: f.SR_rank_stats(X, q.float()),                              # a dtype that does not fit
        lambda: f.SR_rank_stats(X, q, IDS.float()),
        lambda: f.SR_rank_stats(X, q, IDS[:5]),
        lambda: f.SR_rank_stats(X, q - 1),                                  # a payload outside [0, 16384]
        lambda: f.SR_rank_stats(X, q + 16384),
        lambda: f.SR_spearman(X.repeat(400, 1), y.repeat(400)),            # one segment of 9600 rows
        lambda: f.SR_spearman(X.repeat(400, 1), y.repeat(400), torch.zeros(9600, dtype=torch.int64)),
        lambda: f.SR_spearman(X[:0], y[:0], IDS[:0]),                       # an empty id range
        lambda: f.SR_auc(X, y),                                             # labels other than 0 / 1
        lambda: RankFitness(X, y, metric="kendall"),
        lambda: RankFitness(X, y, aggregate="median"),
        lambda: RankFitness(X, y, metric="auc"),
    ]
    for call in bad:
        with pytest.raises(ValueError):
            call()
    assert cpu_rank_ops.calls == n0
    with pytest.raises(ValueError, match="NaN"):                            # (found by the label ranking itself: one rank_rows call)
        f.SR_spearman(X, torch.where(torch.arange(D) == 3, torch.tensor(float("nan")), y))
    assert cpu_rank_ops.calls["rank_stats"] == n0["rank_stats"]


def test_group_ids_in_any_order_give_the_presorted_result():
    (X, y), f = _data(), _forest()
    order = torch.argsort(IDS, stable=True)
    want = f.SR_spearman(X[order], y[order], IDS[order], per_segment=True)
    shuffle = torch.from_numpy(np.random.default_rng(2).permutation(D))
    got = f.SR_spearman(X[shuffle], y[shuffle], IDS[shuffle], per_segment=True)
    assert got.shape == (5, 3) and torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(got[~torch.isnan(got)], want[~torch.isnan(want)])
    assert got[0].tolist() == [1.0, 1.0, 1.0] and got[1].tolist() == [-1.0, -1.0, -1.0] and torch.isnan(got[2:4]).all()
    mean, count = f.SR_spearman(X, y, IDS)
    assert count.tolist() == [3, 3, 0, 0, 3] and mean[:2].tolist() == [1.0, -1.0] and torch.isnan(mean[2:4]).all()
    words, usable = f.SR_rank_stats(X, torch.arange(D), IDS)
    assert words.shape == (5, 3, 2) and usable.tolist() == [True, True, True, False, True] and not words[3].any()
    assert f.SR_auc(X, (y > y.median()).float(), IDS)[0][:2].tolist() == [1.0, 0.0]


def test_rank_fitness_scores():
    (X, y), f = _data(), _forest()
    assert evogp.problem.RankFitness is RankFitness
    fit = RankFitness(X, y, segments=IDS).evaluate(f)
    assert fit.dtype == torch.float32 and fit[:4].tolist() == [1.0, -1.0, float("-inf"), float("-inf")] and -1 < fit[4] < 1
    assert RankFitness(X, y, segments=IDS, absolute=True).evaluate(f)[:2].tolist() == [1.0, 1.0]
    per = f.SR_spearman(X, y, IDS, per_segment=True)[4]
    icir = RankFitness(X, y, segments=IDS, aggregate="icir").evaluate(f)
    assert icir[4] == pytest.approx(float(per.mean() / per.std(unbiased=False)), rel=1e-6)
    assert icir[0] == float("-inf")   # (no spread: 1, 1, 1)
    one = RankFitness(X, (y > y.median()).float(), metric="auc").evaluate(f)   # one segment
    assert one[:4].tolist() == [1.0, 0.0, 0.5, float("-inf")]   # (a constant scorer: every pair tied)

