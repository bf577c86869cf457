"""CPU: tests/rank_ref.py against scipy and scikit-learn on ties, +-inf and -0.0 next to +0.0: equal mid-ranks, scores within a derived bound."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rank_ref as RR  # noqa: E402

stats = pytest.importorskip("scipy.stats")
metrics = pytest.importorskip("sklearn.metrics")
EPS = 2.0 ** -53


@pytest.mark.parametrize("n", [3, 65, 1000, 8192])
def test_restatement_agrees_with_scipy_and_sklearn(n):
    rng = np.random.default_rng([11, n])
    p = np.round(rng.normal(0, 1, n), 1).astype(np.float32)   # ties
    p[rng.integers(0, n, max(1, n // 16))] = np.inf
    p[rng.integers(0, n, max(1, n // 16))] = -np.inf
    p[:2] = 0.0, -0.0
    y = np.round(p.clip(-3, 3) + rng.normal(0, 1, n), 1).astype(np.float32)
    seg = np.array([0, n])
    r2 = RR.mid_ranks2(p)
    assert np.array_equal(r2, (2 * stats.rankdata(p, "average")).astype(np.int64)) and r2[0] == r2[1]
    q = RR.rank_rows(y, seg)[0]
    w, st = RR.words(p[None], [True], q, seg)
    rho = RR.scores(w, RR.consts(q, seg), seg, "spearman")[0, 0]
    # scipy: Pearson of the centred ranks.  A dot product of n terms errs by (n + 2) eps sum |terms|, i.e. relative to each variance and,
    # by Cauchy-Schwarz, to sqrt(var var) for the covariance: rho moves by 2 (n + 2) eps, plus a few eps of centring, root and division.
    assert abs(rho - stats.spearmanr(p, y).statistic) <= 4 * (n + 8) * EPS
    y01 = (y > np.median(y)).astype(np.int64)
    if 0 < y01.sum() < n:
        wa, _ = RR.words(p[None], [True], y01, seg)
        auc = RR.scores(wa, RR.consts(y01, seg), seg, "auc")[0, 0]
        # sklearn: a trapezoid sum of at most n + 1 terms in [0, 1]
        assert abs(auc - metrics.roc_auc_score(y01, np.nan_to_num(p.astype(np.float64), posinf=1e30, neginf=-1e30))) <= (n + 8) * EPS

