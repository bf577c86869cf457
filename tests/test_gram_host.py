"""CPU: the solve of the stacked ensemble (evogp_amd/problem/ensemble.py) against numpy on seeded well-conditioned systems, the
minimum-norm solution of a singular one, and the ValueErrors of Forest.SR_gram / fit_ensemble, raised before any op is called."""
import os
import sys

import numpy as np
import pytest
import torch

import evogp_amd  # noqa: F401  (defines the schemas)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gram_tables  # noqa: E402,F401  (the op's rows of the invariance and binding tables exist in every collection)

from evogp_amd.problem.ensemble import ensemble_weights  # noqa: E402
from evogp_amd.tree import Forest  # noqa: E402


def _moments(P, y):
    return P @ P.T, np.stack([P.sum(1), P @ y], 1), y.sum(), (y * y).sum()


def _solve(P, y, ridge):
    """numpy's solution of the centred, regularised normal equations and the training MSE of the fitted model"""
    n, D = P.shape
    Pc, yc = P - P.mean(1, keepdims=True), y - y.mean()
    C = Pc @ Pc.T
    A = C + ridge * np.trace(C) / n * np.eye(n)
    beta = np.linalg.solve(A, Pc @ yc)
    b0 = y.mean() - beta @ P.mean(1)
    return beta, b0, ((beta @ P + b0 - y) ** 2).mean(), np.linalg.cond(A)


@pytest.mark.parametrize("n", [1, 5, 64])
@pytest.mark.parametrize("ridge", [1e-6, 0.0])
def test_ensemble_weights_against_numpy(n, ridge):
    """G = A^T A + I in the issue's words: rows of P that are orthogonal-plus-noise, so cond < 100; rtol from cond n 2^-53 << 1e-9"""
    rng = np.random.default_rng(n)
    D = 256
    P = np.linalg.qr(rng.normal(size=(D, n)))[0].T * 4.0 + rng.normal(size=(n, D)) * 0.1 + rng.normal(size=(n, 1))
    y = rng.normal(size=n) @ P + 0.5 + rng.normal(size=D) * 0.2
    beta, b0, mse, cond = _solve(P, y, ridge)
    assert cond < 100
    G, lin, sy, syy = _moments(P, y)
    w, i0, loss = ensemble_weights(torch.from_numpy(G), torch.from_numpy(lin), sy, syy, D, ridge)
    assert w.dtype == torch.float64 and w.shape == (n,)
    np.testing.assert_allclose(w.numpy(), beta, rtol=1e-9, atol=1e-9 * np.abs(beta).max())
    np.testing.assert_allclose([float(i0), float(loss)], [b0, mse], rtol=1e-9)


def test_a_duplicated_column_and_an_unusable_member():
    rng = np.random.default_rng(7)
    P = rng.normal(size=(4, 128))
    P[3] = P[1]
    y = 2.0 * P[0] - P[1] + 0.25 + rng.normal(size=128) * 0.1
    G, lin, sy, syy = _moments(P, y)
    w, i0, loss = (t.numpy() for t in ensemble_weights(torch.from_numpy(G), torch.from_numpy(lin), sy, syy, 128, 0.0))
    assert np.isfinite(w).all() and abs(w[1] - w[3]) <= 1e-9 and abs(w[0] - 2.0) < 0.1 and abs(w[1] + w[3] + 1.0) < 0.1   # minimum norm: shared
    assert abs(loss - ((w @ P + i0 - y) ** 2).mean()) <= 1e-9 * loss
    G[2, :], G[:, 2], lin[2] = np.nan, np.nan, np.nan
    for ridge in (0.0, 1e-6):
        w2, _, loss2 = ensemble_weights(torch.from_numpy(G), torch.from_numpy(lin), sy, syy, 128, ridge)
        assert w2[2] == 0 and torch.isfinite(w2).all() and torch.isfinite(loss2)
        assert abs(float(loss2) - float(loss)) < 0.05 * float(loss) + 1e-3   # (member 2 carried no signal)


def test_value_errors_come_before_any_op(monkeypatch):
    value = torch.zeros((4, 8))
    value[:, 0] = 1.0
    t = torch.ones((4, 8), dtype=torch.int16)
    single, multi = Forest(2, 1, value, t, t.clone()), Forest(2, 2, value, t, t.clone())
    X, y = torch.zeros((6, 2)), torch.zeros(6)

    def no_op(*a, **k):
        raise AssertionError("an op was called")
    monkeypatch.setattr(Forest, "_tensors", no_op)
    for forest, call in [
        (multi, lambda f: f.SR_gram(X, y)),
        (single, lambda f: f.SR_gram(X[:, :1], y)),
        (single, lambda f: f.SR_gram(X, y[:5])),
        (single, lambda f: f.SR_gram(X, y.to(torch.int32))),
        (single, lambda f: f.SR_gram(X, None, residuals=True)),
        (single, lambda f: f.SR_gram(X, y, torch.zeros(0, dtype=torch.int32))),
        (single, lambda f: f.SR_gram(X, y, torch.zeros(8193, dtype=torch.int32))),
        (single, lambda f: f.SR_gram(X, y, torch.zeros(3))),
        (single, lambda f: f.SR_gram(X, y, torch.zeros((3, 1), dtype=torch.int32))),
        (single, lambda f: f.fit_ensemble(X, None)),
        (single, lambda f: f.fit_ensemble(X, y, ridge=-1.0)),
        (single, lambda f: f.semantic_cosine(X, y[:, None].expand(6, 2))),
    ]:
        with pytest.raises(ValueError):
            call(forest)
    big = Forest(2, 1, torch.zeros((8193, 1)), torch.ones((8193, 1), dtype=torch.int16), torch.ones((8193, 1), dtype=torch.int16))
    with pytest.raises(ValueError):
        big.SR_gram(X, y)
    with pytest.raises(ValueError):
        ensemble_weights(torch.zeros((2, 3), dtype=torch.float64), torch.zeros((2, 2), dtype=torch.float64), 0.0, 1.0, 4)
