"""The least-squares stacked ensemble of a set of trees, from their Gram matrix (``Forest.SR_gram``, csrc/sr_gram.hip).

``ensemble_weights`` is a pure function of float64 tensors on any device: nothing here evaluates a tree."""
from __future__ import annotations

import torch
from torch import Tensor


def ensemble_weights(G: Tensor, lin: Tensor, sum_y, sum_yy, D: int, ridge: float = 0.0):
    """``(weights (n,), intercept, loss)``, float64: the minimiser of ``sum_d (b0 + sum_i b_i p_i[d] - y[d])^2 + ridge' |b|^2`` from
    ``G[i, j] = sum p_i p_j`` ``(n, n)``, ``lin[i] = (sum p_i, sum p_i y)`` ``(n, 2)``, ``sum_y``, ``sum_yy`` and the number of rows ``D``
    (what ``Forest.SR_gram(inputs, labels, index, residuals=False)`` returns).  The normal equations are CENTRED -- ``C = G - s s^T / D``,
    ``c = lin[:, 1] - s sum_y / D`` -- so the intercept drops out and is not penalised; ``ridge' = ridge * trace(C) / m`` over the ``m``
    usable members goes on the diagonal and the system is solved by a Cholesky factorisation.  ``ridge == 0`` takes the minimum-norm
    least-squares solution instead (``torch.linalg.lstsq``, driver ``gelsd``, on the host: a singular ``C`` -- duplicated members -- has one).
    A member with a NaN diagonal (an unusable tree) is left out of the system and gets weight exactly 0.  ``loss`` is the training mean
    squared error, from the quadratic form ``(Syy - 2 b.c + b.C.b) / D`` with ``Syy = sum_yy - sum_y^2 / D``."""
    if G.dim() != 2 or G.shape[0] != G.shape[1] or G.shape[0] < 1 or lin.shape != (G.shape[0], 2):
        raise ValueError(f"G should be (n, n) and lin (n, 2) with n >= 1, but got {tuple(G.shape)} and {tuple(lin.shape)}")
    if G.dtype != torch.float64 or lin.dtype != torch.float64:
        raise ValueError(f"G and lin should be float64, but got {G.dtype} and {lin.dtype}")
    if not ridge >= 0.0 or int(D) < 1:
        raise ValueError(f"ridge should be >= 0 and D >= 1, but got ridge = {ridge}, D = {D}")
    n, D = G.shape[0], float(int(D))
    sum_y, sum_yy = (torch.as_tensor(v, dtype=torch.float64, device=G.device) for v in (sum_y, sum_yy))
    usable = torch.isfinite(torch.diagonal(G)) & torch.isfinite(lin).all(1)
    both = usable[:, None] & usable[None, :]
    s = torch.where(usable, lin[:, 0], 0.0)
    C = torch.where(both, G, 0.0) - s[:, None] * s[None, :] / D
    c = torch.where(usable, lin[:, 1], 0.0) - s * sum_y / D
    if ridge > 0.0:
        lam = ridge * torch.diagonal(C).sum() / usable.sum().clamp(min=1)
        A = C + torch.diag(torch.where(usable, lam, 1.0))   # an unusable member: the row of the identity, b_i = 0 / 1
        L, info = torch.linalg.cholesky_ex(A)
        beta = torch.cholesky_solve(c[:, None], L)[:, 0]
        singular = (info != 0) | ~torch.isfinite(beta).all()   # (ridge' = 0: every member constant on the data)
        beta = torch.where(singular, torch.zeros_like(beta), beta)
    else:
        beta = torch.linalg.lstsq(C.cpu(), c.cpu()[:, None], driver="gelsd").solution[:, 0].to(G.device)
    beta = torch.where(usable, beta, 0.0)
    intercept = (sum_y - (beta * s).sum()) / D
    syy = sum_yy - sum_y * sum_y / D
    loss = (syy - 2.0 * (beta * c).sum() + beta @ (C @ beta)) / D
    return beta, intercept, loss
