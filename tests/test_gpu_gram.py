"""GPU: the population Gram matrix (csrc/sr_gram.hip) against numpy longdouble sums of the exact products of ``batch_forward`` of the same
forest -- NaN rows and columns and ``usable`` in exactly the reference's positions, every finite word of G and lin within the derived
bound (D + 8) 2^-53 sum |term| (two operand roundings and one product rounding per term, a sum of D terms in any order), no fitted
tolerance and no allowed-bad fraction; then, without any tolerance, what the pinned order of summation promises; the forest invariants;
the stacked ensemble against numpy's solution of the same system; and SymbolicRegression.ensemble on the device.

Measured on an MI355X: the worst error / bound ratio of test 1 is 0.28 (n = 65, D = 5)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import evogp_amd  # noqa: F401  (registers the ops)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forest_invariance as FI  # noqa: E402
import gram_tables as GT  # noqa: E402
import pair_cases as PC  # noqa: E402
import semantic_ref as S  # noqa: E402
from semantic_cases import plant  # noqa: E402

from evogp_amd.problem import SymbolicRegression  # noqa: E402
from evogp_amd.tree import Forest  # noqa: E402

pytestmark = pytest.mark.gpu
LD = np.longdouble
SEG, SLAB = 1024, 4096   # csrc/sr_gram_order.hpp kGramSegment, kGramSlab


def _dev(*arrs):
    return [torch.from_numpy(np.array(a, order="C")).cuda() for a in arrs]   # (a copy: the shared arrays are read-only)


@functools.lru_cache(maxsize=None)
def truth(funcs, gp_len, pop, D, var_len=3):
    """(forest, X, y, P, usable): batch_forward's predictions of a shared forest, once per forest and dataset"""
    f = PC.pair_forest(funcs, gp_len, pop, var_len)
    X, y = PC.pair_data(D, var_len)
    P = Forest(var_len, 1, *_dev(*f)).batch_forward(_dev(X)[0])[:, :, 0].contiguous().cpu().numpy()
    return f, X, y, P, np.isfinite(P).all(1) & S.formed_mask(f[1], f[2])


def gram(f, X, y, index, residuals, var_len=3):
    out = Forest(var_len, 1, *_dev(*f)).SR_gram(_dev(X)[0], None if y is None else _dev(y)[0], _dev(np.asarray(index, np.int32))[0], residuals)
    return [o.cpu().numpy() for o in out]


def reference(P, u, y, index, residuals):
    """(G, lin, usable, |G| terms, |lin| terms): longdouble sums of exact products, rounded once; NaN by the flags"""
    pop = P.shape[0]
    index = np.asarray(index)
    inside = (index >= 0) & (index < pop)
    use = inside & u[np.clip(index, 0, pop - 1)]
    v = np.where(use[:, None], P[np.clip(index, 0, pop - 1)], 0).astype(LD)
    yl = np.zeros(P.shape[1], LD) if y is None else y.astype(LD)
    if residuals:
        v = v - yl[None, :]
    G, Gmag = v @ v.T, np.abs(v) @ np.abs(v).T
    lin = np.stack([v.sum(1), v @ yl], 1)
    lmag = np.stack([np.abs(v).sum(1), np.abs(v) @ np.abs(yl)], 1)
    G[~use, :], G[:, ~use], lin[~use] = np.nan, np.nan, np.nan
    return G.astype(np.float64), lin.astype(np.float64), use, Gmag, lmag


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64))


def _index(n, pop, mixed):
    if not mixed:
        return np.arange(n)
    idx = np.random.default_rng(n).permutation(pop)[:n]   # a permutation holding repeats and indices outside the forest
    idx[[5, 70]], idx[3], idx[77] = idx[[40, 41]], -1, pop
    return idx


# ---- 1. against the plain high-precision reference -----------------------------------------------------------------------------------------
# (funcs, gp_len, n, D, var_len, labels, residuals, mixed index): n at the instruction-tile edge (17), the block edge (65: 67 vectors with
# the two virtual ones) and three blocks (130); D below one group, ragged, one row past a segment and past a slab; var_len 33: the
# scratch-stack kernel alone; gp_len 1024: the 79-node comb, deeper than the register stack, next to register trees
CASES = [
    ("arith", 64, 1, 1, 3, True, True, False),
    ("arith", 64, 17, 3, 3, True, False, False),
    ("all", 64, 65, 5, 3, False, False, False),
    ("all", 64, 65, 257, 3, True, True, False),
    ("all", 1024, 130, SEG + 1, 3, True, True, False),
    ("arith", 64, 130, SLAB + 1, 3, True, False, False),
    ("all", 64, 130, SLAB + 1, 3, True, True, False),
    ("all", 64, 17, 257, 33, True, True, False),
    ("arith", 64, 65, SEG + 1, 33, False, False, False),
    ("all", 64, 130, 257, 3, True, True, True),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "{}-L{}-n{}-D{}-v{}-{}{}{}".format(*c[:5], "y" if c[5] else "noy", "-resid" if c[6] else "", "-mixed" if c[7] else ""))
def test_gram_matches_the_longdouble_reference(case):
    funcs, gp_len, n, D, var_len, labels, residuals, mixed = case
    pop = 1 if n == 1 else 200
    f, X, y, P, u = truth(funcs, gp_len, pop, D, var_len)
    y = y if labels else None
    index = _index(n, pop, mixed)
    want, want_lin, use, mag, lmag = reference(P, u, y, index, residuals)
    if n >= 17:   # the condition on the inputs, on the reference alone
        off = ~np.eye(n, dtype=bool)
        assert np.isfinite(want[off]).mean() >= 0.25 and not use.all()
    G, lin, usable = gram(f, X, y, index, residuals, var_len)
    assert G.shape == (n, n) and lin.shape == (n, 2) and usable.shape == (n,) and G.dtype == lin.dtype == np.float64 and usable.dtype == bool
    assert np.array_equal(usable, use), np.flatnonzero(usable != use)[:8]
    assert np.array_equal(np.isnan(G), np.isnan(want)) and np.array_equal(np.isnan(lin), np.isnan(want_lin))
    assert np.isfinite(G[use][:, use]).all() and np.isfinite(lin[use]).all()
    eps = (D + 8) * 2.0 ** -53
    worst = 0.0
    for got, ref, m in ((G, want, mag), (lin, want_lin, lmag)):
        ok = ~np.isnan(ref)
        err, lim = np.abs(got.astype(LD) - ref)[ok], (eps * m)[ok]
        worst = max(worst, float((err / np.maximum(lim, LD(1e-300))).max()) if err.size else 0.0)
        assert (err <= lim).all(), np.argwhere(ok & (np.abs(got.astype(LD) - ref) > eps * m))[:8]
    if not labels:
        assert (lin[use, 1] == 0).all()
    print(f"n{n} D{D}: {int(use.sum())} usable of {n}, worst error / bound {worst:.3g}")


# ---- 2. bit for bit ----------------------------------------------------------------------------------------------------------------------------
def test_a_word_depends_on_its_two_trees_and_the_data_alone():
    f, X, y, P, u = truth("all", 64, 200, SLAB + 1)
    base = np.arange(130)
    G, lin, usable = gram(f, X, y, base, True)
    assert np.isfinite(G).mean() >= 0.25 and not usable.all()
    assert _same_bits(G, G.T)
    perm = np.random.default_rng(3).permutation(130)
    Gp, linp, up = gram(f, X, y, base[perm], True)
    assert _same_bits(Gp, G[perm][:, perm]) and _same_bits(linp, lin[perm]) and np.array_equal(up, usable[perm])
    sub = np.sort(perm[:40])   # one output block where the whole list has six
    Gs, lins, _ = gram(f, X, y, sub, True)
    assert _same_bits(Gs, G[sub][:, sub]) and _same_bits(lins, lin[sub])
    rep = base.copy()
    rep[100] = rep[3]
    Gr, linr, _ = gram(f, X, y, rep, True)
    assert np.isfinite(Gr[3]).any() and _same_bits(Gr[100], Gr[3]) and _same_bits(Gr[:, 100], Gr[:, 3]) and _same_bits(linr[100], linr[3])
    # 2000 trees: a workgroup owns every segment of a slab and adds them itself; below, one segment each and a second kernel adds
    big = np.concatenate([base, np.random.default_rng(4).integers(0, 200, 1870)])
    Gb, linb, ub = gram(f, X, y, big, True)
    assert _same_bits(Gb[:130, :130], G) and _same_bits(linb[:130], lin) and _same_bits(Gb, Gb.T)
    assert _same_bits(Gb[np.ix_(big == 9, big == 0)], np.full(((big == 9).sum(), (big == 0).sum()), G[9, 0]))

    forest, args = Forest(3, 1, *_dev(*f)), _dev(X, y, base.astype(np.int32))
    one, two = forest.SR_gram(*args, True), forest.SR_gram(*args, True)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        three = forest.SR_gram(*args, True)
    stream.synchronize()
    torch.cuda.synchronize()
    for other in (two, three):
        assert all(_same_bits(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(one[:2], other[:2])) and torch.equal(one[2], other[2])
    assert _same_bits(one[0].cpu().numpy(), G)


# ---- 3. the tables ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FI.cases_for(GT.GRAM))
def test_op_keeps_the_invariants(case):
    FI.check(GT.GRAM, FI.TABLE[GT.GRAM], FI.build_case(case), "cuda")
    torch.cuda.synchronize()


def test_binding_contract():
    GT.BC.test_valid_call_and_one_fault_at_a_time(GT.GRAM)


# ---- 4. the stacked ensemble -------------------------------------------------------------------------------------------------------------------
def test_fit_ensemble_solves_the_reference_system():
    """45 arithmetic trees that are nearly orthogonal on the data (x_i and x_i * x_j over 10 uniform variables: cond of the centred system
    is about 10) and three unusable members; the derivation of the tolerance: cond n (D + 8) 2^-53 <= 1e4 * 48 * 1032 * 1.1e-16 = 6e-8 is
    the worst relative perturbation of the solution, and a decade is added for the solve"""
    n, D, V, ridge = 48, 1024, 10, 1e-6
    rng = np.random.default_rng(31)
    X = rng.uniform(-1, 1, (D, V)).astype(np.float32)
    y = (0.5 * X[:, 0] + X[:, 1] * X[:, 2] - 0.3 * X[:, 3] * X[:, 4] + 0.7 + rng.normal(0, 0.3, D)).astype(np.float32)
    f = [np.zeros((n, 64), np.float32), np.zeros((n, 64), np.int16), np.zeros((n, 64), np.int16)]
    feats = [("x", i) for i in range(V)] + [("mul", ("x", i), ("x", j)) for i in range(V) for j in range(i + 1, V)]
    for t in range(n):
        plant(*f, t, feats[t])
    plant(*f, 20, ("div", ("x", 0), ("c", np.float32(0.0))))   # NaN on every row
    f[2][33, 0] = 0                                             # malformed
    index = np.arange(n)
    index[41] = n                                               # outside the forest
    forest = Forest(V, 1, *_dev(*f))
    Xd, yd, idx = _dev(X, y, index.astype(np.int32))
    w, b0, loss = forest.fit_ensemble(Xd, yd, idx, ridge)
    assert w.dtype == torch.float64 and w.shape == (n,) and b0.dtype == loss.dtype == torch.float64
    w, b0, loss = w.cpu().numpy(), float(b0), float(loss)

    P = forest.batch_forward(Xd)[:, :, 0].cpu().numpy()
    u = np.isfinite(P).all(1) & S.formed_mask(f[1], f[2])
    G, lin, use, _, _ = reference(P, u, y, index, False)
    assert use.sum() == 45 and (w[~use] == 0).all()
    yl = y.astype(LD)
    s, sy = lin[use, 0], float(yl.sum())
    C = G[use][:, use] - np.outer(s, s) / D
    c = lin[use, 1] - s * sy / D
    A = C + ridge * np.trace(C) / use.sum() * np.eye(use.sum())
    assert np.linalg.cond(A) <= 1e4
    beta = np.linalg.solve(A, c)
    assert np.abs(w[use] - beta).max() <= 1e-6 * np.abs(beta).max()
    mse = ((P[use].astype(np.float64) - y[None, :].astype(np.float64)) ** 2).mean(1)
    assert loss <= mse.min() * (1 + 1e-9)
    pred = forest.ensemble_predict(Xd, idx, *_dev(w), b0).cpu().numpy()
    direct = float(((pred - y.astype(np.float64)) ** 2).mean())
    syy = float((yl * yl).sum() / D)
    assert syy / 1e3 <= loss <= syy   # the quadratic form cancels at most three decades
    assert abs(loss - direct) <= 1e-9 * direct, (loss, direct)


# ---- 5. reach ----------------------------------------------------------------------------------------------------------------------------------
def test_symbolic_regression_ensemble_on_the_device():
    f, X, y, P, u = truth("arith", 64, 200, 257)
    forest = Forest(3, 1, *_dev(*f))
    problem = SymbolicRegression(datapoints=_dev(X)[0], labels=_dev(y)[0][:, None].contiguous())
    index, w, b0, loss = problem.ensemble(forest, k=16)
    scores = problem.scores(forest).cpu().numpy()
    assert index.dtype == torch.int32 and 1 <= index.numel() <= 16 and w.shape == index.shape and w.is_cuda
    assert np.isfinite(scores[index.cpu().numpy()]).all() and np.isfinite(w.cpu().numpy()).all()
    # the ridge solution is no worse than the best member up to ridge * (mean member variance) / best MSE, far below 1e-3 here
    assert 0 <= float(loss) <= -scores.max() * (1 + 1e-3)
