"""GPU: semantic neighbourhoods (csrc/sr_neigh.hip).  1: against numpy longdouble sums of the exact products of ``batch_forward`` of the
same forest, every distance within the derived bound (D + 12) 2^-53 (sum p_i^2 + sum p_j^2 + 2 sum |p_i p_j|) -- Gram's (D + 8) per word
with -2 G exact, two roundings of the combination and slack for the clamp; not fitted -- and the counts equal at radii the reference
separates.  2: without any tolerance, all five outputs against the numpy restatement of the definition on SR_gram's words, under
permutation, repeats, forced splits and on a side stream.  3: the forest invariants and the binding contract.  4: NichedFitness.

Measured on an MI355X: the worst error / bound ratio of test 1 is 0.24 (n = 65, D = 1025)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import evogp_amd  # noqa: F401  (registers the ops)
from evogp_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forest_invariance as FI  # noqa: E402
import neigh_tables as NT  # noqa: E402
import pair_cases as PC  # noqa: E402
import semantic_ref as S  # noqa: E402
from semantic_cases import X0, X1, plant  # noqa: E402

from evogp_amd.problem import NichedFitness, SymbolicRegression  # noqa: E402
from evogp_amd.tree import Forest  # noqa: E402

pytestmark = pytest.mark.gpu
LD = np.longdouble
TWIN_A, TWIN_B = 32, 33   # x0 + x1 and x1 + x0, planted: equal predictions from different trees


def _dev(*arrs):
    return [torch.from_numpy(np.array(a, order="C")).cuda() for a in arrs]   # (a copy: the shared arrays are read-only)


@functools.lru_cache(maxsize=None)
def truth(funcs, gp_len, pop, D, var_len=3):
    """(forest, X, y, P, usable): pair_cases' forest with the twins planted, and batch_forward's predictions of it"""
    f = [np.array(a) for a in PC.pair_forest(funcs, gp_len, pop, var_len)]
    if pop > TWIN_B:
        plant(*f, TWIN_A, ("add", X0, X1))
        plant(*f, TWIN_B, ("add", X1, X0))
    X, y = PC.pair_data(D, var_len)
    P = Forest(var_len, 1, *_dev(*f)).batch_forward(_dev(X)[0])[:, :, 0].contiguous().cpu().numpy()
    return f, X, y, P, np.isfinite(P).all(1) & S.formed_mask(f[1], f[2])


def neighbours(f, X, index, k, radius2, var_len=3):
    out = torch.ops.evogp_hip.tree_SR_neighbours(*_dev(*f), *_dev(X, np.asarray(index, np.int32)), k, _dev(np.asarray(radius2, np.float64))[0])
    return [o.cpu().numpy() for o in out]


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64))


def _index(n, pop, mixed):
    if not mixed:
        return np.arange(n)
    idx = np.random.default_rng(n).permutation(pop)[:n]   # a permutation holding repeats and indices outside the forest
    idx[[5, 70]], idx[3], idx[77] = idx[[40, 41]], -1, pop
    return idx


# ---- 1. against the plain high-precision reference -----------------------------------------------------------------------------------------
# (funcs, gp_len, n, D, var_len, k, mixed index): n at one tree, k > n - 1, the instruction-tile edge, the block edge on both sides and three
# blocks; D below one group, ragged, one row past a segment and past a slab; var_len 33: the scratch-stack panel kernel alone; gp_len 1024
CASES = [
    ("arith", 64, 1, 3, 3, 1, False),
    ("arith", 64, 2, 257, 3, 16, False),
    ("all", 64, 17, 257, 33, 16, False),
    ("all", 64, 64, 1025, 3, 1, False),
    ("all", 1024, 65, 1025, 3, 16, False),
    ("arith", 64, 130, 4097, 3, 16, False),
    ("all", 64, 130, 257, 3, 5, True),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "{}-L{}-n{}-D{}-v{}-k{}{}".format(*c[:6], "-mixed" if c[6] else ""))
def test_neighbours_match_the_longdouble_reference(case):
    funcs, gp_len, n, D, var_len, k, mixed = case
    pop = 1 if n == 1 else 200
    f, X, _, P, u = truth(funcs, gp_len, pop, D, var_len)
    index = _index(n, pop, mixed)
    inside = (index >= 0) & (index < pop)
    use = inside & u[np.clip(index, 0, pop - 1)]
    v = np.where(use[:, None], P[np.clip(index, 0, pop - 1)], 0).astype(LD)
    G, mag = v @ v.T, np.abs(v) @ np.abs(v).T
    N, M = np.diag(G), np.diag(mag)
    cand = use[:, None] & use[None, :] & ~np.eye(n, dtype=bool)
    d2 = np.where(cand, np.maximum(N[:, None] + N[None, :] - 2 * G, 0), np.inf)
    bound = (D + 12) * 2.0 ** -53 * (M[:, None] + M[None, :] + 2 * mag)
    if n >= 17:   # the condition on the inputs, on the reference alone
        assert use.mean() >= 0.25 and not use.all()
    # the radii: the midpoints of the two widest gaps of the reference's sorted distances, which no distance comes near
    flat = np.sort(d2[cand])
    gaps = np.argsort(np.diff(flat))[-2:] if flat.size > 2 else []
    radius2 = np.array([float((flat[g] + flat[g + 1]) / 2) for g in gaps] or [1.0])
    for r in radius2:
        assert not (cand & (np.abs(d2 - r) <= bound)).any()
    dist2, neigh, count, norm, usable = neighbours(f, X, index, k, radius2, var_len)
    assert dist2.shape == neigh.shape == (n, k) and count.shape == (n, len(radius2)) and norm.shape == usable.shape == (n,)
    assert dist2.dtype == norm.dtype == np.float64 and neigh.dtype == count.dtype == np.int32 and usable.dtype == bool
    assert np.array_equal(usable, use), np.flatnonzero(usable != use)[:8]
    assert np.isnan(dist2[~use]).all() and (neigh[~use] == -1).all() and (count[~use] == 0).all() and np.isnan(norm[~use]).all()
    assert np.array_equal(count, np.stack([(d2 <= r).sum(1) for r in radius2], 1)), "counts"
    assert (np.abs(norm[use].astype(LD) - N[use]) <= (D + 8) * 2.0 ** -53 * M[use]).all()
    worst = 0.0
    for i in np.flatnonzero(use):
        m = min(k, int(cand[i].sum()))
        assert (dist2[i, m:] == np.inf).all() and (neigh[i, m:] == -1).all() and np.isfinite(dist2[i, :m]).all()
        js = neigh[i, :m]
        assert len(set(js.tolist())) == m and cand[i, js].all(), (i, js)                      # distinct, != i, usable
        assert (np.diff(dist2[i, :m]) >= 0).all()
        row = bound[i][cand[i]].max() if m else 0.0
        err_rank = np.abs(dist2[i, :m].astype(LD) - np.sort(d2[i])[:m])                       # an order statistic moves no more than its inputs
        err_pair = np.abs(dist2[i, :m].astype(LD) - d2[i, js])
        assert (err_rank <= row).all() and (err_pair <= bound[i, js]).all(), (i, err_rank, err_pair)
        worst = max([worst] + (err_pair / np.maximum(bound[i, js], LD(1e-300))).astype(float).tolist())
    print(f"n{n} D{D}: {int(use.sum())} usable of {n}, worst error / bound {worst:.3g}")


# ---- 2. word for word ----------------------------------------------------------------------------------------------------------------------
def restate(Gt, ut, pos, k, radius2):
    """the definition in numpy on SR_gram's words Gt (t, t) of the distinct trees; position i of the list holds tree pos[i]"""
    N = np.diag(Gt)
    d2t = np.maximum(0.0, (N[:, None] + N[None, :]) - 2.0 * Gt)
    n, up = len(pos), ut[pos]
    dist, nb = np.full((n, k), np.nan), np.full((n, k), -1, np.int32)
    count = np.zeros((n, len(radius2)), np.int32)
    for a in np.unique(pos[up]):
        row = np.where(up, d2t[a][pos], np.inf)             # every position as a candidate of tree a ...
        order = np.argsort(row, kind="stable")[:k + 1]      # ... by (d2, j)
        within = (row[:, None] <= radius2[None, :]).sum(0)
        for i in np.flatnonzero(pos == a):                  # ... and each position of a leaves itself out
            o = order[order != i][:k]
            o = o[np.isfinite(row[o])]
            dist[i], nb[i, :len(o)] = np.inf, o
            dist[i, :len(o)] = row[o]
            count[i] = within - (row[i] <= radius2)
    return dist, nb, count, np.where(up, N[pos], np.nan), up


def _check(got, want, what):
    for g, w, name in zip(got, want, ("dist2", "neighbour", "count", "norm", "usable")):
        same = _same_bits(g, w) if g.dtype == np.float64 else np.array_equal(g, w)
        assert same, (what, name, np.argwhere(g != w)[:4])


def test_every_output_equals_the_restatement_bit_for_bit():
    f, X, _, P, u = truth("all", 64, 200, 4097)
    forest = Forest(3, 1, *_dev(*f))
    Gt, _, ut = [o.cpu().numpy() for o in forest.SR_gram(_dev(X)[0], None, None, False)]
    radius2 = np.array([0.0, float(np.nanmedian(Gt.diagonal()))])
    base = np.arange(130)
    first = neighbours(f, X, base, 16, radius2)
    _check(first, restate(Gt, ut, base, 16, radius2), "n = 130")
    assert not first[4].all() and first[4].mean() >= 0.25
    assert first[0][TWIN_A, 0] == 0.0 and first[1][TWIN_A, 0] == TWIN_B and first[1][TWIN_B, 0] == TWIN_A   # equal semantics: exactly 0
    perm = np.random.default_rng(3).permutation(130)
    _check(neighbours(f, X, perm, 16, radius2), restate(Gt, ut, perm, 16, radius2), "a permutation")
    for n, stages in ((2000, 15), (2000, 15 | 1 << 8), (2000, 15 | 7 << 8), (8300, 15)):   # the host's splits, one split, seven; beyond Gram's cap
        idx = np.random.default_rng(n).integers(0, 200, n)
        try:
            assert _lib.lib.evogp_hip_debug_sr_neighbours(stages) == 0
            got = neighbours(f, X, idx, 15, radius2)
        finally:
            assert _lib.lib.evogp_hip_debug_sr_neighbours(15) == 0
        _check(got, restate(Gt, ut, idx, 15, radius2), f"n = {n}, stages {stages:#x}")

    args = _dev(*f) + _dev(X, base.astype(np.int32)) + [16, _dev(radius2)[0]]
    call = lambda: torch.ops.evogp_hip.tree_SR_neighbours(*args)   # noqa: E731
    two = call()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        three = call()
    stream.synchronize()
    torch.cuda.synchronize()
    for other in (two, three):
        _check([o.cpu().numpy() for o in other], first, "a second call / a side stream")


# ---- 3. the tables ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FI.cases_for(NT.NEIGH))
def test_op_keeps_the_invariants(case):
    FI.check(NT.NEIGH, FI.TABLE[NT.NEIGH], FI.build_case(case), "cuda")
    torch.cuda.synchronize()


def test_binding_contract():
    NT.BC.test_valid_call_and_one_fault_at_a_time(NT.NEIGH)


# ---- 4. reach ----------------------------------------------------------------------------------------------------------------------------------
def test_niched_fitness_on_the_device():
    f, X, y, P, u = truth("arith", 64, 200, 257)
    forest = Forest(3, 1, *_dev(*f))
    problem = SymbolicRegression(datapoints=_dev(X)[0], labels=_dev(y)[0][:, None].contiguous())
    raw = problem.scores(forest)
    dist2, neigh, count, norm, usable = forest.SR_neighbours(_dev(X)[0], k=4, radii=[1e-3])
    assert np.array_equal(usable.cpu().numpy(), u) and int(count[TWIN_A, 0]) >= 1 and int(count[TWIN_B, 0]) >= 1
    shared = NichedFitness(problem, "sharing", radius=1e-3).evaluate(forest)
    assert torch.equal(shared == -np.inf, raw == -np.inf) and bool((shared <= raw).all())
    assert float(shared[TWIN_A]) < float(raw[TWIN_A]) < 0 and float(shared[TWIN_B]) < float(raw[TWIN_B])   # a larger shared loss
    novel = NichedFitness(problem, "novelty", k=4, weight=0.5).evaluate(forest)
    nov = forest.semantic_novelty(_dev(X)[0], k=4)
    assert torch.equal(novel == -np.inf, raw == -np.inf) and bool((novel >= raw).all()) and bool((novel > raw).any())
    assert torch.equal(torch.isnan(nov), ~usable) and bool((nov[usable] >= 0).all())
