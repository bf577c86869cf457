"""GPU: the weighted losses (csrc/sr_wloss.hip) against the numpy restatement (tests/weighted_loss_ref.py) on the device's own
batch_forward predictions, exact fixtures bit for bit, the rules that decide a value exactly, and the new call next to SR_fitness and
to the problem's torch mode."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

import evogp_amd  # noqa: F401  (registers the ops)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sr_grad_ref as R  # noqa: E402
import test_gpu_binding_contract as BC  # noqa: E402
import weighted_loss_ref as WL  # noqa: E402
from test_gpu_linear_scaling import _case, _dev, _plant  # noqa: E402
from test_gpu_subtree import _malform  # noqa: E402

from evogp_amd.tree import Forest  # noqa: E402

pytestmark = pytest.mark.gpu

B, V, C = R.T_BFUNC, R.T_VAR, R.T_CONST
KINDS = [("mse", None), ("mae", None), ("huber", 0.75), ("pinball", 0.3), ("logcosh", None)]




# The new op joins the binding-contract table (tests/test_gpu_binding_contract.py: one row per op, every argument faulted in turn; its
# test_the_table_covers_every_op reads the table when it runs).  The rows are checked below, by that module's own test body.
def _wloss_row(kind, param, faulty_params):
    return dict(args=BC._data_head(1, use_mse=False) + BC._forest() + BC._xy() + [BC._f("weights", 2, BC.D), ("loss_kind", kind), ("loss_param", param)],
                outs=[((BC.POP, 2), BC.F32)], scalars=dict(BC.SIZES, out_len=(0, 2), loss_kind=(-1, 5), loss_param=faulty_params),
                tensors={"weights": [("of no rows", torch.zeros(0, BC.D)), ("of nine rows", torch.zeros(9, BC.D))]},
                also=[("no weights", {"weights": None}, [((BC.POP, 1), BC.F32)])])


_OP = "evogp_hip::tree_SR_weighted_loss"
_WLOSS_ROWS = {"mse": (0, 0.0, (float("nan"),)), "huber": (2, 1.0, (0.0, -1.0, float("inf"), float("nan"))),
               "pinball": (3, 0.5, (0.0, 1.0, float("nan")))}
BC.TABLE[_OP] = lambda: _wloss_row(*_WLOSS_ROWS["mse"])


@pytest.mark.parametrize("kind", sorted(_WLOSS_ROWS))
def test_binding_contract_of_the_new_op(kind, monkeypatch):
    monkeypatch.setitem(BC.TABLE, _OP, lambda: _wloss_row(*_WLOSS_ROWS[kind]))
    BC.test_valid_call_and_one_fault_at_a_time(_OP)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _loss(value, type_, size, X, y, W, kind, param=None):
    """the op itself: (pop, K) float32, K = 1 without weights"""
    v, t, s, Xd, yd = _dev(value, type_, size, X, y)
    Wd = None if W is None else _dev(np.asarray(W, np.float32).reshape(-1, X.shape[0]))[0]
    pop, L = value.shape
    out = torch.ops.evogp_hip.tree_SR_weighted_loss(pop, X.shape[0], L, X.shape[1], 1, v, t, s, Xd, yd, Wd, WL.KINDS[kind],
                                                    0.0 if param is None else param)
    assert out.shape == (pop, 1 if W is None else Wd.shape[0]) and out.dtype == torch.float32
    return out.cpu().numpy()


def _predictions(value, type_, size, X):
    v, t, s, Xd = _dev(value, type_, size, X)
    pop, L = value.shape
    return torch.ops.evogp_hip.tree_batch_evaluate(pop, X.shape[0], L, X.shape[1], 1, v, t, s, Xd)[:, :, 0].cpu().numpy()


def _weights(rng, K, D):
    """uniform(0, 2) with a third of the entries exactly 0; a row that came out all zero (D = 1) gets one entry back, so that every
    row can be used (the all-zero row is a rule of its own, below)"""
    W = rng.uniform(0, 2, (K, D)).astype(np.float32)
    W[rng.random((K, D)) < 1 / 3] = 0
    for k in np.flatnonzero(~W.any(axis=1)):
        W[k, rng.integers(D)] = np.float32(rng.uniform(0.5, 2))
    return W


# ---- 1. against the restatement on the device's own predictions ------------------------------------------------------------------------
# D below, at and above the 1024-row workgroup tile (and 5000: more tiles than waves, rows reloaded per tree), var_len on both sides of
# the two register-tuple widths (<= 12, 13..32) and past them (the scratch-stack kernel alone); 'arith' forests stay in the LEAN build,
# 'all' forests send trees to the FULL one, the chains _case plants go on to the scratch stack.
SHAPES = [("all", 64, 3, 24, 1), ("arith", 64, 3, 257, 63), ("all", 1024, 3, 257, 65), ("all", 64, 12, 257, 1023),
          ("arith", 64, 13, 257, 1024), ("all", 1024, 32, 24, 1025), ("all", 64, 33, 24, 300), ("all", 64, 3, 24, 5000)]


@pytest.mark.parametrize("kind,param", KINDS)
@pytest.mark.parametrize("funcs,gp_len,var_len,pop,D", SHAPES)
def test_matches_reference_on_batch_forward_predictions(rng, funcs, gp_len, var_len, pop, D, kind, param):
    value, type_, size, X, y = _case(rng, funcs, gp_len, var_len, pop, D)
    P = _predictions(value, type_, size, X)
    for K in (None, 1, 2, 8):   # no weights (nothing loaded), the 2-accumulator build twice, the 8-accumulator build
        W = None if K is None else _weights(rng, K, D)
        got = _loss(value, type_, size, X, y, W, kind, param)
        ref = WL.weighted_loss(P, y, W, kind, param)
        what = f"{funcs} L{gp_len} v{var_len} pop{pop} D{D} {kind} K={K}"
        worst = WL.check(got, ref, D, kind, what)   # equal NaN masks, EVERY finite entry within the derived tolerance
        print(f"{what}: worst error {worst:.3g} of the tolerance, {int(np.isfinite(ref).sum())} of {ref.size} finite")
        assert pop < 24 or np.all(np.isfinite(ref).sum(axis=0) >= pop // 4), what


# ---- 2. exact fixtures: bit equality ------------------------------------------------------------------------------------------------------
def _grid(rng, shape, lo=-4.0):
    return (rng.integers(int(lo * 64), 4 * 64 + 1, shape) / 64.0).astype(np.float32)   # multiples of 2^-6 in [lo, 4]


@pytest.mark.parametrize("D", [1, 300, 1031, 4097])
def test_exact_fixtures_bit_for_bit(rng, D):
    X, y = _grid(rng, (D, 2)), _grid(rng, (D, 1))
    W = _grid(rng, (3, D), lo=0.0)
    W[:, 0] = np.maximum(W[:, 0], np.float32(1 / 64))   # (no all-zero row at D = 1)
    value, type_, size = np.zeros((3, 8), np.float32), np.zeros((3, 8), np.int16), np.zeros((3, 8), np.int16)
    _plant(value, type_, size, 0, [(R.F_SUB, B, 3), (0, V, 1), (1, V, 1)])   # x0 - x1
    _plant(value, type_, size, 1, [(R.F_MUL, B, 3), (0, V, 1), (1, V, 1)])   # x0 * x1
    _plant(value, type_, size, 2, [(_grid(rng, ())[()], C, 1)])               # a CONST
    x0, x1 = X[:, 0].astype(np.float64), X[:, 1].astype(np.float64)
    P = np.stack([x0 - x1, x0 * x1, np.full(D, float(value[2, 0]))])
    assert np.array_equal(P.astype(np.float32).astype(np.float64), P), "the predictions are exact in float32"
    assert np.array_equal(_bits(_predictions(value, type_, size, X)), _bits(P.astype(np.float32)))
    r = P - y[:, 0].astype(np.float64)[None, :]
    for kind, param in (("mse", None), ("mae", None), ("huber", 0.5), ("pinball", 0.25)):
        rho = WL.rho(r, kind, param)
        for Wk in (None, W):
            Wn = np.ones((1, D)) if Wk is None else Wk.astype(np.float64)
            S = (rho[:, None, :] * Wn[None, :, :]).sum(axis=2)   # (3, K)
            # the exactness the bit equality rests on: every term and every partial sum is a float64, in any order
            for t in range(3):
                for k in range(Wn.shape[0]):
                    exact = sum((Fraction(float(w)) * Fraction(float(x)) for w, x in zip(Wn[k], rho[t])), Fraction(0))
                    assert Fraction(float(S[t, k])) == exact, (kind, t, k)
            want = (S / Wn.sum(axis=1)[None, :]).astype(np.float32)
            got = _loss(value, type_, size, X, y, Wk, kind, param)
            assert np.array_equal(_bits(got), _bits(want)), (kind, D, Wk is None, got, want)


# ---- 3. the rules that decide a value exactly ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("var_len", [3, 13, 40])
@pytest.mark.parametrize("D", [1, 300, 1031])
def test_decided_rules_and_determinism(rng, D, var_len):
    pop = 40
    value, type_, size, X, y = _case(rng, "all", 64, var_len, pop, D)
    bad = _malform(value, type_, size)
    # 1 / (x0 - c) with c = the x0 of ONE row: a division by zero on that row
    _plant(value, type_, size, 3, [(R.F_DIV, B, 5), (1.0, C, 1), (R.F_SUB, B, 3), (0, V, 1), (X[D // 2, 0], C, 1)])
    P = _predictions(value, type_, size, X)
    assert not np.isfinite(P[3, D // 2]) and np.isfinite(np.delete(P[3], D // 2)).all()
    kind, param = "huber", 0.75
    W = _weights(rng, 2, D)
    W[0, D // 2], W[1, D // 2] = 0, 1
    got = _loss(value, type_, size, X, y, W, kind, param)
    ref = WL.weighted_loss(P, y, W, kind, param)
    WL.check(got, ref, D, kind, f"rules D{D} v{var_len}")
    assert np.isnan(got[3, 1]), "a row WITH weight on which the tree is not finite: NaN"
    if D > 1:
        assert np.isfinite(got[3, 0]), "a row without weight is not looked at"
    else:   # the one row has no weight in column 0: an all-zero weight row, NaN for every tree
        assert np.isnan(got[:, 0]).all()
    assert np.isnan(got[list(bad)]).all(), "malformed rows are NaN in every column"
    assert np.isfinite(got[:, 1]).sum() >= 10
    # a negative weight, a NaN weight, an all-zero row: NaN for every tree, the columns around them untouched
    Wa, Wb = _weights(rng, 1, D)[0], _weights(rng, 1, D)[0]
    neg, nan = Wa.copy(), Wb.copy()
    neg[D // 3], nan[D - 1] = -0.5, np.nan
    five = _loss(value, type_, size, X, y, np.stack([Wa, neg, Wb, nan, np.zeros(D, np.float32)]), kind, param)
    assert np.isnan(five[:, [1, 3, 4]]).all()
    alone = [_loss(value, type_, size, X, y, w, kind, param)[:, 0] for w in (Wa, Wb)]
    assert np.array_equal(_bits(five[:, 0]), _bits(alone[0])) and np.array_equal(_bits(five[:, 2]), _bits(alone[1]))
    assert np.isfinite(alone[0]).sum() >= 10
    # column independence: a K = 3 call (the 8-accumulator build) is its three K = 1 calls (the 2-accumulator build)
    W3 = _weights(rng, 3, D)
    three = _loss(value, type_, size, X, y, W3, "pinball", 0.3)
    for k in range(3):
        assert np.array_equal(_bits(three[:, k]), _bits(_loss(value, type_, size, X, y, W3[k], "pinball", 0.3)[:, 0])), k
    # no weights is a row of ones, and two identical calls give equal bits
    ones = _loss(value, type_, size, X, y, np.ones(D, np.float32), "logcosh")
    assert np.array_equal(_bits(_loss(value, type_, size, X, y, None, "logcosh")), _bits(ones))
    assert np.array_equal(_bits(_loss(value, type_, size, X, y, W3, "pinball", 0.3)), _bits(three))
    # dedup=True gives the plain call's bits on a forest with duplicate rows
    value2, type2, size2 = (np.concatenate([x, x[:17]]) for x in (value, type_, size))
    forest = Forest(var_len, 1, *_dev(value2, type2, size2))
    Xd, yd, Wd = _dev(X, y, W3)
    plain = forest.SR_weighted_loss(Xd, yd, Wd, "pinball", 0.3).cpu().numpy()
    dedup = forest.SR_weighted_loss(Xd, yd, Wd, "pinball", 0.3, dedup=True).cpu().numpy()
    assert plain.shape == (pop + 17, 3) and np.array_equal(_bits(dedup), _bits(plain))
    assert np.array_equal(_bits(plain[:pop]), _bits(three)) and np.array_equal(_bits(plain[pop:]), _bits(three[:17]))
    flat = forest.SR_weighted_loss(Xd, yd, Wd[1], "pinball", 0.3)
    assert flat.shape == (pop + 17,) and np.array_equal(_bits(flat.cpu().numpy()), _bits(plain[:, 1]))


def test_graph_capture_replays_the_call(rng):
    value, type_, size, X, y = _case(rng, "arith", 64, 3, 200, 300)
    v, t, s, Xd, yd, Wd = _dev(value, type_, size, X, y, _weights(rng, 2, 300))
    args = (200, 300, 64, 3, 1, v, t, s, Xd, yd, Wd, WL.KINDS["huber"], 1.0)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        eager = torch.ops.evogp_hip.tree_SR_weighted_loss(*args)   # (the stream's counter ring is made outside the capture)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            out = torch.ops.evogp_hip.tree_SR_weighted_loss(*args)
        for _ in range(2):
            out.fill_(7.0)
            g.replay()
            side.synchronize()
            assert np.array_equal(_bits(out.cpu().numpy()), _bits(eager.cpu().numpy()))


# ---- 4. next to what exists -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("funcs,gp_len,var_len,pop,D", [("all", 64, 3, 257, 300), ("arith", 1024, 13, 100, 1031), ("all", 64, 40, 24, 70)])
def test_unweighted_mse_and_mae_agree_with_SR_fitness(rng, funcs, gp_len, var_len, pop, D):
    value, type_, size, X, y = _case(rng, funcs, gp_len, var_len, pop, D)
    forest = Forest(var_len, 1, *_dev(value, type_, size))
    Xd, yd = _dev(X, y)
    for use_mse, kind in ((True, "mse"), (False, "mae")):
        fit = forest.SR_fitness(Xd, yd, use_mse).cpu().numpy().astype(np.float64)
        got = forest.SR_weighted_loss(Xd, yd, None, kind).cpu().numpy().astype(np.float64)
        both = np.isfinite(fit) & np.isfinite(got)
        assert both.sum() >= pop // 4
        rel = np.abs(got[both] - fit[both]) / np.abs(fit[both])
        print(f"{funcs} L{gp_len} v{var_len} D{D} {kind}: {both.sum()} trees finite in both, worst relative difference {rel.max():.3g}")
        assert np.all(rel <= 1e-5)   # the project's stated fitness parity


def test_problem_on_the_device_equals_its_torch_twin(rng):
    from evogp_amd.problem import SymbolicRegression

    D, pop = 300, 257
    value, type_, size, X, y = _case(rng, "all", 64, 3, pop, D)
    forest = Forest(3, 1, *_dev(value, type_, size))
    Xd, yd = _dev(X, y)
    w = torch.from_numpy(_weights(rng, 1, D)[0]).cuda()
    m = torch.from_numpy(rng.random(D) < 0.3).cuda()
    opts = dict(datapoints=Xd, labels=yd, loss="huber", loss_param=1.0, sample_weights=w, validation_mask=m)
    prob, twin = SymbolicRegression(**opts), SymbolicRegression(**opts, execute_mode="torch")
    ev, tv = prob.evaluate(forest), twin.evaluate(forest)
    WL.check(-ev.cpu().numpy(), -tv.cpu().numpy(), D, "huber", "training column")
    WL.check(prob.last_validation_loss.cpu().numpy(), twin.last_validation_loss.cpu().numpy(), D, "huber", "validation column")
    assert np.isfinite(ev.cpu().numpy()).sum() >= pop // 4 and np.isfinite(prob.last_validation_loss.cpu().numpy()).sum() >= pop // 4
    # the two columns are two single-row calls, and the scores are the scrubbed columns
    train = forest.SR_weighted_loss(Xd, yd, w * (~m), "huber", 1.0)
    held = forest.SR_weighted_loss(Xd, yd, w * m, "huber", 1.0)
    assert np.array_equal(_bits(ev.cpu().numpy()), _bits((-train).cpu().numpy()))
    assert np.array_equal(_bits(prob.last_validation_loss.cpu().numpy()), _bits(held.cpu().numpy()))
    sc = prob.scores(forest)
    vs = prob.validation_scores(forest, sc)
    ninf = torch.full_like(train, float("-inf"))
    assert torch.equal(sc, torch.where(torch.isnan(train), ninf, -train))
    assert torch.equal(vs, torch.where((sc == float("-inf")) | torch.isnan(held), ninf, -held))
