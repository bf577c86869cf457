"""GPU: second input derivatives (csrc/sr_hessian.hip) through tree_SR_input_gradient / tree_SR_derivative_loss with pair codes: the
materialising form against tests/hessian_ref.py (per tree and pair |kernel - ref64| <= 8 max_rows |ref32 - ref64|, floor 2^-23, over the
rows of the shared 130-row reference finite in both runs; MI355X: worst ratio 1.0, profiles/hessian_report.json), exact cases bit for bit,
the fused form against the materialised arrays ((D + 8) 2^-53 relative plus half a float32 ulp of the stored column), the binding's
errors, Forest and SymbolicRegression(sampled_convex=)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import evogp_amd  # noqa: F401  (registers the ops)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hessian_ref as H  # noqa: E402
import sr_grad_ref as R  # noqa: E402
import test_hessian_ref as TH  # noqa: E402
from helpers import fbits  # noqa: E402
from interval_cases import B, C, IF, V, chain, rows  # noqa: E402

from evogp_amd.problem import SymbolicRegression  # noqa: E402
from evogp_amd.tree import Forest  # noqa: E402

pytestmark = pytest.mark.gpu
hip = torch.ops.evogp_hip
MARGIN, FLOOR = 8.0, 2.0 ** -23
REPORT = {}


def _dev(*arrs):
    return [torch.from_numpy(np.array(a, copy=True, order="C")).cuda() for a in arrs]


def hess(forest, X, pairs):
    pred, dpred = hip.tree_SR_input_gradient(*_dev(*forest), *_dev(X), [H.code(a, b) for a, b in pairs])
    return pred.cpu().numpy(), dpred.cpu().numpy()


def closs(forest, X, y, dy, pairs, lo=None, hi=None):
    opt = [None if a is None else _dev(np.asarray(a, np.float32))[0] for a in (dy, lo, hi)]
    loss, viol = hip.tree_SR_derivative_loss(*_dev(*forest), *_dev(X, y), opt[0], [H.code(a, b) for a, b in pairs], opt[1], opt[2])
    return loss.cpu().numpy(), viol.cpu().numpy()


@pytest.mark.parametrize("P", [1, 8])
@pytest.mark.parametrize("D", [1, 64, 65, 130])
@pytest.mark.parametrize("name", ["arith", "all"])
def test_materialised_against_the_reference(name, D, P):
    forest, X, _, pairs, (p64, h64), (_, h32), ok = TH.gpu_case(name)
    sel = slice(1, 2) if P == 1 else slice(0, 8)   # one mixed pair, or all eight
    pred, h = hess(forest, X[:D], pairs[sel])
    assert h.shape == (P, forest[0].shape[0], D) and pred.shape == h.shape[1:]
    ok, h64, h32 = ok[sel], h64[sel], h32[sel]
    with np.errstate(all="ignore"):
        yard = np.where(ok, np.abs(h32.astype(np.float64) - h64), 0.0).max(2, keepdims=True)   # per pair and tree, over the reference's rows
        err = np.abs(h.astype(np.float64) - h64[:, :, :D])
        ratio = np.where(ok[:, :, :D], err / np.maximum(MARGIN * yard, FLOOR) * MARGIN, 0.0)
    ratio = np.where(ok[:, :, :D] & ~np.isfinite(ratio), np.inf, ratio)
    worst = float(ratio.max())
    REPORT[f"{name} D={D} P={P}"] = worst
    at = np.unravel_index(ratio.argmax(), ratio.shape)
    print(f"{name} D={D} P={P}: worst |kernel - ref64| / yardstick = {worst:.3g} over {int(ok[:, :, :D].sum())} entries")
    assert worst <= MARGIN, f"pair, tree, row {at}: got {h[at]!r}, want {h64[:, :, :D][at]!r}, yardstick {float(yard[at[0], at[1], 0]):.3g}"
    if name == "arith" and P == 8:   # pairs 6 and 7 name the columns no tree reads: +0.0 exactly (a malformed tree: NaN)
        assert (np.isnan(h[6:]) | (fbits(h[6:]) == 0)).all()


def _exact_forest():
    x0, x1 = V(0), V(1)
    trees = [B(R.F_MUL, x0, x1), B(R.F_MUL, x0, x0), B(R.F_ADD, x0, x1), C(1.5), x1,
             IF(x0, B(R.F_MUL, x0, x0), x1), B(R.F_MUL, x0, x1), chain(R.F_MUL, 20, leaf=lambda k: [np.float32(0), R.T_VAR, 1] if k < 2 else [np.float32(1.0), R.T_CONST, 1])]
    value, type_, size = rows(trees, 64)
    size[6, 0] = 65   # malformed: size[0] > L
    return value, type_, size


def test_exact_cases_bit_for_bit():
    forest = _exact_forest()
    X = np.array([[1.5, -2.0], [-0.5, 3.0], [2.0, 0.25], [-3.0, -1.0]], np.float32).repeat(17, 0)   # 68 rows: a ragged second tile
    pred, h = hess(forest, X, [(0, 0), (0, 1)])
    f32 = lambda v: fbits(np.full(len(X), v, np.float32))
    assert (fbits(h[1, 0]) == f32(1.0)).all() and (fbits(h[0, 0]) == 0).all()          # x0 * x1
    assert (fbits(h[0, 1]) == f32(2.0)).all()                                           # x0 * x0
    assert (fbits(h[:, 2:5]) == 0).all()                                                # x0 + x1, a constant, a lone variable
    assert (fbits(h[0, 5]) == np.where(X[:, 0] > 0, f32(2.0), 0)).all() and (fbits(h[1, 5]) == 0).all()
    assert np.isnan(pred[6]).all() and np.isnan(h[:, 6]).all()                          # malformed
    assert (fbits(h[0, 7]) == f32(2.0)).all()                                           # DEEP: x0 * x0 * 1 * 1 ...
    plain = hip.tree_SR_input_gradient(*_dev(*forest), *_dev(X), [0])[0].cpu().numpy()
    assert (fbits(pred) == fbits(plain)).all()                                          # the interpreters' common forward semantics
    again = hess(forest, X, [(0, 0), (0, 1)])
    assert (fbits(again[0]) == fbits(pred)).all() and (fbits(again[1]) == fbits(h)).all()


@pytest.mark.parametrize("name", ["arith", "all"])
def test_a_moved_tree_keeps_its_bits(name):
    forest, X, y, pairs = TH.gpu_case(name)[:4]
    pop = forest[0].shape[0]
    order = np.random.default_rng(3).permutation(pop)[: pop - 5]
    moved = tuple(a[order] for a in forest)
    for call in (lambda f: hess(f, X[:70], pairs), lambda f: closs(f, X[:70], y[:70], None, pairs)):
        a, b = call(forest), call(moved)
        assert (fbits(b[0]) == fbits(a[0][order])).all()
        assert np.array_equal(b[1], a[1][:, order] if a[1].ndim == 3 else a[1][order], equal_nan=True)


@pytest.mark.parametrize("P", [1, 8])
@pytest.mark.parametrize("D", [1, 65, 130])
@pytest.mark.parametrize("name", ["arith", "all"])
def test_fused_against_materialised(name, D, P):
    forest, X, y, pairs = TH.gpu_case(name)[:4]
    pairs, X, y = pairs[:P], X[:D], y[:D]
    pred, h = hess(forest, X, pairs)
    dy = np.random.default_rng(11).uniform(-1, 1, (D, P)).astype(np.float32)
    for labels, lo, hi in ((dy, np.full(P, -0.75, np.float32), np.full(P, 1.5, np.float32)), (None, np.zeros(P, np.float32), np.full(P, np.inf, np.float32)),
                           (None, None, None)):
        loss, viol = closs(forest, X, y, labels, pairs, lo, hi)
        want, want_viol = H.curvature_loss(pred, h, y, labels, lo, hi)
        assert loss.dtype == np.float32 and viol.dtype == np.int32 and np.array_equal(viol, want_viol)
        assert np.array_equal(np.isnan(loss), np.isnan(want))
        with np.errstate(all="ignore"):   # (the terms are non-negative: sum |term| is the sum itself; a column beyond float32 is not held to a bound)
            fin = np.isfinite(want.astype(np.float32))
            bound = (D + 8) * 2.0 ** -53 * want + 0.5 * np.abs(np.spacing(want.astype(np.float32))).astype(np.float64)
            assert (np.abs(loss.astype(np.float64) - want)[fin] <= bound[fin]).all()


@pytest.mark.parametrize("wrt, word", [([1, H.code(0, 1)], "both"), ([H.code(1, 0)], "a <= b"), ([H.code(0, 1), H.code(0, 1)], "twice"),
                                       ([H.code(0, 0)] * 9, "1 to 8"), ([H.code(0, 2)], "a <= b")])
def test_the_binding_rejects(wrt, word):
    forest = _exact_forest()
    X = np.ones((4, 2), np.float32)
    with pytest.raises(RuntimeError, match="wrt") as e:
        hip.tree_SR_input_gradient(*_dev(*forest), *_dev(X), wrt)
    assert word in str(e.value)
    with pytest.raises(RuntimeError, match="wrt"):
        hip.tree_SR_derivative_loss(*_dev(*forest), *_dev(X, X[:, :1]), None, wrt, None, None)


def test_forest_and_problem():
    value, type_, size = rows([B(R.F_MUL, V(0), V(0)), B(R.F_SUB, C(0.0), B(R.F_MUL, V(0), V(0))), V(0)], 8)
    forest = Forest(2, 1, *_dev(value, type_, size))
    X = torch.linspace(-2, 2, 70).reshape(35, 2).cuda()
    y = (X[:, :1] * X[:, :1]).contiguous()
    pred, hs = forest.SR_input_hessians(X, [0, (1, 0)])
    assert hs.shape == (3, 35, 2) and torch.equal(hs[:, :, 0], torch.tensor([2.0, -2.0, 0.0]).cuda()[:, None].expand(3, 35)) and (hs[:, :, 1] == 0).all()
    loss, viol = forest.SR_curvature_loss(X, y, 0, bounds={0: +1})
    assert viol[:, 0].tolist() == [0, 35, 0] and loss[:, 1].tolist() == [4.0, 4.0, 0.0] and float(loss[0, 0]) == 0.0
    for bad in ([], [(0, 1), (1, 0)], [(0, 2)], [0.5], list(range(2)) * 5):
        with pytest.raises(ValueError):
            forest.SR_input_hessians(X, bad)
    with pytest.raises(ValueError):
        forest.SR_curvature_loss(X, y, 0, bounds={0: 2})
    multi = Forest(2, 2, *_dev(value, type_, size))
    for call in (lambda: multi.SR_input_hessians(X, 0), lambda: multi.SR_curvature_loss(X, y, 0)):
        with pytest.raises(ValueError):
            call()
    prob, plain = SymbolicRegression(datapoints=X, labels=y, sampled_convex={0: +1}), SymbolicRegression(datapoints=X, labels=y)
    sc, sc0 = prob.scores(forest), plain.scores(forest)
    assert sc[1] == float("-inf") and torch.equal(sc[[0, 2]], sc0[[0, 2]]) and torch.isfinite(sc0).all()


def test_write_report():
    out = os.environ.get("EVOGP_REPORT_DIR", "")
    if out and os.path.isdir(out) and REPORT:
        json.dump({"margin": MARGIN, "worst_ratio": REPORT}, open(os.path.join(out, "hessian_report.json"), "w"), indent=1, sort_keys=True)
    assert all(r <= MARGIN for r in REPORT.values())
