"""GPU: the input-gradient kernels (csrc/sr_xgrad.hip; ops tree_SR_input_gradient and tree_SR_derivative_loss).

  * the materialising op against the float64 restatement (tests/input_grad_ref.py) on the five fixture forests, all 100 rows, and against
    the derivative truth of tests/golden/input_grad_truth_*.npz on the first 32: every entry the exclusion rule keeps (the rule and its
    floors are those of tests/test_input_grad_truth.py) within 1e-3 scale + 1e-7, the bound tests/test_gpu_sr_grad.py holds the same
    float32 adjoint rules to; no allowed-bad fraction.  The worst ratios go to input_grad_truth_report.json under EVOGP_REPORT_DIR;
  * every path: LDS and global tapes, ragged tiles, 1 to 4 waves per tree and the one-wave plan of a population that fills the chip,
    1, 3 and 8 requested variables in no order;
  * the fused op against the materialised arrays: the losses recomputed in float64 numpy within 1 float32 ulp (float64 sums of at most D
    non-negative terms differ by D 2^-53 relative), NaN columns and violation counts exactly; column 0 against
    tree_SR_weighted_gradient(weights=None, MSE) bit for bit;
  * edge rows among ordinary trees, determinism, the binding contract, the forest invariants, Forest and SymbolicRegression end to end."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import evogp_amd  # noqa: F401  (registers the ops)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_eval_ref as ex  # noqa: E402
import forest_invariance as FI  # noqa: E402
import input_grad_ref as XR  # noqa: E402
import sr_grad_ref as R  # noqa: E402
import test_input_grad_truth as TT  # noqa: E402
import xgrad_tables as XT  # noqa: E402
from grad_trees import ALL_FUNCS, ARITH, random_forest  # noqa: E402
from helpers import assert_close_classes, fbits  # noqa: E402
from interval_cases import B, C, IF, U, V, rows  # noqa: E402

from evogp_amd.algorithm import DefaultCrossover, DefaultMutation, DefaultSelection, GeneticProgramming  # noqa: E402
from evogp_amd.pipeline import StandardPipeline  # noqa: E402
from evogp_amd.problem import SymbolicRegression  # noqa: E402
from evogp_amd.tree import Forest, GenerateDescriptor  # noqa: E402

pytestmark = pytest.mark.gpu
hip = torch.ops.evogp_hip
REPORT = {}
MSE = 0   # EVOGP_LOSS_MSE


def _dev(*arrs):
    return [torch.from_numpy(np.array(a, copy=True, order="C")).cuda() for a in arrs]


def xgrad(forest, X, wrt):
    pred, dpred = hip.tree_SR_input_gradient(*_dev(*forest), *_dev(X), [int(v) for v in wrt])
    return pred.cpu().numpy(), dpred.cpu().numpy()


def dloss(forest, X, y, dy, wrt, dmin=None, dmax=None):
    opt = [None if a is None else _dev(np.asarray(a, np.float32))[0] for a in (dy, dmin, dmax)]
    loss, viol = hip.tree_SR_derivative_loss(*_dev(*forest), *_dev(X, y), opt[0], [int(v) for v in wrt], opt[1], opt[2])
    return loss.cpu().numpy(), viol.cpu().numpy()


def batch_evaluate(forest, X):
    pop, L = forest[0].shape
    return hip.tree_batch_evaluate(pop, X.shape[0], L, X.shape[1], 1, *_dev(*forest), *_dev(X))[:, :, 0].cpu().numpy()


def fits_float32(forest, X, wrt):
    """bool (V, pop, D): the float32 run of the restatement's walk stays finite -- prediction, derivative and scale.  The forests of the
    path tests are drawn here, over all 29 functions: an entry whose value, or an intermediate of it, is beyond float32's range (a float64
    derivative of 9.6e47 occurs) has no float32 value to hold the kernel to; the rule alone, which looks at float64, does not see that"""
    with np.errstate(all="ignore"):
        p, d, s = XR.forest_xgrad(*forest, X, wrt, dtype=np.float32)
        return np.isfinite(p)[None] & np.isfinite(d) & np.isfinite(s)


def assert_within(got, want, scale, mask, what, report_key=None):
    """every masked entry of got within 1e-3 scale + 1e-7 of want"""
    worst, ratio = TT.worst_ratio(got, want, 1e-3 * scale + 1e-7, mask)
    print(f"{what}: worst |got - want| / (1e-3 scale + 1e-7) = {worst:.3g} over {int(mask.sum())} entries")
    if report_key:
        REPORT[report_key] = worst
    if not worst <= 1.0:
        at = np.unravel_index(np.argmax(ratio), ratio.shape)
        raise AssertionError(f"{what}: variable, tree, row {tuple(int(i) for i in at)}: got {got[at]!r}, want {want[at]!r}, scale {scale[at]:.3g}; "
                             f"{int((ratio > 1).sum())} of {int(mask.sum())} compared entries beyond the bound")


def check_fused_against_materialised(forest, X, y, dy, wrt, pred, dpred, what):
    """the fused op with labels and finite bounds, with +-1 signs and with neither, against the arrays of the materialising op"""
    V_ = len(wrt)
    signs = [(0.0, np.inf) if k % 2 == 0 else (-np.inf, 0.0) for k in range(V_)]
    for name, labels, lo, hi in (("finite bounds", dy, np.full(V_, -0.75, np.float32), np.full(V_, 1.5, np.float32)),
                                 ("signs", dy, [s[0] for s in signs], [s[1] for s in signs]), ("no labels, no bounds", None, None, None)):
        loss, viol = dloss(forest, X, y, labels, wrt, lo, hi)
        want_loss, want_viol = XR.loss_columns(pred, dpred, y, labels, lo, hi)
        assert loss.shape == want_loss.shape and loss.dtype == np.float32 and viol.dtype == np.int32
        assert np.array_equal(np.isnan(loss), np.isnan(want_loss)), f"{what}, {name}: the NaN columns differ at {np.argwhere(np.isnan(loss) != np.isnan(want_loss))[:4].tolist()}"
        fin = ~np.isnan(want_loss)
        with np.errstate(all="ignore"):
            w32 = want_loss.astype(np.float32)
            ulp = np.abs(np.spacing(w32)).astype(np.float64)
            bad = fin & ~(np.abs(loss.astype(np.float64) - w32.astype(np.float64)) <= ulp) & ~(np.isinf(w32) & (loss == w32))
        assert not bad.any(), f"{what}, {name}: loss differs by more than 1 ulp at {np.argwhere(bad)[:4].tolist()}: {loss[bad][:4]} against {want_loss[bad][:4]}"
        assert np.array_equal(viol, want_viol), f"{what}, {name}: violations differ at {np.argwhere(viol != want_viol)[:4].tolist()}"
    return loss   # (of the last call: no labels, no bounds)


def check_column0_against_weighted_gradient(forest, X, y, loss0, what):
    pop, L = forest[0].shape
    wl, _ = hip.tree_SR_weighted_gradient(pop, X.shape[0], L, X.shape[1], 1, *_dev(*forest), *_dev(X, y), None, MSE, 0.0)
    wl = wl.cpu().numpy()
    same = fbits(loss0) == fbits(wl)
    assert same.all(), f"{what}: column 0 and the weighted gradient's MSE differ in {int((~same).sum())} trees, first {np.flatnonzero(~same)[:4].tolist()}: " \
                       f"{loss0[~same][:4]} against {wl[~same][:4]}"


# ---- the fixture forests: the restatement on 100 rows, the truth on 32 ----------------------------------------------------------------
@pytest.mark.parametrize("name", TT.GROUPS)
def test_fixture_forests_meet_the_restatement_and_the_truth(name):
    f = TT.fixture(name)
    assert f.rule.mean() >= TT.FLOORS[name]
    pred, dpred = xgrad(f.forest, f.X, TT.WRT)
    assert_within(dpred, f.d, f.scale, f.rule, f"{name} dpred against the restatement", f"{name} GPU against the restatement (100 rows), worst ratio")
    assert_within(dpred[:, :, :TT.TRUTH_ROWS], f.dT, f.scale[:, :, :TT.TRUTH_ROWS], f.truth_mask, f"{name} dpred against the truth",
                  f"{name} GPU against the truth (32 rows), worst ratio")
    # pred: the tape's forward walk against the register interpreters (the same device library) and against the value truth
    assert_close_classes(pred, batch_evaluate(f.forest, f.X), rtol=1e-5, what=f"{name} pred against batch_evaluate")
    ex.assert_entries(pred[:, :, None], ex.group(name), np.arange(f.X.shape[0]), f"{name} pred of the tape walk")
    y = ex.group(name).labels(np.arange(f.X.shape[0]))
    loss = check_fused_against_materialised(f.forest, f.X, y, (0.5 * f.X).astype(np.float32), TT.WRT, pred, dpred, name)
    check_column0_against_weighted_gradient(f.forest, f.X, y, loss[:, 0], name)


# ---- every path ------------------------------------------------------------------------------------------------------------------------
SETS = {"arith_v3_k1": (ARITH, 3, [2]), "arith_v3_k3": (ARITH, 3, [2, 0, 1]), "all_v12_k3": (ALL_FUNCS, 12, [2, 0, 11]),
        "all_v12_k8": (ALL_FUNCS, 12, [7, 3, 11, 0, 5, 1, 9, 2])}


@functools.lru_cache(maxsize=None)
def path_case(kind, gp_len, D):
    """24 random trees (W up to 4), a dataset and the float64 restatement with its rule: computed once, shared, never written to"""
    import zlib
    funcs, var_len, wrt = SETS[kind]
    rng = np.random.default_rng([20261020, zlib.crc32(kind.encode()), gp_len, D])
    forest = random_forest(rng, 24, gp_len, funcs, var_len, 1, max_depth=5 if gp_len == 64 else 7)
    for t, ops in ((0, (gp_len - 1) // 2), (1, gp_len // 4)):   # rows that fill their storage: n = gp_len - 1 (or gp_len - 2) nodes; half of it
        FI._set(*forest, t, FI._chain(rng, ops, var_len, ARITH if funcs is ARITH else (R.F_ADD, R.F_SUB, R.F_MUL)))
    X = rng.uniform(0.5, 1.5, (D, var_len)).astype(np.float32)
    X[rng.random(X.shape) < 0.3] *= -1.0
    y = (1.5 * X[:, :1] ** 2 - X[:, -1:]).astype(np.float32)
    dy = rng.uniform(-1, 1, (D, len(wrt))).astype(np.float32)
    base = XR.forest_xgrad(*forest, X.astype(np.float64), wrt)
    rule = XR.comparable(*forest, X.astype(np.float64), wrt, base=base) & fits_float32(forest, X, wrt)
    for a in forest + (X, y, dy, rule) + base:
        a.setflags(write=False)
    return forest, X, y, dy, wrt, base, rule


@pytest.mark.parametrize("D", [1, 63, 65, 130, 777])
@pytest.mark.parametrize("gp_len", [64, 96, 1024])
@pytest.mark.parametrize("kind", sorted(SETS))
def test_paths(kind, gp_len, D):
    forest, X, y, dy, wrt, (rp, rd, rs), rule = path_case(kind, gp_len, D)
    what = f"{kind} L={gp_len} D={D}"
    pred, dpred = xgrad(forest, X, wrt)
    assert pred.shape == (24, D) and dpred.shape == (len(wrt), 24, D)
    assert rule.mean() >= 0.5, f"{what}: the rule keeps only {rule.mean():.2f} of the entries"
    assert_within(dpred, rd, rs, rule, what)
    assert_close_classes(pred, batch_evaluate(forest, X), rtol=1e-5, what=f"{what} pred against batch_evaluate")
    loss = check_fused_against_materialised(forest, X, y, dy, wrt, pred, dpred, what)
    check_column0_against_weighted_gradient(forest, X, y, loss[:, 0], what)
    again = xgrad(forest, X, wrt)
    assert np.array_equal(fbits(again[0]), fbits(pred)) and np.array_equal(fbits(again[1]), fbits(dpred)), f"{what}: two calls differ"
    # the order of wrt only permutes the slices
    if len(wrt) > 1:
        perm = list(reversed(range(len(wrt))))
        assert np.array_equal(fbits(xgrad(forest, X, [wrt[k] for k in perm])[1]), fbits(dpred[perm])), f"{what}: wrt reversed"


def test_a_population_that_fills_the_chip_takes_one_wave_per_tree():
    """pop >= 16 x compute units: the plan gives every tree ONE wave (W = 1), which walks the three tiles of D = 130 itself"""
    pop, L, D = 4200, 16, 130
    assert pop >= 16 * torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(4200)
    forest = random_forest(rng, pop, L, ALL_FUNCS, 3, 1, max_depth=3)
    X = rng.uniform(0.5, 1.5, (D, 3)).astype(np.float32)
    y = (X[:, :1] * X[:, 1:2]).astype(np.float32)
    wrt = [2, 0]
    pred, dpred = xgrad(forest, X, wrt)
    sub = np.arange(0, pop, 35)   # the restatement of every 35th tree
    base = XR.forest_xgrad(*(a[sub] for a in forest), X.astype(np.float64), wrt)
    rule = XR.comparable(*(a[sub] for a in forest), X.astype(np.float64), wrt, base=base) & fits_float32(tuple(a[sub] for a in forest), X, wrt)
    assert rule.mean() >= 0.5
    assert_within(dpred[:, sub], base[1], base[2], rule, "W = 1")
    loss = check_fused_against_materialised(forest, X, y, None, wrt, pred, dpred, "W = 1")
    check_column0_against_weighted_gradient(forest, X, y, loss[:, 0], "W = 1")
    # a slice of the forest runs under another plan (W = 3): the materialised arrays do not depend on it
    p2, d2 = xgrad(tuple(a[:24] for a in forest), X, wrt)
    assert np.array_equal(fbits(p2), fbits(pred[:24])) and np.array_equal(fbits(d2), fbits(dpred[:, :24]))


# ---- edge rows among ordinary trees ----------------------------------------------------------------------------------------------------
def test_edge_rows_among_ordinary_trees(rng):
    L, D = 16, 70
    ordinary = [B(R.F_MUL, V(0), V(0)), B(R.F_ADD, V(0), B(R.F_MUL, V(1), C(0.5))), U(R.F_SIN, B(R.F_MUL, V(0), V(1)))]
    edge = [C(np.nan),                                                              # 3: a NaN constant
            B(R.F_DIV, V(0), B(R.F_SUB, V(1), V(1))),                               # 4: x0 / (x1 - x1)
            U(R.F_SQRT, V(0)),                                                      # 5: sqrt(x0), a row at x0 == 0
            IF(C(1.0), V(0), B(R.F_MUL, U(R.F_LOG, C(-1.0)), V(1))),                # 6: an IF whose untaken branch is NaN
            V(1), C(2.5)]                                                           # 7, 8: a VAR root, a CONST-only tree
    exprs = ordinary + edge + ordinary
    value, type_, size = rows(exprs, L)
    n = len(exprs)
    # the three malformed rows of tests/test_gpu_sr_grad.py, appended: too many leaves, size 0, a root missing an operand
    mal = np.zeros((3, L), np.float32), np.zeros((3, L), np.int16), np.zeros((3, L), np.int16)
    mal[0][0, :3], mal[1][0, :3], mal[2][0, :3] = [0, 1, 0.5], [R.T_VAR, R.T_VAR, R.T_CONST], [3, 1, 1]          # three leaves under n = 3
    mal[0][1, 0], mal[1][1, 0], mal[2][1, 0] = 0.5, R.T_CONST, 0                                                # n = 0
    mal[0][2, :2], mal[1][2, :2], mal[2][2, :2] = [R.F_ADD, 0], [R.T_BFUNC, R.T_VAR], [2, 1]                     # x0 + <nothing>
    tail = rows(ordinary, L)
    forest = tuple(np.concatenate([a, m, t]) for a, m, t in zip((value, type_, size), mal, tail))
    X = rng.uniform(0.5, 1.5, (D, 2)).astype(np.float32)
    X[17, 0] = 0.0
    y = (X[:, :1] ** 2).astype(np.float32)
    wrt = [1, 0]
    pred, dpred = xgrad(forest, X, wrt)
    rp, rd, rs = XR.forest_xgrad(*forest, X.astype(np.float64), wrt)
    # the classes (NaN, +inf, -inf, finite) are the restatement's everywhere; the values within the bound where it is finite
    with np.errstate(all="ignore"):
        assert np.array_equal(np.isnan(dpred), np.isnan(rd)) and np.array_equal(np.isposinf(dpred), np.isposinf(rd.astype(np.float32)))
        assert np.array_equal(np.isnan(pred), np.isnan(rp))
    assert_within(dpred, rd, rs, np.isfinite(rd) & np.isfinite(rp)[None], "edge rows")
    m0 = n
    assert np.isnan(pred[m0:m0 + 3]).all() and np.isnan(dpred[:, m0:m0 + 3]).all()          # malformed: NaN in both
    assert np.isnan(pred[3]).all() and not dpred[:, 3].any() and not np.signbit(dpred[:, 3]).any()   # a NaN constant holds no variable: +0.0
    assert np.isnan(pred[4]).all() and np.isnan(dpred[0, 4]).all() and np.isposinf(dpred[1, 4]).all()
    assert pred[5, 17] == 0.0 and np.isposinf(dpred[1, 5, 17]) and np.isfinite(np.delete(dpred[1, 5], 17)).all()
    assert np.array_equal(pred[6], X[:, 0]) and np.array_equal(dpred[1, 6], np.ones(D, np.float32)) and np.isnan(dpred[0, 6]).all()
    assert np.array_equal(dpred[0, 7], np.ones(D, np.float32)) and not dpred[1, 7].any() and not dpred[:, 8].any() and not np.signbit(dpred[:, 8]).any()
    # the neighbours are untouched: the ordinary trees in front, between and behind give the same words
    for a, b in ((0, n - 3), (0, n + 3)):
        assert np.array_equal(fbits(pred[a:a + 3]), fbits(pred[b:b + 3])) and np.array_equal(fbits(dpred[:, a:a + 3]), fbits(dpred[:, b:b + 3]))
    alone = xgrad(rows(ordinary, L), X, wrt)
    assert np.array_equal(fbits(alone[0]), fbits(pred[:3])) and np.array_equal(fbits(alone[1]), fbits(dpred[:, :3]))
    # the fused op: NaN and violation rules
    loss = check_fused_against_materialised(forest, X, y, None, wrt, pred, dpred, "edge rows")
    check_column0_against_weighted_gradient(forest, X, y, loss[:, 0], "edge rows")
    loss, viol = dloss(forest, X, y, None, wrt, [-np.inf, 0.0], [np.inf, 100.0])
    assert np.isnan(loss[m0:m0 + 3]).all() and (viol[m0:m0 + 3] == D).all()                  # malformed: every column NaN, viol = D
    assert np.isnan(loss[3, 0]) and (loss[3, 1:] == 0).all() and (viol[3] == 0).all()        # NaN constant: the prediction column alone
    assert np.isnan(loss[4]).all() and viol[4].tolist() == [D, D]                            # x0 / 0: NaN in x1 counts; +inf in x0 is beyond 100
    assert np.isfinite(loss[5, 0]) and np.isnan(loss[5, 2]) and loss[5, 1] == 0 and viol[5].tolist() == [0, 1]   # sqrt: one inf row
    assert np.isfinite(loss[6, 0]) and np.isnan(loss[6, 1]) and loss[6, 2] == 1.0 and viol[6].tolist() == [D, 0]
    assert np.isfinite(loss[:3]).all() and not viol[:3, 0].any()
    # null bounds: only NaN counts (+inf does not)
    _, v0 = dloss(forest, X, y, None, wrt)
    assert v0[4].tolist() == [D, 0] and v0[5].tolist() == [0, 0] and v0[6].tolist() == [D, 0] and (v0[m0:m0 + 3] == D).all() and not v0[:3].any()


# ---- the binding contract and the forest invariants of the two ops --------------------------------------------------------------------
@pytest.mark.parametrize("op", [XT.GRAD, XT.LOSS])
def test_binding_contract(op):
    XT.BC.test_valid_call_and_one_fault_at_a_time(op)


@pytest.mark.parametrize("op,case", [(op, c) for op in (XT.GRAD, XT.LOSS) for c in FI.cases_for(op)])
def test_op_keeps_the_invariants(op, case):
    FI.check(op, FI.TABLE[op], FI.build_case(case), "cuda")
    torch.cuda.synchronize()


def test_argument_errors_through_the_c_abi_launch_nothing():
    import ctypes as C
    from evogp_amd import _lib
    L = _lib.lib
    forest = _dev(*rows([V(0)] * 4, 8))
    X, y = _dev(np.ones((8, 2), np.float32), np.ones((8, 1), np.float32))
    pred = torch.full((4, 8), 7.0, device="cuda")
    dpred = torch.full((1, 4, 8), 7.0, device="cuda")
    loss, viol = torch.full((4, 2), 7.0, device="cuda"), torch.full((4, 1), 7, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    wrt = lambda *v: (C.c_int * len(v))(*v)  # noqa: E731

    def grad(pop=4, D=8, gp_len=8, var_len=2, out_len=1, n=1, w=wrt(0)):
        return L.evogp_hip_sr_input_gradient(pop, D, gp_len, var_len, out_len, *(p(a) for a in forest), p(X), n, w, p(pred), p(dpred), None)

    def dl(pop=4, D=8, gp_len=8, var_len=2, out_len=1, n=1, w=wrt(0)):
        return L.evogp_hip_sr_derivative_loss(pop, D, gp_len, var_len, out_len, *(p(a) for a in forest), p(X), p(y), None, n, w, None, None,
                                              p(loss), p(viol), None)

    for f in (grad, dl):
        for bad in (dict(pop=0), dict(D=0), dict(gp_len=0), dict(gp_len=1025), dict(var_len=0), dict(out_len=0), dict(n=0),
                    dict(n=9, w=wrt(*range(9))), dict(w=wrt(2)), dict(w=wrt(-1)), dict(n=2, w=wrt(1, 1))):
            assert f(**bad) == -1, (f.__name__, bad)
        assert f(w=None) == -2 and f(out_len=2) == -3
    torch.cuda.synchronize()
    assert (pred == 7).all() and (dpred == 7).all() and (loss == 7).all() and (viol == 7).all()   # nothing was launched
    assert grad() == 0 and dl() == 0
    torch.cuda.synchronize()
    assert (pred == 1).all() and (dpred == 1).all() and (loss[:, 0] == 0).all() and (loss[:, 1] == 1).all() and (viol == 0).all()


# ---- Forest and SymbolicRegression end to end ---------------------------------------------------------------------------------------
def _target(rng, D=256):
    X = rng.uniform(-2, 2, (D, 2)).astype(np.float32)
    y = (X[:, :1] ** 2 + np.sin(X[:, 1:2])).astype(np.float32)
    dy = np.stack([2 * X[:, 0], np.cos(X[:, 1])], 1).astype(np.float32)
    return _dev(X, y, dy)


def _descriptor():
    return GenerateDescriptor(max_tree_len=32, input_len=2, output_len=1, using_funcs=["+", "-", "*", "sin"], max_layer_cnt=4, const_samples=[-1, 0, 1, 2])


def test_forest_methods_on_a_200_tree_forest(rng):
    X, y, dy = _target(rng)
    forest = Forest.random_generate(200, _descriptor(), keys=torch.tensor([3, 4], dtype=torch.uint32, device="cuda"))
    pred, grad = forest.SR_input_gradients(X)
    assert pred.shape == (200, 256) and grad.shape == (200, 256, 2) and grad.stride() == (256, 1, 200 * 256)
    assert torch.equal(pred.view(torch.int32), forest.batch_forward(X)[:, :, 0].contiguous().view(torch.int32)) or \
        torch.allclose(pred, forest.batch_forward(X)[:, :, 0], rtol=1e-5, equal_nan=True)
    loss, viol = forest.SR_derivative_loss(X, y, dy, bounds={0: (-4.5, 4.5)})
    want_loss, want_viol = XR.loss_columns(pred.cpu().numpy(), grad.permute(2, 0, 1).contiguous().cpu().numpy(), y.cpu().numpy(), dy.cpu().numpy(),
                                           [-4.5, -np.inf], [4.5, np.inf])
    assert np.array_equal(viol.cpu().numpy(), want_viol) and 0 < (want_viol[:, 0] > 0).sum() < 200
    np.testing.assert_allclose(loss.cpu().numpy(), want_loss, rtol=2e-7, equal_nan=True)
    sens, _ = forest.SR_derivative_loss(X, y)   # no labels: the mean squared sensitivity
    np.testing.assert_allclose(sens[:, 1:].cpu().numpy(), (grad.double() ** 2).mean(1).cpu().numpy(), rtol=2e-7, equal_nan=True)


def _pipeline(problem):
    d = _descriptor()
    algo = GeneticProgramming(Forest.random_generate(200, d, keys=torch.tensor([1, 2], dtype=torch.uint32, device="cuda")),
                              DefaultCrossover(), DefaultMutation(0.2, d), DefaultSelection(0.3, 2))
    return StandardPipeline(algo, problem, generation_limit=3, is_show_details=False), algo


def test_three_generations_with_derivative_labels(rng):
    X, y, dy = _target(rng)
    prob = SymbolicRegression(datapoints=X, labels=y, derivative_labels=dy, derivative_weight=[0.5, 2.0], sampled_monotonic={0: (-4.5, 4.5)})
    pipe, algo = _pipeline(prob)
    best = pipe.run()
    assert best is pipe.best_tree and np.isfinite(float(pipe.best_fitness))
    forest = algo.forest
    loss, viol = prob.derivative_loss(forest)
    want = -(loss[:, 0] + (0.5 * loss[:, 1] + 2.0 * loss[:, 2]))
    ninf = torch.full_like(want, float("-inf"))
    want = torch.where(torch.isnan(want) | (viol[:, 0] != 0), ninf, want)
    assert torch.equal(prob.scores(forest), want) and torch.isfinite(want).any()
    one = Forest(2, 1, *(x[None].contiguous() for x in (best.node_value, best.node_type, best.subtree_size)))
    bl, bv = prob.derivative_loss(one)
    assert int(bv[0, 0]) == 0 and float(-(bl[0, 0] + (0.5 * bl[0, 1] + 2.0 * bl[0, 2]))) == float(pipe.best_fitness)


def test_three_generations_with_a_sampled_constraint_alone(rng):
    X, y, dy = _target(rng)
    prob = SymbolicRegression(datapoints=X, labels=y, sampled_monotonic={0: +1})
    plain = SymbolicRegression(datapoints=X, labels=y)
    pipe, algo = _pipeline(prob)
    first = algo.forest
    viol = prob.derivative_loss(first)[1]
    sc, sc0 = prob.scores(first), plain.scores(first)
    obeys = viol[:, 0] == 0
    assert torch.equal(sc[obeys], sc0[obeys]) and (sc[~obeys] == float("-inf")).all() and obeys.any() and (~obeys).any()   # it only masks
    best = pipe.run()
    one = Forest(2, 1, *(x[None].contiguous() for x in (best.node_value, best.node_type, best.subtree_size)))
    assert int(prob.derivative_loss(one)[1][0, 0]) == 0 and np.isfinite(float(pipe.best_fitness))   # the best tree never falls in x0 on the data
    assert float(plain.scores(one)[0]) == float(pipe.best_fitness)


def test_write_report():
    TT.write_report(REPORT)
    assert all(r <= 1.0 for r in REPORT.values())
