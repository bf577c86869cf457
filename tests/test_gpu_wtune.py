"""GPU: constant tuning under sample weights, robust losses and held-out rows -- the weighted builds of the two tape kernels
(csrc/sr_grad.hip, csrc/sr_lm.hip; evogp_hip_sr_weighted_gradient / evogp_hip_sr_weighted_normal_eq) against the float64 reference
(tests/weighted_grad_ref.py), their rules for rows without weight, unusable weight rows and non-finite predictions, their agreement
with the scorer (Forest.SR_weighted_loss), Forest.optimize_constants(weights=, loss=, param=) on the device, and the two planted
problems of tests/wtune_cases.py through StandardPipeline.step."""
import os
import sys

import numpy as np
import pytest
import torch

import evogp_amd  # noqa: F401  (registers the ops)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sr_grad_ref as R  # noqa: E402
import sr_lm_ref as LM  # noqa: E402
import test_gpu_binding_contract as BC  # noqa: E402
import weighted_grad_ref as WG  # noqa: E402
import weighted_loss_ref as WL  # noqa: E402
import wtune_cases as C  # noqa: E402
from grad_trees import ALL_FUNCS, random_forest  # noqa: E402

pytestmark = pytest.mark.gpu

NTRI = len(LM.TRI)


# The two new ops join the binding-contract table (tests/test_gpu_binding_contract.py: one row per op, every argument faulted in turn;
# its test_the_table_covers_every_op reads the table when it runs).  The rows are checked below, by that module's own test body.
def _wgrad_row(kind, param, faulty_params):
    return dict(args=BC._data_head(1, use_mse=False) + BC._forest() + BC._xy() + [BC._f("weights", BC.D), ("loss_kind", kind), ("loss_param", param)],
                outs=[((BC.POP,), BC.F32), ((BC.POP, BC.L), BC.F32)],
                scalars=dict(BC.SIZES, out_len=(0, 2), loss_kind=(-1, 5), loss_param=faulty_params),
                also=[("no weights", {"weights": None}, [((BC.POP,), BC.F32), ((BC.POP, BC.L), BC.F32)])])


_WGRAD, _WNEQ = "evogp_hip::tree_SR_weighted_gradient", "evogp_hip::tree_SR_weighted_normal_eq"
_WGRAD_ROWS = {"mse": (0, 0.0, (float("nan"),)), "huber": (2, 1.0, (0.0, -1.0, float("inf"), float("nan"))),
               "pinball": (3, 0.5, (0.0, 1.0, float("nan"))), "logcosh": (4, 0.0, (float("nan"),))}
BC.TABLE[_WGRAD] = lambda: _wgrad_row(*_WGRAD_ROWS["mse"])
BC.TABLE[_WNEQ] = lambda: dict(args=BC._data_head(1, use_mse=False) + BC._forest() + BC._xy() + [BC._f("weights", BC.D)],
                               outs=[((BC.POP,), BC.F32), ((BC.POP, BC.NORMAL), BC.F32)], scalars=dict(BC.SIZES, out_len=(0, 2)),
                               also=[("no weights", {"weights": None}, [((BC.POP,), BC.F32), ((BC.POP, BC.NORMAL), BC.F32)])])


@pytest.mark.parametrize("kind", sorted(_WGRAD_ROWS))
def test_binding_contract_of_the_weighted_gradient(kind, monkeypatch):
    monkeypatch.setitem(BC.TABLE, _WGRAD, lambda: _wgrad_row(*_WGRAD_ROWS[kind]))
    BC.test_valid_call_and_one_fault_at_a_time(_WGRAD)


def test_binding_contract_of_the_weighted_normal_equations():
    BC.test_valid_call_and_one_fault_at_a_time(_WNEQ)


def _dev(*arrs):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _wgrad(value, type_, size, X, y, w, kind="mse", param=None):
    v, t, s, Xd, yd, wd = _dev(value, type_, size, X, y, w)
    pop, L = value.shape
    loss, grad = torch.ops.evogp_hip.tree_SR_weighted_gradient(pop, X.shape[0], L, X.shape[1], 1, v, t, s, Xd, yd, wd, WL.KINDS[kind],
                                                               0.0 if param is None else param)
    assert loss.shape == (pop,) and grad.shape == (pop, L)
    return loss.cpu().numpy(), grad.cpu().numpy()


def _wnormal(value, type_, size, X, y, w):
    v, t, s, Xd, yd, wd = _dev(value, type_, size, X, y, w)
    pop, L = value.shape
    loss, normal = torch.ops.evogp_hip.tree_SR_weighted_normal_eq(pop, X.shape[0], L, X.shape[1], 1, v, t, s, Xd, yd, wd)
    assert loss.shape == (pop,) and normal.shape == (pop, LM.WORDS)
    return loss.cpu().numpy(), normal.cpu().numpy()


def _u(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return all(np.array_equal(_u(x), _u(y)) for x, y in zip(a, b))


def _check_grad(want_loss, want, gabs, stable, loss, grad, need=0.5):
    """the bounds of test_gradient_matches_float64_reference on the comparable trees"""
    assert stable.mean() >= need, f"only {stable.sum()} of {len(stable)} trees are comparable"
    for t in np.flatnonzero(stable):
        ok = np.isfinite(want[t]) & np.isfinite(gabs[t])
        err = np.abs(grad[t][ok].astype(np.float64) - want[t][ok])
        bound = 1e-3 * gabs[t][ok] + 1e-7
        worst = np.argmax(err - bound)
        assert (err <= bound).all(), (t, np.flatnonzero(ok)[worst], grad[t][ok][worst], want[t][ok][worst])
        assert np.isfinite(loss[t]) and abs(loss[t] - want_loss[t]) <= 1e-4 * abs(want_loss[t]) + 1e-6, (t, loss[t], want_loss[t])


def _check_normal(type_, size, want_loss, want, nabs, stable, loss, normal, gloss, grad, need=0.5):
    """the bounds of tests/test_gpu_sr_lm.py, the loss against the weighted gradient's bit for bit"""
    assert stable.mean() >= need, f"only {stable.sum()} of {len(stable)} trees are comparable"
    assert np.array_equal(_u(loss), _u(gloss)), "the two passes sum the same rows in the same order"
    for t in np.flatnonzero(stable):
        ok = np.isfinite(want[t]) & np.isfinite(nabs[t])
        err = np.abs(normal[t][ok].astype(np.float64) - want[t][ok])
        bound = 1e-3 * nabs[t][ok] + 1e-7
        worst = np.argmax(err - bound)
        assert (err <= bound).all(), (t, np.flatnonzero(ok)[worst], normal[t][ok][worst], want[t][ok][worst])
        assert np.isfinite(loss[t]) and abs(loss[t] - want_loss[t]) <= 1e-4 * abs(want_loss[t]), (t, loss[t], want_loss[t])
        cidx = LM.optimised_consts(type_[t], size[t])
        for j, c in enumerate(cidx):   # b is half the gradient of the loss at the optimised constants
            if c >= 0 and ok[NTRI + j] and np.isfinite(grad[t, c]):
                assert abs(float(normal[t, NTRI + j]) - float(grad[t, c]) / 2) <= 1e-3 * nabs[t, NTRI + j] + 1e-7, (t, j)


# ---- 1, 2. the two passes against the float64 reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("funcs,gp_len,D", WG.CASES)
def test_weighted_gradient_matches_float64_reference(oracle, funcs, gp_len, D):
    value, type_, size, X, y, w = WG.make_case(funcs, gp_len, D)
    for kind, param in WG.KINDS:
        loss, grad = _wgrad(value, type_, size, X, y, w, kind, param)
        _check_grad(*WG.comparable_grad(oracle, value, type_, size, X, y, w, kind, param), loss, grad)


@pytest.mark.parametrize("funcs,gp_len,D", WG.CASES)
def test_weighted_normal_equations_match_float64_reference(oracle, funcs, gp_len, D):
    value, type_, size, X, y, w = WG.make_case(funcs, gp_len, D)
    loss, normal = _wnormal(value, type_, size, X, y, w)
    gloss, grad = _wgrad(value, type_, size, X, y, w, "mse")
    _check_normal(type_, size, *WG.comparable_normal(oracle, value, type_, size, X, y, w), loss, normal, gloss, grad)


# ---- 3. one wave per tree: the geometry of a population that fills the chip --------------------------------------------------------
def test_one_wave_per_tree(oracle):
    pop, n, gp_len, D = 4100, 64, 16, 130
    assert pop >= 16 * torch.cuda.get_device_properties(0).multi_processor_count, "the population must fill the chip"
    rng = np.random.default_rng(20261021)
    value, type_, size = random_forest(rng, n, gp_len, ALL_FUNCS, 3, 1, max_depth=3)
    X = rng.uniform(0.5, 1.5, (D, 3)).astype(np.float32)
    y = rng.uniform(-1, 1, (D, 1)).astype(np.float32)
    w = rng.uniform(0.5, 2, D).astype(np.float32)
    w[rng.random(D) < 0.3] = 0
    reps = -(-pop // n)
    tiled = [np.tile(a, (reps, 1))[:pop] for a in (value, type_, size)]
    loss, normal = _wnormal(*tiled, X, y, w)
    gloss, grad = _wgrad(*tiled, X, y, w, "mse")
    _check_grad(*WG.comparable_grad(oracle, value, type_, size, X, y, w, "mse", None), gloss[:n], grad[:n])
    _check_normal(type_, size, *WG.comparable_normal(oracle, value, type_, size, X, y, w), loss[:n], normal[:n], gloss[:n], grad[:n])
    hloss, hgrad = _wgrad(*tiled, X, y, w, "huber", 0.5)
    _check_grad(*WG.comparable_grad(oracle, value, type_, size, X, y, w, "huber", 0.5), hloss[:n], hgrad[:n])
    for a in (loss, normal, gloss, grad, hloss, hgrad):   # every copy of a tree gets its bits
        assert np.array_equal(_u(a[n:2 * n]), _u(a[:n])) and np.array_equal(_u(a[pop - n:]), _u(a[(pop - n) % n:][:n]))


# ---- 4. rows without weight are not looked at --------------------------------------------------------------------------------------
def _case300(rng):
    value, type_, size = random_forest(rng, 24, 64, ALL_FUNCS, 3, 1, max_depth=5)
    X = rng.uniform(0.5, 1.5, (300, 3)).astype(np.float32)
    y = rng.uniform(-1, 1, (300, 1)).astype(np.float32)
    w = rng.uniform(0.5, 2, 300).astype(np.float32)
    return value, type_, size, X, y, w


def test_zero_weight_rows_are_not_looked_at(rng):
    value, type_, size, X, y, w = _case300(rng)
    value[2, :2], type_[2, :2], size[2, :2] = [R.F_INV, 0], [R.T_UFUNC, R.T_VAR], [2, 1]   # 1 / x0: NaN at x0 = 0 and nowhere else
    X2 = np.concatenate([X, np.zeros((200, 3), np.float32)])   # x = 0 under /, log, inv: NaN and inf in many trees
    y2 = np.concatenate([y, rng.uniform(-1, 1, (200, 1)).astype(np.float32)])
    w2 = np.concatenate([w, np.zeros(200, np.float32)])
    plain = _wgrad(value, type_, size, X2, y2, np.ones(500, np.float32))[0]
    assert np.isnan(plain).sum() >= 4, "the appended rows must break some trees when they carry weight"
    for kind, param in WG.KINDS:
        a, b = _wgrad(value, type_, size, X, y, w, kind, param), _wgrad(value, type_, size, X2, y2, w2, kind, param)
        assert np.isfinite(a[0]).sum() >= 12 and _same(a, b), kind
    assert _same(_wnormal(value, type_, size, X, y, w), _wnormal(value, type_, size, X2, y2, w2))
    # the reverse: a zero on the one row where a tree is NaN makes its loss finite
    X3 = X.copy()
    X3[70] = 0.0
    l_with = _wgrad(value, type_, size, X3, y, w)[0]
    w3 = w.copy()
    w3[70] = 0.0
    l_without, g_without = _wgrad(value, type_, size, X3, y, w3)
    healed = np.isnan(l_with) & np.isfinite(l_without)
    assert healed[2] and not (np.isfinite(l_with) & ~np.isfinite(l_without)).any()
    assert np.isfinite(g_without[healed]).all()
    n_with, n_without = _wnormal(value, type_, size, X3, y, w)[0], _wnormal(value, type_, size, X3, y, w3)[0]
    assert np.array_equal(np.isnan(n_with), np.isnan(l_with)) and np.array_equal(_u(n_without), _u(l_without))


# ---- 5. scale invariance --------------------------------------------------------------------------------------------------------------
def test_weights_times_four_change_no_bit(rng):
    value, type_, size, X, y, w = _case300(rng)
    w[rng.random(300) < 0.3] = 0
    for kind, param in WG.KINDS:
        assert _same(_wgrad(value, type_, size, X, y, w, kind, param), _wgrad(value, type_, size, X, y, 4 * w, kind, param)), kind
    assert _same(_wnormal(value, type_, size, X, y, w), _wnormal(value, type_, size, X, y, 4 * w))


# ---- 6. NaN rules, layout, determinism ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gp_len", [64, 128])
def test_nan_rules_layout_and_determinism(rng, gp_len):
    pop, D = 40, 200
    value, type_, size = random_forest(rng, pop, gp_len, ALL_FUNCS, 3, 1, max_depth=5)
    X = rng.uniform(0.5, 1.5, (D, 3)).astype(np.float32)
    y = rng.uniform(-1, 1, (D, 1)).astype(np.float32)
    w = rng.uniform(0.5, 2, D).astype(np.float32)
    w[rng.random(D) < 0.3] = 0
    w[17] = 1.0
    for bad in (np.where(np.arange(D) == 3, -1.0, w), np.where(np.arange(D) == 3, np.nan, w), np.where(np.arange(D) == 3, np.inf, w),
                np.zeros(D)):
        bad = bad.astype(np.float32)
        for kind, param in (("mse", None), ("logcosh", None)):
            loss, grad = _wgrad(value, type_, size, X, y, bad, kind, param)
            assert np.isnan(loss).all() and not _u(grad).any()
        loss, normal = _wnormal(value, type_, size, X, y, bad)
        assert np.isnan(loss).all() and not _u(normal).any()
    clean = _wgrad(value, type_, size, X, y, w, "huber", 0.5), _wnormal(value, type_, size, X, y, w)
    size[9, 0] = 0                                    # empty tree
    value[11, 0], type_[11, 0] = R.F_ADD, R.T_BFUNC   # the root now pops a missing operand
    size[11, 0] = 1
    value[13, :3], type_[13, :3], size[13, :3] = [R.F_INV, R.F_SUB, 0], [R.T_UFUNC, R.T_BFUNC, R.T_VAR], [4, 3, 1]   # 1 / (x0 - c):
    value[13, 3], type_[13, 3], size[13, 3] = X[17, 0], R.T_CONST, 1                     # NaN on row 17, which carries weight
    (loss, grad), (nloss, normal) = _wgrad(value, type_, size, X, y, w, "huber", 0.5), _wnormal(value, type_, size, X, y, w)
    again = _wgrad(value, type_, size, X, y, w, "huber", 0.5), _wnormal(value, type_, size, X, y, w)
    assert _same((loss, grad), again[0]) and _same((nloss, normal), again[1])
    for t in (9, 11, 13):
        assert np.isnan(loss[t]) and not _u(grad[t]).any() and np.isnan(nloss[t]) and not _u(normal[t]).any()
    others = np.setdiff1d(np.arange(pop), [9, 11, 13])
    assert _same([a[others] for a in (loss, grad, nloss, normal)], [a[others] for a in (*clean[0], *clean[1])])
    w0 = w.copy()
    w0[17] = 0.0
    assert np.isfinite(_wgrad(value, type_, size, X, y, w0, "huber", 0.5)[0][13])   # (without weight the pole is not looked at)
    for t in range(pop):
        n = min(max(int(size[t, 0]), 0), gp_len)
        is_c = type_[t].astype(np.int32) == R.T_CONST
        is_c[n:] = False
        assert np.all(_u(grad[t][~is_c]) == 0)
        nc = int((LM.optimised_consts(type_[t], size[t]) >= 0).sum())
        absent = np.array([i >= nc or j >= nc for i, j in LM.TRI] + [i >= nc for i in range(LM.K)])
        assert np.all(_u(normal[t][absent]) == 0), t


# ---- 7. agreement with the scorer -------------------------------------------------------------------------------------------------------
def scorer_agreement(seed=20261022, pop=200, D=300):
    """per kind: the largest |op loss - SR_weighted_loss| relative to the loss over the trees both give a finite loss, the number of
    those trees, and the trees on which one is NaN and the other is not"""
    from evogp_amd.tree import Forest

    rng = np.random.default_rng(seed)
    value, type_, size = random_forest(rng, pop, 64, ALL_FUNCS, 3, 1, max_depth=5)
    X = rng.uniform(0.5, 1.5, (D, 3)).astype(np.float32)
    y = rng.uniform(-1, 1, (D, 1)).astype(np.float32)
    w = rng.uniform(0.5, 2, D).astype(np.float32)
    w[rng.random(D) < 0.3] = 0
    v, t, s, Xd, yd, wd = _dev(value, type_, size, X, y, w)
    forest = Forest(3, 1, v, t, s)
    out = {}
    for kind, param in WG.KINDS:
        got = _wgrad(value, type_, size, X, y, w, kind, param)[0].astype(np.float64)
        ref = forest.SR_weighted_loss(Xd, yd, wd, kind, param).cpu().numpy().astype(np.float64)
        both = np.isfinite(got) & np.isfinite(ref)
        with np.errstate(all="ignore"):
            rel = np.abs(got - ref)[both] / np.abs(ref[both])
        out[kind] = dict(finite_in_both=int(both.sum()), nan_in_one_only=int((np.isnan(got) != np.isnan(ref)).sum()),
                         max_rel_diff=float(rel.max(initial=0.0)), ref_tolerance=WL.tolerance(D, kind),
                         within_bound=bool((np.abs(got - ref)[both] <= 1e-4 * np.abs(ref[both]) + 1e-6).all()))
    return out


def test_loss_agrees_with_the_scorer():
    for kind, r in scorer_agreement().items():
        print(kind, r)
        assert r["finite_in_both"] >= 100 and r["within_bound"], (kind, r)


# ---- 8. tuning invariants on the device -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,param", WG.KINDS)
def test_optimize_constants_invariants(rng, kind, param):
    from evogp_amd.tree import Forest

    value, type_, size = random_forest(rng, 100, 64, ALL_FUNCS, 3, 1, max_depth=5)
    value[60:], type_[60:], size[60:] = value[:40], type_[:40], size[:40]   # duplicates for dedup
    size[5, 0] = 0
    X = rng.uniform(0.5, 1.5, (300, 3)).astype(np.float32)
    y = rng.uniform(-1, 1, (300, 1)).astype(np.float32)
    w = rng.uniform(0.5, 2, 300).astype(np.float32)
    w[rng.random(300) < 0.3] = 0
    v, t, s, Xd, yd, wd = _dev(value, type_, size, X, y, w)
    f0 = Forest(3, 1, v, t, s)
    before = f0.SR_gradient(Xd, yd, weights=wd, loss=kind, param=param)[0].cpu().numpy()
    f1, loss1 = f0.optimize_constants(Xd, yd, steps=8, weights=wd, loss=kind, param=param)
    f2, loss2 = f0.optimize_constants(Xd, yd, steps=8, weights=wd, loss=kind, param=param, dedup=True)
    assert torch.equal(f0.batch_node_value, v) and torch.equal(f1.batch_node_type, t) and torch.equal(f1.batch_subtree_size, s)
    assert _same((f1.batch_node_value.cpu().numpy(), loss1.cpu().numpy()), (f2.batch_node_value.cpu().numpy(), loss2.cpu().numpy()))
    after = loss1.cpu().numpy()
    fin = ~np.isnan(before)
    assert np.isnan(before[5]) and fin.sum() >= 50
    assert np.array_equal(np.isnan(after), np.isnan(before)) and np.all(after[fin] <= before[fin]) and (after[fin] < before[fin]).mean() > 0.2
    v1 = f1.batch_node_value.cpu().numpy()
    is_c = (type_ == R.T_CONST) & (np.arange(64)[None, :] < np.clip(size[:, :1], 0, 64))
    assert np.array_equal(_u(value)[~is_c], _u(v1)[~is_c]) and np.array_equal(_u(value)[~fin], _u(v1)[~fin])
    if kind == "mse":   # Levenberg-Marquardt on the weighted normal equations
        start = f0.SR_normal_equations(Xd, yd, weights=wd)[0].cpu().numpy()
        assert np.array_equal(_u(start), _u(before))
        g1, l1 = f0.optimize_constants(Xd, yd, steps=8, method="lm", weights=wd)
        g2, l2 = f0.optimize_constants(Xd, yd, steps=8, method="lm", weights=wd, dedup=True)
        assert _same((g1.batch_node_value.cpu().numpy(), l1.cpu().numpy()), (g2.batch_node_value.cpu().numpy(), l2.cpu().numpy()))
        l1 = l1.cpu().numpy()
        assert np.array_equal(np.isnan(l1), np.isnan(before)) and np.all(l1[fin] <= before[fin])
        assert np.array_equal(_u(value)[~is_c], _u(g1.batch_node_value.cpu().numpy())[~is_c])


def test_keywords_left_at_none_are_the_unweighted_call(rng):
    from evogp_amd.tree import Forest

    value, type_, size = random_forest(rng, 60, 64, ALL_FUNCS, 3, 1, max_depth=5)
    X = rng.uniform(0.5, 1.5, (200, 3)).astype(np.float32)
    y = rng.uniform(-1, 1, (200, 1)).astype(np.float32)
    v, t, s, Xd, yd = _dev(value, type_, size, X, y)
    f0 = Forest(3, 1, v, t, s)
    for method in ("descent", "lm"):
        a = f0.optimize_constants(Xd, yd, steps=4, method=method)
        b = f0.optimize_constants(Xd, yd, steps=4, method=method, weights=None, loss=None, param=None)
        assert torch.equal(a[0].batch_node_value.view(torch.int32), b[0].batch_node_value.view(torch.int32))
        assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    loss, grad = torch.ops.evogp_hip.tree_SR_gradient(60, 200, 64, 3, 1, True, v, t, s, Xd, yd)
    l2, g2 = f0.SR_gradient(Xd, yd, weights=None, loss=None, param=None)
    assert torch.equal(loss.view(torch.int32), l2.view(torch.int32)) and torch.equal(grad.view(torch.int32), g2.view(torch.int32))


# ---- 9. the planted problems on the device ----------------------------------------------------------------------------------------------
def test_held_out_rows_are_not_leaked():
    from evogp_amd.tree import Forest

    X, y, m = C.held_out_data()
    c = C.tuned_constants("cuda", X, y, validation_mask=torch.from_numpy(m), const_opt_steps=C.HELD_OUT_STEPS, const_opt_method="lm",
                          const_opt_loss="problem")
    assert C.distance(c) <= C.BOUND, c
    f = Forest(1, 1, *_dev(*C.planted_arrays()))
    leak = f.optimize_constants(*_dev(X, y), steps=C.HELD_OUT_STEPS, method="lm")[0]
    assert C.distance(leak.batch_node_value.cpu().numpy()[0, [2, 4]]) > C.BOUND


def test_robust_tuning_resists_outliers():
    X, y = C.robust_data()
    huber = C.tuned_constants("cuda", X, y, loss="huber", loss_param=1.0, const_opt_steps=C.ROBUST_STEPS, const_opt_loss="problem")
    mse = C.tuned_constants("cuda", X, y, loss="mse", const_opt_steps=C.ROBUST_STEPS, const_opt_loss="problem")
    assert C.distance(huber) < C.distance(mse), (huber, mse)
