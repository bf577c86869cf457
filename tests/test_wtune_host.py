"""CPU: constant tuning under sample weights, robust losses and held-out rows.  The float64 reference (tests/weighted_grad_ref.py)
against the references it is built on; the host logic of Forest.SR_gradient / SR_normal_equations / optimize_constants(weights=,
loss=, param=) and SymbolicRegression(const_opt_loss="problem") with that reference registered as test-only CPU kernels
(tests/cpu_wgrad_ops.py); the two planted problems through StandardPipeline.step; and the argument checks of the two new C entry
points, which return before any launch."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cpu_dedup_ops  # noqa: E402
import cpu_grad_ops  # noqa: E402
import cpu_lm_ops  # noqa: E402
import cpu_ops  # noqa: E402
import cpu_wgrad_ops  # noqa: E402
import cpu_wloss_ops  # noqa: E402
import sr_grad_ref as R  # noqa: E402
import sr_lm_ref as LM  # noqa: E402
import weighted_grad_ref as WG  # noqa: E402
import weighted_loss_ref as WL  # noqa: E402
import wtune_cases as C  # noqa: E402
from grad_trees import ALL_FUNCS, ARITH, random_forest  # noqa: E402

for _m in (cpu_ops, cpu_grad_ops, cpu_lm_ops, cpu_dedup_ops, cpu_wloss_ops, cpu_wgrad_ops):
    _m.register()

from evogp_amd.problem import SymbolicRegression  # noqa: E402
from evogp_amd.tree import Forest, set_default_device  # noqa: E402
from evogp_amd.tree import utils as _tree_utils  # noqa: E402

D = 40


@pytest.fixture(autouse=True)
def _cpu_default_device():
    saved = _tree_utils._DEVICE
    set_default_device("cpu")
    yield
    _tree_utils._DEVICE = saved


def _case(rng, funcs=ALL_FUNCS, pop=30, out_len=1):
    value, type_, size = random_forest(rng, pop, 32, funcs, 2, out_len, max_depth=4)
    X = rng.uniform(0.5, 1.5, (D, 2)).astype(np.float32)
    y = rng.uniform(-1, 1, (D, out_len)).astype(np.float32)
    return value, type_, size, X, y


def _forest(value, type_, size, out_len=1):
    return Forest(2, out_len, *(torch.from_numpy(a) for a in (value, type_, size)))


def _bits(t):
    return t.contiguous().numpy().view(np.uint32)


# ---- 1. the reference against the references it is built on --------------------------------------------------------------------------
@pytest.mark.parametrize("funcs", ["arith", "all"])
def test_unit_weights_are_the_unweighted_reference(rng, funcs):
    value, type_, size, X, y = _case(rng, ARITH if funcs == "arith" else ALL_FUNCS)
    size[3, 0] = 0
    for kind, use_mse in (("mse", True), ("mae", False)):
        with np.errstate(all="ignore"):
            want_loss, want, wabs = R.forest_grad(value, type_, size, X, y, use_mse)
        for w in (None, np.ones(D, np.float32), np.full(D, 0.25, np.float32)):
            loss, grad, gabs = WG.forest_wgrad(value, type_, size, X, y, w, kind)
            fin = np.isfinite(loss)   # (a float32-infinite prediction is NaN here and passes through there)
            assert fin.sum() >= 20 and np.isnan(loss[3]) and not grad[3].any()
            np.testing.assert_allclose(loss[fin], want_loss[fin], rtol=1e-12)
            ok = fin[:, None] & np.isfinite(want) & np.isfinite(wabs)
            assert np.all(np.abs(grad - want)[ok] <= 1e-12 * wabs[ok])
            np.testing.assert_allclose(gabs[ok], wabs[ok], rtol=1e-12)
    # ... and the normal equations those of sr_lm_ref
    with np.errstate(all="ignore"):
        want_loss, want, wabs = LM.forest_normal_eq(value, type_, size, X, y)
    loss, normal, nabs = WG.forest_wnormal_eq(value, type_, size, X, y, None)
    fin = np.isfinite(loss)
    np.testing.assert_allclose(loss[fin], want_loss[fin], rtol=1e-12)
    ok = fin[:, None] & np.isfinite(want) & np.isfinite(wabs)
    assert np.all(np.abs(normal - want)[ok] <= 1e-12 * wabs[ok])


def _loss64(value, type_, size, X, y, w, kind, param):
    """weighted_loss_ref's loss of one tree from float64 predictions (its rho, not rounded to float32)"""
    pred, _ = WG.tree_adjoints(value, type_, size, X)
    return float(np.sum(w * WL.rho(pred - y.reshape(-1).astype(np.float64), kind, param)) / np.sum(w))


def test_gradient_is_the_finite_difference_of_the_weighted_loss(rng):
    # c1 * sin(c2 * x0) + c3 and (c1 * x0 + c2) / (x1 + c3): smooth in their constants on these rows, residuals away from 0
    C_, V, U, B = R.T_CONST, R.T_VAR, R.T_UFUNC, R.T_BFUNC
    trees = [[(R.F_ADD, B, 8), (R.F_MUL, B, 6), (1.2, C_, 1), (R.F_SIN, U, 4), (R.F_MUL, B, 3), (1.5, C_, 1), (0, V, 1), (0.3, C_, 1)],
             [(R.F_DIV, B, 9), (R.F_ADD, B, 5), (R.F_MUL, B, 3), (0.8, C_, 1), (0, V, 1), (-0.4, C_, 1), (R.F_ADD, B, 3), (1, V, 1), (2.0, C_, 1)]]
    X = rng.uniform(0.5, 1.5, (D, 2)).astype(np.float32)
    y = rng.uniform(3, 4, (D, 1)).astype(np.float32)   # every residual is negative and larger than the Huber delta
    y[::2] -= 6                                        # ... or positive
    w = rng.uniform(0.5, 2, D).astype(np.float32)
    w[rng.random(D) < 0.3] = 0
    for nodes in trees:
        value, type_, size = np.zeros((1, 16), np.float32), np.zeros((1, 16), np.int16), np.zeros((1, 16), np.int16)
        for i, (v, t, s) in enumerate(nodes):
            value[0, i], type_[0, i], size[0, i] = v, t, s
        for kind, param in WG.KINDS + [("huber", 50.0)]:   # (the last: every residual inside delta)
            loss, grad, _ = WG.forest_wgrad(value, type_, size, X, y, w, kind, param)
            assert abs(loss[0] - _loss64(value[0].astype(np.float64), type_[0], size[0], X, y, w.astype(np.float64), kind, param)) <= 1e-12 * loss[0]
            for i in np.flatnonzero(type_[0] == C_):
                h = 2.0 ** -10   # (node values are float32: c +- h is exact there; the central difference is off by O(h^2))
                lo, hi = value[0].copy(), value[0].copy()
                lo[i] -= np.float32(h)
                hi[i] += np.float32(h)
                assert float(hi[i]) - float(lo[i]) == 2 * h
                fd = (_loss64(hi, type_[0], size[0], X, y, w.astype(np.float64), kind, param) -
                      _loss64(lo, type_[0], size[0], X, y, w.astype(np.float64), kind, param)) / (2 * h)
                assert abs(fd - grad[0, i]) <= 2e-5 * max(1.0, abs(fd)), (kind, i, fd, grad[0, i])


def test_zero_one_weights_are_the_kept_rows(rng):
    value, type_, size, X, y = _case(rng)
    keep = rng.random(D) < 0.6
    X0 = X.copy()
    X0[~keep] = 0.0   # rows on which many trees are NaN or infinite: they are not looked at
    with np.errstate(all="ignore"):
        want_loss, want, _ = R.forest_grad(value, type_, size, X[keep], y[keep], True)
        nl, nn, _ = LM.forest_normal_eq(value, type_, size, X[keep], y[keep])
    loss, grad, _ = WG.forest_wgrad(value, type_, size, X0, y, keep.astype(np.float32), "mse")
    fin = np.isfinite(loss)
    assert fin.sum() >= 20
    np.testing.assert_allclose(loss[fin], want_loss[fin], rtol=1e-12)
    np.testing.assert_allclose(grad[fin], want[fin], rtol=1e-9, atol=1e-12)
    loss, normal, _ = WG.forest_wnormal_eq(value, type_, size, X0, y, keep.astype(np.float32))
    np.testing.assert_allclose(loss[fin], nl[fin], rtol=1e-12)
    np.testing.assert_allclose(normal[fin], nn[fin], rtol=1e-9, atol=1e-12)
    for kind, param in WG.KINDS:
        a = WG.forest_wgrad(value, type_, size, X0, y, 3.0 * keep.astype(np.float32), kind, param)
        b = WG.forest_wgrad(value, type_, size, X[keep], y[keep], None, kind, param)
        for u, v in zip(a, b):
            np.testing.assert_allclose(u, v, rtol=1e-12, atol=0, equal_nan=True)
    for bad in (-keep.astype(np.float32), np.zeros(D, np.float32), np.where(keep, np.nan, 1).astype(np.float32)):
        loss, grad, _ = WG.forest_wgrad(value, type_, size, X, y, bad, "mse")
        assert np.isnan(loss).all() and not grad.any()
        loss, normal, _ = WG.forest_wnormal_eq(value, type_, size, X, y, bad)
        assert np.isnan(loss).all() and not normal.any()


@pytest.mark.parametrize("funcs,gp_len,D_", WG.CASES)
def test_reference_leaves_enough_trees_for_the_committed_seeds(funcs, gp_len, D_):
    """the conditioning part of the GPU tests' exclusion rule (the ulp probe needs the oracle library and runs with them): at least
    16 of 24 trees, 21 of 24 under the full function set"""
    value, type_, size, X, y, w = WG.make_case(funcs, gp_len, D_)
    assert (w != 0).any() and (D_ < 60 or (w == 0).sum() >= D_ // 5)
    floor = 21 if funcs == "all" else 16
    for kind, param in WG.KINDS:
        assert WG.comparable_grad(None, value, type_, size, X, y, w, kind, param)[3].sum() >= floor, kind
    assert WG.comparable_normal(None, value, type_, size, X, y, w)[3].sum() >= floor


# ---- 2. host plumbing ----------------------------------------------------------------------------------------------------------------
def test_value_errors(rng):
    value, type_, size, X, y = _case(rng, pop=6)
    f, Xt, yt = _forest(value, type_, size), torch.from_numpy(X), torch.from_numpy(y)
    w = torch.ones(D)
    for kw in (dict(loss="cauchy"), dict(loss="huber"), dict(loss="huber", param=0.0), dict(loss="pinball", param=1.0),
               dict(loss="mse", param=1.0), dict(param=1.0), dict(loss="mae", use_MSE=False), dict(weights=torch.ones(D + 1)),
               dict(weights=torch.ones(1, D)), dict(weights=torch.ones(D, dtype=torch.int64)), dict(weights=[1.0] * D)):
        with pytest.raises(ValueError):
            f.SR_gradient(Xt, yt, **kw)
        with pytest.raises(ValueError):
            f.optimize_constants(Xt, yt, steps=1, **kw)
    for kw in (dict(weights=torch.ones(D + 1)), dict(weights=torch.ones(D, dtype=torch.int32))):
        with pytest.raises(ValueError):
            f.SR_normal_equations(Xt, yt, **kw)
    for kw in (dict(loss="mae"), dict(loss="huber", param=1.0), dict(loss="logcosh", weights=w)):
        with pytest.raises(ValueError):
            f.optimize_constants(Xt, yt, steps=1, method="lm", **kw)
    f.optimize_constants(Xt, yt, steps=1, method="lm", loss="mse", weights=w)
    f.optimize_constants(Xt, yt, steps=1, method="lm", weights=w.to(torch.float64))
    value3, type3, size3, _, y3 = _case(rng, pop=4, out_len=3)
    f3, y3 = _forest(value3, type3, size3, 3), torch.from_numpy(y3)
    for kw in (dict(weights=w), dict(loss="mse"), dict(loss="huber", param=1.0)):
        with pytest.raises(ValueError):
            f3.SR_gradient(Xt, y3, **kw)
        with pytest.raises(ValueError):
            f3.optimize_constants(Xt, y3, steps=1, **kw)
    f3.optimize_constants(Xt, y3, steps=1)   # (the unweighted descent takes multi-output forests, as ever)
    # SymbolicRegression
    m = torch.from_numpy(np.arange(D) % 3 == 0)
    own = [dict(loss="mae"), dict(loss="huber", loss_param=1.0), dict(sample_weights=w), dict(validation_mask=m)]
    for opt in own:
        with pytest.raises(ValueError):   # the default keeps the error of the parent
            SymbolicRegression(datapoints=Xt, labels=yt, const_opt_steps=2, **opt)
        SymbolicRegression(datapoints=Xt, labels=yt, const_opt_steps=2, const_opt_loss="problem", **opt)
        for other in (dict(simplify_every=1), dict(linear_scaling=True)):   # out of scope: they keep theirs
            with pytest.raises(ValueError):
                SymbolicRegression(datapoints=Xt, labels=yt, const_opt_steps=2, const_opt_loss="problem", **opt, **other)
    for opt in (dict(loss="mae"), dict(loss="huber", loss_param=1.0), dict(loss="logcosh", validation_mask=m)):
        with pytest.raises(ValueError):
            SymbolicRegression(datapoints=Xt, labels=yt, const_opt_steps=2, const_opt_method="lm", const_opt_loss="problem", **opt)
    for opt in (dict(loss="mse"), dict(sample_weights=w), dict(validation_mask=m), dict()):
        SymbolicRegression(datapoints=Xt, labels=yt, const_opt_steps=2, const_opt_method="lm", const_opt_loss="problem", **opt)
    for bad in ("mse", "Problem", True, 1):
        with pytest.raises(ValueError):
            SymbolicRegression(datapoints=Xt, labels=yt, const_opt_loss=bad)
    prob = SymbolicRegression(datapoints=Xt, labels=yt, const_opt_steps=1, const_opt_loss="problem", loss="huber", loss_param=1.0)
    with pytest.raises(ValueError):
        prob.optimize(f, use_MSE=False)


def test_keywords_left_at_none_call_none_of_the_new_ops(rng):
    value, type_, size, X, y = _case(rng)
    f, Xt, yt = _forest(value, type_, size), torch.from_numpy(X), torch.from_numpy(y)
    before = dict(cpu_wgrad_ops.calls)
    n_lm = cpu_lm_ops.calls["normal_eq"]
    f.SR_gradient(Xt, yt)
    f.SR_gradient(Xt, yt, False)
    f.SR_normal_equations(Xt, yt)
    a = f.optimize_constants(Xt, yt, steps=2)
    f.optimize_constants(Xt, yt, steps=2, method="lm", dedup=True)
    assert cpu_lm_ops.calls["normal_eq"] == n_lm + 1 + 3
    for kw in (dict(), dict(const_opt_loss="problem"), dict(const_opt_loss="problem", const_opt_method="lm")):
        prob = SymbolicRegression(datapoints=Xt, labels=yt, const_opt_steps=2, **kw)   # none of the four loss options: as ever
        out = prob.optimize(f)
        if "const_opt_method" not in kw:
            assert np.array_equal(_bits(out.batch_node_value), _bits(a[0].batch_node_value))
    assert cpu_wgrad_ops.calls == before


def test_new_keywords_reach_the_new_ops(rng):
    value, type_, size, X, y = _case(rng)
    f, Xt, yt = _forest(value, type_, size), torch.from_numpy(X), torch.from_numpy(y)
    w = torch.from_numpy(rng.uniform(0, 2, D))   # float64: converted on the host
    n = dict(cpu_wgrad_ops.calls)
    loss, grad = f.SR_gradient(Xt, yt, weights=w)
    assert cpu_wgrad_ops.last["kind"] == "mse" and cpu_wgrad_ops.last["weights"].dtype == torch.float32
    want = WG.forest_wgrad(value, type_, size, X, y, w.numpy().astype(np.float32), "mse")
    assert np.array_equal(_bits(loss), want[0].astype(np.float32).view(np.uint32)) and grad.shape == (30, 32)
    f.SR_gradient(Xt, yt, False, weights=w)
    assert cpu_wgrad_ops.last["kind"] == "mae"
    f.SR_gradient(Xt, yt, loss="pinball", param=0.25)
    assert cpu_wgrad_ops.last["kind"] == "pinball" and cpu_wgrad_ops.last["param"] == 0.25 and cpu_wgrad_ops.last["weights"] is None
    assert cpu_wgrad_ops.calls["weighted_gradient"] == n["weighted_gradient"] + 3
    l2, A, b, cidx = f.SR_normal_equations(Xt, yt, weights=w)
    assert cpu_wgrad_ops.calls["weighted_normal_eq"] == n["weighted_normal_eq"] + 1
    assert np.array_equal(_bits(l2), _bits(loss)) and A.shape == (30, 8, 8) and torch.equal(A, A.transpose(1, 2))
    fin = torch.isfinite(loss)
    for t in torch.nonzero(fin)[:, 0].tolist():   # b is half the gradient at the optimised constants
        for j, c in enumerate(cidx[t].tolist()):
            if c >= 0:
                assert abs(float(b[t, j]) - float(grad[t, c]) / 2) <= 1e-5 * max(1.0, abs(float(b[t, j])))
    # 3 steps: 4 dataset passes, each the weighted one
    n = dict(cpu_wgrad_ops.calls)
    f.optimize_constants(Xt, yt, steps=3, weights=w, loss="huber", param=0.5)
    f.optimize_constants(Xt, yt, steps=3, weights=w, method="lm")
    assert cpu_wgrad_ops.calls == {"weighted_gradient": n["weighted_gradient"] + 4, "weighted_normal_eq": n["weighted_normal_eq"] + 4}


@pytest.mark.parametrize("method,kw", [("descent", dict(loss="huber", param=0.5)), ("descent", dict()), ("lm", dict())])
def test_dedup_gives_the_same_bits(rng, method, kw):
    value, type_, size, X, y = _case(rng)
    f = _forest(value, type_, size)
    twice = f + f[:10]
    Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
    w = torch.from_numpy(rng.uniform(0, 2, D).astype(np.float32))
    w[::4] = 0
    h0 = cpu_dedup_ops.calls["tree_classes"]
    a = twice.optimize_constants(Xt, yt, steps=3, method=method, weights=w, **kw)
    b = twice.optimize_constants(Xt, yt, steps=3, method=method, weights=w, dedup=True, **kw)
    assert cpu_dedup_ops.calls["tree_classes"] == h0 + 1
    assert np.array_equal(_bits(a[0].batch_node_value), _bits(b[0].batch_node_value)) and np.array_equal(_bits(a[1]), _bits(b[1]))
    assert np.array_equal(_bits(a[1][30:]), _bits(a[1][:10]))
    # no tree's loss rises, and only constants of the live prefix move
    before = twice.SR_gradient(Xt, yt, weights=w, **kw)[0].numpy()
    after = a[1].numpy()
    fin = np.isfinite(before)
    assert np.all(after[fin] <= before[fin]) and np.array_equal(np.isnan(after), np.isnan(before))
    v0, v1 = twice.batch_node_value.numpy(), a[0].batch_node_value.numpy()
    t0, s0 = twice.batch_node_type.numpy(), twice.batch_subtree_size.numpy()
    is_c = (t0 == R.T_CONST) & (np.arange(32)[None, :] < np.clip(s0[:, :1], 0, 32))
    assert np.array_equal(v0.view(np.uint32)[~is_c], v1.view(np.uint32)[~is_c]) and (v0 != v1).any()


def test_problem_tunes_on_its_training_row(rng):
    value, type_, size, X, y = _case(rng)
    f, Xt, yt = _forest(value, type_, size), torch.from_numpy(X), torch.from_numpy(y)
    w = torch.from_numpy(rng.uniform(0.1, 2, D).astype(np.float32))
    m = torch.from_numpy(np.arange(D) % 4 == 1)
    prob = SymbolicRegression(datapoints=Xt, labels=yt, sample_weights=w, validation_mask=m, loss="pinball", loss_param=0.3,
                              const_opt_steps=2, const_opt_loss="problem", const_step_size=0.2)
    out = prob.optimize(f)
    assert torch.equal(cpu_wgrad_ops.last["weights"], w * (~m)) and cpu_wgrad_ops.last["kind"] == "pinball"
    want = f.optimize_constants(Xt, yt, 2, 0.2, weights=w * (~m), loss="pinball", param=0.3)[0]
    assert np.array_equal(_bits(out.batch_node_value), _bits(want.batch_node_value))
    # weights or a mask alone: the weighted MSE, or the weighted MAE under use_MSE=False
    prob = SymbolicRegression(datapoints=Xt, labels=yt, validation_mask=m, const_opt_steps=1, const_opt_loss="problem")
    prob.optimize(f)
    assert cpu_wgrad_ops.last["kind"] == "mse" and torch.equal(cpu_wgrad_ops.last["weights"], (~m).to(torch.float32))
    prob.optimize(f, use_MSE=False)
    assert cpu_wgrad_ops.last["kind"] == "mae"
    # a loss alone: no weight row at all
    prob = SymbolicRegression(datapoints=Xt, labels=yt, loss="logcosh", const_opt_steps=1, const_opt_loss="problem")
    prob.optimize(f)
    assert cpu_wgrad_ops.last["kind"] == "logcosh" and cpu_wgrad_ops.last["weights"] is None


# ---- 3. the planted problems, through StandardPipeline.step ------------------------------------------------------------------------
def test_reference_step_count():
    X, y, m = C.held_out_data()
    v, t, s = C.planted_arrays(1)
    w = (~m).astype(np.float32)
    met = [C.distance(WG.lm_optimize(v, t, s, X, y, w, k)[0][0, [2, 4]]) <= C.BOUND for k in range(C.HELD_OUT_REFERENCE_STEPS + 1)]
    assert met == [False] * C.HELD_OUT_REFERENCE_STEPS + [True]


def test_held_out_rows_are_not_leaked():
    X, y, m = C.held_out_data()
    c = C.tuned_constants("cpu", X, y, validation_mask=torch.from_numpy(m), const_opt_steps=C.HELD_OUT_STEPS, const_opt_method="lm",
                          const_opt_loss="problem")
    assert C.distance(c) <= C.BOUND, c
    # the same forest tuned by the unweighted call reads the held-out rows, whose labels are 100 off
    f = Forest(1, 1, *(torch.from_numpy(a) for a in C.planted_arrays()))
    leak = f.optimize_constants(torch.from_numpy(X), torch.from_numpy(y), steps=C.HELD_OUT_STEPS, method="lm")[0]
    assert C.distance(leak.batch_node_value.numpy()[0, [2, 4]]) > C.BOUND


def test_robust_tuning_resists_outliers():
    X, y = C.robust_data()
    huber = C.tuned_constants("cpu", X, y, loss="huber", loss_param=1.0, const_opt_steps=C.ROBUST_STEPS, const_opt_loss="problem")
    mse = C.tuned_constants("cpu", X, y, loss="mse", const_opt_steps=C.ROBUST_STEPS, const_opt_loss="problem")
    assert C.distance(huber) < C.distance(mse), (huber, mse)


# ---- 4. the C entry points' argument checks ------------------------------------------------------------------------------------------
def test_argument_errors_without_gpu():
    from evogp_amd import _lib

    L = _lib.lib
    p, q = 8, 16  # (never dereferenced: the host checks come first)

    def grad(pop=4, D=8, gp_len=32, var_len=3, out_len=1, value=p, X=p, y=p, weights=p, kind=0, param=0.0, loss=q, out=q):
        return L.evogp_hip_sr_weighted_gradient(pop, D, gp_len, var_len, out_len, value, p, p, X, y, weights, kind, param, loss, out, None)

    def neq(pop=4, D=8, gp_len=32, var_len=3, out_len=1, value=p, X=p, y=p, weights=p, loss=q, out=q):
        return L.evogp_hip_sr_weighted_normal_eq(pop, D, gp_len, var_len, out_len, value, p, p, X, y, weights, loss, out, None)

    for call in (grad, neq):
        for kw in (dict(pop=0), dict(D=0), dict(gp_len=0), dict(gp_len=1025), dict(var_len=0), dict(out_len=0)):
            assert call(**kw) == -1, kw
        assert call(out_len=2) == -3                                   # multi-output: unsupported
        assert call(out_len=2, gp_len=1025) == -1                      # (the argument checks come first)
        for kw in (dict(value=None), dict(X=None), dict(y=None), dict(loss=None), dict(out=None), dict(weights=None, out=None)):
            assert call(**kw) == -2, kw
    for kw in (dict(kind=-1), dict(kind=5), dict(kind=2, param=0.0), dict(kind=2, param=-1.0), dict(kind=2, param=float("inf")),
               dict(kind=2, param=float("nan")), dict(kind=3, param=0.0), dict(kind=3, param=1.0), dict(kind=3, param=float("nan")),
               dict(kind=0, param=float("nan")), dict(kind=4, param=float("nan"))):
        assert grad(**kw) == -1, kw
    assert grad(out_len=2, kind=5) == -1
    assert L.evogp_hip_abi_version() == _lib.ABI_VERSION
