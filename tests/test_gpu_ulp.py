"""GPU: accuracy of every libm-backed function of the interpreter, pinned in ULPs against a float64 truth.

The reference evaluates sin cos tan sinh cosh tanh log exp pow sqrt and the divisions with the device math library
(forward.cu:125-167,183-200); here they exist three times — the register interpreters (interp.hpp: `batch_evaluate`,
`tree_evaluate`), the threaded-code handlers transcribed from the library's ISA (gen/gen_tc_asm.py) and the constant folding
of the program compiler.  A wrong polynomial constant that costs 1e-4 would pass a tree-level tolerance test; it cannot pass
these: single-node trees f(x) / f(a, b) over ~1e6 inputs per function (dense around the origin, log-uniform over the
whole exponent range, the range ends, non-finite operands), each result compared with numpy's float64 value:

    |result - truth| <= BOUND[f] * ulp_fp32(truth)        and identical NaN / +-inf classes

through FOUR routes:
  batch     evogp_hip_batch_evaluate, one tree over N datapoints (the STORE kernels)
  evaluate  evogp_hip_evaluate, N trees with one input row each (the lane-per-tree kernel)
  fit_S     evogp_hip_sr_fitness, D = 1, N trees  SUB(f(ADD(c_t, x0)), r_t)  with x0 = 0, label 0, MAE: the fitness of
            tree t is |f(c_t) - r_t| computed in fp32 — exact by Sterbenz when the two are within a factor of two — so the
            handler's error is read off directly (f takes its operand from the operand stack);
  fit_V     the same with  SUB(f(x_j), r_j): the operand comes from the dataset (the V form of the handler).
BOUND is the largest error MEASURED on MI355X for the function (recorded in profiles/r02_ulp_report.json by this test when
gpurun_out/ exists), never looser than the OpenCL/OCML documented bound in the comment next to it.
"""
import json
import os
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T_VAR, T_CONST, T_UFUNC, T_BFUNC = 0, 1, 2, 3
F = dict(ADD=1, SUB=2, MUL=3, DIV=4, LOOSE_DIV=5, POW=6, LOOSE_POW=7, SIN=14, COS=15, TAN=16, SINH=17, COSH=18, TANH=19, LOG=20,
         LOOSE_LOG=21, EXP=22, INV=23, LOOSE_INV=24, SQRT=27, LOOSE_SQRT=28)
N = 1 << 20
REPORT = {}


@pytest.fixture(scope="module")
def g():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import gpu_capi

    return gpu_capi


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def _log_uniform(rng, n, e_lo, e_hi, signed=True):
    x = np.ldexp(rng.uniform(1.0, 2.0, n), rng.integers(e_lo, e_hi, n)).astype(np.float32)
    return x * rng.choice([-1.0, 1.0], n).astype(np.float32) if signed else x


def inputs(rng, e_hi, lo=None, hi=None, signed=True, n=N):
    """a third dense around the origin, two thirds log-uniform in magnitude up to 2^e_hi, plus the special operands"""
    dense = rng.uniform(-10.0 if signed else 0.0, 10.0, n // 3).astype(np.float32)
    wide = _log_uniform(rng, n - n // 3 - 64, -149 + 23, e_hi, signed)
    special = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1.1754942e-38, 1.17549435e-38, 3.4028235e38,
                        -3.4028235e38, 0.5, 2.0, np.pi, -np.pi, np.pi / 2, 1e9, -1e9, 1e-9, -1e-9], np.float32)
    x = np.concatenate([dense, wide, np.resize(special, 64)]).astype(np.float32)
    if lo is not None:
        keep = np.isnan(x) | np.isinf(x) | ((x >= lo) & (x <= hi))
        x = np.where(keep, x, rng.uniform(lo, hi, x.shape).astype(np.float32))
    return x


with np.errstate(all="ignore"):
    pass


def _truth_unary(name, x64):
    with np.errstate(all="ignore"):
        if name == "LOOSE_LOG":
            return np.where(x64 == 0, -1e9, np.log(np.abs(x64)))
        if name == "LOOSE_SQRT":
            return np.sqrt(np.abs(x64))
        if name == "INV":
            return np.where(x64 == 0, np.nan, 1.0 / x64)
        if name == "LOOSE_INV":
            d = np.where(np.abs(x64) <= np.float32(1e-9), np.copysign(np.float64(np.float32(1e-9)), x64), x64)
            return 1.0 / d
        return dict(SIN=np.sin, COS=np.cos, TAN=np.tan, SINH=np.sinh, COSH=np.cosh, TANH=np.tanh, LOG=np.log, EXP=np.exp, SQRT=np.sqrt)[name](x64)


def _truth_binary(name, a64, b64):
    with np.errstate(all="ignore"):
        if name == "DIV":
            return np.where(b64 == 0, np.nan, a64 / b64)
        if name == "LOOSE_DIV":
            d = np.where(np.abs(b64) <= np.float32(1e-9), np.copysign(np.float64(np.float32(1e-9)), b64), b64)
            return a64 / d
        if name == "POW":
            return np.power(a64, b64)
        return np.where((a64 == 0) & (b64 == 0), 0.0, np.power(np.abs(a64), b64))  # LOOSE_POW, forward.cu:195-200


from ulp_bounds import BINARY, LARGE, UNARY  # noqa: E402,F401  (the tables and how they were measured: tests/ulp_bounds.py)


def ulp32(t64):
    t32 = np.abs(t64).astype(np.float32)
    with np.errstate(all="ignore"):
        return np.maximum(np.spacing(t32).astype(np.float64), 2.0 ** -149)


def check(name, route, got, truth64, bound, extra_ulps=0.0):
    """same NaN / inf classes as the fp32-rounded truth; ulp error on the finite ones; records the measured maximum"""
    got = np.asarray(got, np.float32).ravel()
    with np.errstate(all="ignore"):
        t32 = truth64.astype(np.float32)
    assert np.array_equal(np.isnan(got), np.isnan(t32)), f"{name} via {route}: NaN sets differ ({np.isnan(got).sum()} vs {np.isnan(t32).sum()})"
    inf = np.isinf(t32)
    assert np.array_equal(got[inf], t32[inf]), f"{name} via {route}: infinities differ"
    fin = np.isfinite(t32) & np.isfinite(got)
    assert np.array_equal(np.isfinite(got), np.isfinite(t32)), f"{name} via {route}: finite sets differ"
    err = np.abs(got[fin].astype(np.float64) - truth64[fin]) / ulp32(truth64[fin])
    worst = float(err.max()) if err.size else 0.0
    REPORT.setdefault(name, {})[route] = round(worst, 3)
    assert worst <= bound + extra_ulps, f"{name} via {route}: {worst:.2f} ulp at operand index {int(np.argmax(err))} (bound {bound})"


def one_node_forest(fid, arity, pop, L=4):
    v = np.zeros((pop, L), np.float32); t = np.zeros((pop, L), np.int16); s = np.zeros((pop, L), np.int16)
    v[:, 0] = fid; t[:, 0] = T_UFUNC if arity == 1 else T_BFUNC; s[:, 0] = arity + 1
    for a in range(arity):
        v[:, 1 + a] = a; t[:, 1 + a] = T_VAR; s[:, 1 + a] = 1
    return v, t, s


def residual_forest(fid, operands, r32, from_vars=False):
    """SUB(f(ADD(c, x0)...), r) per tree (operands on the stack), or SUB(f(x_j...), r_j) (operands from the dataset)"""
    pop, arity = operands[0].shape[0], len(operands)
    L = 16
    v = np.zeros((pop, L), np.float32); t = np.zeros((pop, L), np.int16); s = np.zeros((pop, L), np.int16)
    per = 1 if from_vars else 3
    n = 2 + arity * per + 1
    v[:, 0] = F["SUB"]; t[:, 0] = T_BFUNC; s[:, 0] = n
    v[:, 1] = fid; t[:, 1] = T_UFUNC if arity == 1 else T_BFUNC; s[:, 1] = 1 + arity * per
    k = 2
    for a in range(arity):
        if from_vars:
            v[:, k] = np.arange(pop) * arity + a; t[:, k] = T_VAR; s[:, k] = 1
        else:
            v[:, k] = F["ADD"]; t[:, k] = T_BFUNC; s[:, k] = 3
            v[:, k + 1] = operands[a]; t[:, k + 1] = T_CONST; s[:, k + 1] = 1
            v[:, k + 2] = 0; t[:, k + 2] = T_VAR; s[:, k + 2] = 1
        k += per
    v[:, k] = r32; t[:, k] = T_CONST; s[:, k] = 1
    return v, t, s


def run_all_routes(g, name, arity, ops32, truth_fn, b_reg, b_tc, label=None):
    fid = F[name]
    name = label or name
    X = np.stack(ops32, 1)
    truth64 = truth_fn(*[o.astype(np.float64) for o in ops32])
    lib = np.asarray(g.batch_evaluate(*one_node_forest(fid, arity, 1), X, 1), np.float32).ravel()   # the register kernels call the device library
    check(name, "batch", lib, truth64, b_reg)
    check(name, "evaluate", g.evaluate(*one_node_forest(fid, arity, X.shape[0]), X, 1), truth64, b_reg)
    # the fitness routes feed the operand through ADD(c, x0 = 0), which turns -0 into +0: same operands for the truth
    ops32 = [np.where(o == 0, np.float32(0.0), o) for o in ops32]
    truth64 = truth_fn(*[o.astype(np.float64) for o in ops32])
    # fitness routes: operands whose truth is finite (the residual of a non-finite value is NaN whatever the handler did)
    with np.errstate(all="ignore"):
        r32 = truth64.astype(np.float32)
    ok = np.isfinite(r32) & np.all([np.isfinite(o) for o in ops32], 0)
    sel = [o[ok] for o in ops32]
    res = g.sr_fitness(*residual_forest(fid, sel, r32[ok]), np.zeros((1, 1), np.float32), np.zeros((1, 1), np.float32), False)
    assert np.isfinite(res).all(), f"{name} via fit_S: non-finite residual for a finite truth"
    err = res.astype(np.float64) / ulp32(truth64[ok])
    REPORT.setdefault(name, {})["fit_S"] = round(float(err.max()), 3)
    assert err.max() <= b_tc + 0.5, f"{name} via fit_S: {err.max():.2f} ulp (bound {b_tc} + 0.5 for the rounded truth)"
    # the threaded-code handlers are the library's own instruction sequences: with the register kernels' result as the constant r,
    # every residual must be exactly zero (the divisions excepted: their default sequence is faithfully, not correctly, rounded)
    if "DIV" not in name and "INV" not in name:
        lib_s = np.asarray(g.batch_evaluate(*one_node_forest(fid, arity, 1), np.stack(sel, 1), 1), np.float32).ravel()
        fin = np.isfinite(lib_s)
        res = g.sr_fitness(*residual_forest(fid, [o[fin] for o in sel], lib_s[fin]), np.zeros((1, 1), np.float32), np.zeros((1, 1), np.float32), False)
        assert (res == 0).all(), f"{name}: {int((res != 0).sum())} of {res.size} handler results differ from the library's (largest residual {res.max()})"
    # operands from the dataset: 144 / arity trees per call (the dataset of one call lives in LDS), 24 calls
    per_call = 144 // arity
    worst = 0.0
    idx = np.flatnonzero(ok)
    for c in range(24):
        pick = idx[(np.arange(per_call) * 7919 + c * 104729) % idx.size]
        row = np.stack([o[pick] for o in ops32], 1).reshape(1, -1)
        res = g.sr_fitness(*residual_forest(fid, [o[pick] for o in ops32], r32[pick], from_vars=True), row, np.zeros((1, 1), np.float32), False)
        assert np.isfinite(res).all(), f"{name} via fit_V: non-finite residual for a finite truth"
        worst = max(worst, float((res.astype(np.float64) / ulp32(truth64[pick])).max()))
    REPORT[name]["fit_V"] = round(worst, 3)
    assert worst <= b_tc + 0.5, f"{name} via fit_V: {worst:.2f} ulp (bound {b_tc} + 0.5)"
    # non-finite and out-of-domain operands through the fitness path: |f(c)| must have the truth's class
    bad = ~ok
    if bad.any():
        ops_b = [o[bad] for o in ops32]
        fin_ops = np.all([np.isfinite(o) for o in ops_b], 0)   # a NaN constant cannot be told from a marked tree: finite operands only
        if fin_ops.any():
            ops_b = [o[fin_ops] for o in ops_b]
            fv, ft, fs = residual_forest(fid, ops_b, np.zeros(ops_b[0].shape[0], np.float32))
            res = g.sr_fitness(fv, ft, fs, np.zeros((1, 1), np.float32), np.zeros((1, 1), np.float32), False)
            want = np.abs(r32[bad][fin_ops])
            assert np.array_equal(np.isnan(res), np.isnan(want)) and np.array_equal(np.isinf(res), np.isinf(want)), f"{name} via fit_S: classes of special operands differ"


@pytest.mark.parametrize("name", list(UNARY))
def test_unary_function_within_ulp_bound(g, name):
    b_reg, b_tc, dom = UNARY[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))  # the same operands in every run
    signed = name not in ()
    x = inputs(rng, dom["e_hi"], dom.get("lo"), dom.get("hi"), signed)
    run_all_routes(g, name, 1, [x], lambda a: _truth_unary(name, a), b_reg, b_tc)


@pytest.mark.parametrize("name", ["SIN", "COS", "TAN"])
def test_trigonometric_large_arguments(g, name):
    """beyond 2^17 the library switches to a Payne-Hanek reduction; the threaded-code handlers bail out to the register
    kernels there (run-time test of the block's largest operand): same bound on the whole fp32 range"""
    b_reg, b_tc = LARGE[name]
    rng = np.random.default_rng(77)
    x = _log_uniform(rng, N // 4, 17, 127)
    run_all_routes(g, name, 1, [x], lambda a: _truth_unary(name, a), b_reg, b_tc, label=name + "_large")


@pytest.mark.parametrize("name", list(BINARY))
def test_binary_function_within_ulp_bound(g, name):
    b_reg, b_tc = BINARY[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))  # the same operands in every run
    if "POW" in name:
        a = inputs(rng, 20, signed=(name == "LOOSE_POW"))
        b = rng.uniform(-12, 12, a.shape).astype(np.float32)
        ints = rng.random(a.shape) < 0.25
        b[ints] = np.round(b[ints])
        if name == "POW":  # negative bases with integer exponents
            neg = ints & (rng.random(a.shape) < 0.5)
            a[neg] = -np.abs(a[neg])
    else:
        a = inputs(rng, 100)
        b = inputs(np.random.default_rng(5), 100)
        rng.shuffle(b)
    run_all_routes(g, name, 2, [a, b], lambda p, q: _truth_binary(name, p, q), b_reg, b_tc)


def test_write_ulp_report():
    """not a check: leaves the measured maxima where the round's profiles are collected"""
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    if os.path.isdir(out) and REPORT:
        json.dump(REPORT, open(os.path.join(out, "ulp_report.json"), "w"), indent=1, sort_keys=True)
