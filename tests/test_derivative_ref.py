"""CPU: the numpy restatement of the derivative bounds (tests/derivative_ref.py) against hand cases, against the interval restatement it
builds on, and against exact evaluation (tests/derivative_exact.py: fractions.Fraction, mpmath at 256 bits) of the value and the
forward-mode derivative of every subtree of random trees, with no tolerance."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import derivative_exact as DX  # noqa: E402
import derivative_ref as DR  # noqa: E402
import interval_cases as IC  # noqa: E402
import interval_ref as IR  # noqa: E402
import sr_grad_ref as R  # noqa: E402
from interval_cases import B, C, IF, U, V  # noqa: E402

F = np.float32
INF = F(np.inf)
JUMP, MAL, DEP = DR.JUMP, IR.MALFORMED, DR.DEPENDS
# arith; arith + comparisons + IF + abs / max / min; all 29
SHAPES = IC.LOGIC + [R.F_ABS, R.F_MAX, R.F_MIN]
SETS = {"arith": IC.ARITH, "shapes": SHAPES, "all": IC.ALL}


def _root(expr, lower, upper, wrt, L=16, **kw):
    """[(dlo, dhi, dflags) of the root for every requested variable], (vlo, vhi, vflags) of the root"""
    v, t, s = IC.rows([expr], L)
    o = DR.forest_derivative_intervals(v, t, s, lower, upper, wrt, **kw)
    return [(o[3][k, 0, 0], o[4][k, 0, 0], int(o[5][k, 0, 0])) for k in range(len(wrt))], (o[0][0, 0], o[1][0, 0], int(o[2][0, 0]))


def _d(expr, lower, upper, v=0, **kw):
    return _root(expr, lower, upper, [v], **kw)[0][0]


def _ulps(a, b):
    return abs(int(IC.ulp_key(a)) - int(IC.ulp_key(b)))


def _about(got, lo, hi, ulps=4):
    """got = (dlo, dhi, flags) contains [lo, hi] and is within ``ulps`` of it"""
    return got[0] <= F(lo) and got[1] >= F(hi) and _ulps(got[0], F(lo)) <= ulps and _ulps(got[1], F(hi)) <= ulps


def test_leaves_and_independence():
    assert _d(C(3.0), [-1], [1]) == (F(0), F(0), 0)
    assert _root(V(1), [-1, -1], [1, 1], [0, 1])[0] == [(F(0), F(0), 0), (F(1), F(1), DEP)]
    # a subtree without x_v is exactly [0, 0] with flags 0, even under a division by an interval that holds 0
    e = B(R.F_DIV, V(1), B(R.F_SUB, V(1), V(1)))
    (d0, d1), r = _root(e, [-1, -1], [1, 1], [0, 1])
    assert d0 == (F(0), F(0), 0) and d1 == (-INF, INF, DEP) and r[2] == IR.MAY_NAN
    assert _d(U(R.F_LOG, B(R.F_POW, V(1), V(1))), [-1, -1], [1, 1]) == (F(0), F(0), 0)
    assert _d(U(5, V(0)), [1], [2]) == (F(0), F(0), 0) and _d(B(20, V(0), V(0)), [1], [2]) == (F(0), F(0), 0)     # unknown ids


def test_arithmetic_rules():
    assert _about(_d(B(R.F_MUL, V(0), V(0)), [-1], [2]), -2, 4) and _d(B(R.F_MUL, V(0), V(0)), [-1], [2])[2] == DEP
    assert _d(B(R.F_ADD, V(0), V(1)), [-1, -1], [1, 1]) == (F(1), F(1), DEP)        # D(b) = [0, 0]: a point-zero operand, exact
    assert _about(_d(B(R.F_ADD, V(0), V(0)), [-1], [1]), 2, 2, 1)
    assert _about(_d(B(R.F_SUB, V(1), V(0)), [-1, -1], [1, 1]), -1, -1, 0)
    assert _d(U(R.F_NEG, V(0)), [0], [1]) == (F(-1), F(-1), DEP)
    assert _d(B(R.F_MUL, V(0), C(3.0)), [-1], [1]) == (F(3), F(3), DEP)              # 1 * [3, 3] + R(a) * [0, 0]: both exact
    # x0 / x1 over x1 in [1, 2]: d/dx0 = 1 / x1 in [0.5, 1], d/dx1 = -x0 / x1^2 in [-2, 2] for x0 in [-2, 2]
    (d0, d1), _ = _root(B(R.F_DIV, V(0), V(1)), [-2, 1], [2, 2], [0, 1])
    assert _about(d0, 0.5, 1) and d0[2] == DEP and d1[0] <= F(-2) and d1[1] >= F(2) and d1[1] <= F(4.001)
    assert _d(B(R.F_DIV, V(0), V(1)), [-2, -1], [2, 2]) == (-INF, INF, DEP)          # the divisor holds 0: the fallback, no JUMP
    assert _about(_d(U(R.F_INV, V(0)), [1], [2]), -1, -0.25, 6)
    assert _d(U(R.F_INV, V(0)), [0], [2]) == (-INF, INF, DEP)
    # the loose forms: the strict rule away from [-kDelta, kDelta], the fallback with JUMP where the divisor can meet it
    assert _about(_d(U(R.F_LOOSE_INV, V(0)), [1], [2]), -1, -0.25, 6)
    assert _d(U(R.F_LOOSE_INV, V(0)), [-1], [2]) == (-INF, INF, DEP | JUMP)
    assert _about(_d(B(R.F_LOOSE_DIV, V(0), V(1)), [-2, 1], [2, 2]), 0.5, 1)
    assert _d(B(R.F_LOOSE_DIV, V(0), V(1)), [-2, 0], [2, 2]) == (-INF, INF, DEP | JUMP)


def test_abs_max_min():
    assert _d(U(R.F_ABS, V(0)), [-1], [2]) == (F(-1), F(1), DEP)
    assert _d(U(R.F_ABS, V(0)), [0], [2]) == (F(1), F(1), DEP) and _d(U(R.F_ABS, V(0)), [-3], [0]) == (F(-1), F(-1), DEP)
    two = B(R.F_MUL, V(0), C(2.0))
    assert _d(B(R.F_MAX, two, V(1)), [1, -1], [2, 1]) == (F(2), F(2), DEP)           # separated: the winner's
    assert _d(B(R.F_MIN, two, V(1)), [1, -1], [2, 1]) == (F(0), F(0), 0)
    assert _d(B(R.F_MAX, two, V(1)), [0, -1], [2, 1]) == (F(0), F(2), DEP)           # overlapping: the hull
    assert _d(B(R.F_MAX, C(np.nan), two), [0], [1]) == (F(2), F(2), DEP)             # a NaN constant first: the second operand
    # the first operand may be a NaN and moves with x0: the value can switch to the second operand, JUMP
    d = _d(B(R.F_MAX, U(R.F_SQRT, V(0)), V(1)), [-1, 0], [4, 1])
    assert d[2] == DEP | JUMP and d[0] == -INF


def test_comparisons_and_if():
    assert _d(B(R.F_LT, V(0), C(0.5)), [-1], [1]) == (F(0), F(0), DEP | JUMP)        # undecided over the box
    assert _d(B(R.F_LT, V(0), C(2.0)), [-1], [1]) == (F(0), F(0), DEP)               # decided: a constant
    assert _d(B(R.F_GE, V(1), C(0.0)), [-1, -1], [1, 1]) == (F(0), F(0), 0)
    (d0, d1, d2), _ = _root(IF(V(0), V(1), V(2)), [-1] * 3, [1] * 3, [0, 1, 2])
    assert d0 == (F(0), F(0), DEP | JUMP) and d1 == (F(0), F(1), DEP) and d2 == (F(0), F(1), DEP)
    (d0, d1, d2), _ = _root(IF(V(0), V(1), V(2)), [0.5, -1, -1], [1, 1, 1], [0, 1, 2])
    assert d0 == (F(0), F(0), 0) and d1 == (F(1), F(1), DEP) and d2 == (F(0), F(0), 0)      # decided: the branch, the condition drops out
    assert _d(IF(C(np.nan), V(0), U(R.F_NEG, V(0))), [0], [1]) == (F(-1), F(-1), DEP)


def test_roots_logs_and_library_rules():
    assert _about(_d(U(R.F_SQRT, V(0)), [1], [4]), 0.25, 0.5, 6)
    assert _d(U(R.F_SQRT, V(0)), [0], [4]) == (-INF, INF, DEP)
    assert _about(_d(U(R.F_LOOSE_SQRT, V(0)), [-4], [-1]), -0.5, -0.25, 6)
    assert _d(U(R.F_LOOSE_SQRT, V(0)), [-4], [1]) == (-INF, INF, DEP)                # continuous, the slope unbounded: no JUMP
    d = _d(U(R.F_EXP, V(0)), [0], [1])
    assert d[0] <= F(1) and d[1] >= F(np.e) and _ulps(d[1], F(np.e)) <= 2 * IR.W_ULPS[R.F_EXP] + 2 and d[2] == DEP
    assert _about(_d(U(R.F_LOG, V(0)), [1], [4]), 0.25, 1, 2)
    assert _d(U(R.F_LOG, V(0)), [0], [4]) == (-INF, INF, DEP)
    assert _about(_d(U(R.F_LOOSE_LOG, V(0)), [-4], [-1]), -1, -0.25, 2)
    assert _d(U(R.F_LOOSE_LOG, V(0)), [-4], [1]) == (-INF, INF, DEP | JUMP)
    w = 2 * IR.W_ULPS[R.F_SIN] + 4
    d = _d(U(R.F_SIN, V(0)), [0.5], [1])                                             # cos over [0.5, 1]
    assert d[0] <= F(np.cos(1.0)) and d[1] >= F(np.cos(0.5)) and _ulps(d[0], F(np.cos(1.0))) <= w and _ulps(d[1], F(np.cos(0.5))) <= w
    d = _d(U(R.F_COS, V(0)), [0.5], [1])                                             # -sin over [0.5, 1]
    assert d[0] <= F(-np.sin(1.0)) and d[1] >= F(-np.sin(0.5)) and _ulps(d[0], F(-np.sin(1.0))) <= w and d[2] == DEP
    d = _d(U(R.F_TAN, V(0)), [0], [1])
    assert d[0] <= F(1) and d[1] >= F(1 + np.tan(1.0) ** 2) and d[1] <= F(4.5) and d[2] == DEP
    assert _d(U(R.F_TAN, V(0)), [1], [2])[2] == DEP | JUMP                           # a pole inside
    d = _d(U(R.F_SINH, V(0)), [-1], [1])
    assert d[0] <= F(1) and d[1] >= F(np.cosh(1.0)) and d[1] <= F(1.55)
    d = _d(U(R.F_COSH, V(0)), [-1], [1])
    assert d[0] <= F(-np.sinh(1.0)) and d[1] >= F(np.sinh(1.0)) and d[1] <= F(1.18)
    d = _d(U(R.F_TANH, V(0)), [-1], [1])
    assert F(0.41) <= d[0] <= F(1 - np.tanh(1.0) ** 2) and d[1] == F(1)              # 1 - Q Q = [0.42, 1.58] cut to [0, 1]
    d = _d(U(R.F_TANH, V(0)), [1], [2])
    assert F(0) <= d[0] <= F(1 - np.tanh(2.0) ** 2) and F(1 - np.tanh(1.0) ** 2) <= d[1] <= F(0.43)
    for f in (R.F_POW, R.F_LOOSE_POW):
        assert _d(B(f, V(0), C(2.0)), [1], [2]) == (-INF, INF, DEP)                  # the closed forms are not built
        assert _d(B(f, V(0), C(-1.0)), [-1], [2]) == (-INF, INF, DEP | JUMP)         # a pole the fp32 flags do not show
        assert _d(B(f, V(1), C(2.0)), [1, 1], [2, 2]) == (F(0), F(0), 0)


def test_malformed_rows_and_dead_words():
    v, t, s = IC.rows([B(R.F_ADD, V(0), V(0))] * 3 + [V(0)], 8)
    t[0, 2] = 3
    s[1, 0] = 2
    s[2, 1] = 2
    s[3, 0] = 0
    o = DR.forest_derivative_intervals(v, t, s, [1], [2], [0, 0])
    for k in range(2):
        for r, n in ((0, 3), (1, 2), (2, 3), (3, 1)):
            assert np.isnan(o[3][k, r, :n]).all() and np.isnan(o[4][k, r, :n]).all() and (o[5][k, r, :n] == MAL).all()
            assert not o[3][k, r, n:].any() and not o[4][k, r, n:].any() and not o[5][k, r, n:].any()
    assert np.array_equal(o[3][0].view(np.uint32), o[3][1].view(np.uint32))          # a repeated index: equal slices
    assert not DR.monotone(*o, [(0.0, np.inf)] * 2).any()


@pytest.mark.parametrize("box", range(3))
@pytest.mark.parametrize("funcs", ["arith", "logic", "all"])
def test_enclosures_contain_the_fp32_intervals(funcs, box, oracle, rng):
    """R contains interval_ref's interval with equal flags on every node of the forests test_interval_ref.py's fuzz draws"""
    ids = {"arith": IC.ARITH, "logic": IC.LOGIC, "all": IC.ALL}[funcs]
    v, t, s = IC.oracle_forest(oracle, rng, 200, ids, key=box)
    lo, hi, fl = IR.forest_intervals(v, t, s, *IC.BOXES[box])
    vlo, vhi, vfl = DR.forest_enclosures(v, t, s, *IC.BOXES[box])
    live = np.arange(v.shape[1])[None, :] < s[:, :1]
    assert not (fl & MAL).any() and live.sum() > 1000
    bad = np.argwhere(live & ~((vlo <= lo) & (vhi >= hi) & (vfl == fl)))
    assert len(bad) == 0, [(a, b, lo[a, b], hi[a, b], fl[a, b], vlo[a, b], vhi[a, b], vfl[a, b]) for a, b in bad[:4]]
    assert not vlo[~live].any() and not vhi[~live].any() and not vfl[~live].any()


@pytest.fixture(scope="module")
def soundness_forests(oracle):
    """200 oracle-generated trees per function set (no planted NaN / inf constants: such a tree has no real value anywhere).  The
    generator draws the constant 0 and expressions like x - x, so about one arith tree in ten divides by zero at every point and about
    one shapes tree in eight sits on a tie everywhere; the keys are the ones of 160 tried (40 .. 199) for which the exact evaluator ALONE
    -- no bound computed -- skips the fewest (tree, point) pairs on [-1, 1]^3: the 5 % cap below is a condition on the test's data"""
    rng = np.random.default_rng(20261019)
    keys = {"arith": 141, "shapes": 114, "all": 42}
    return {name: IC.oracle_forest(oracle, rng, 200, ids, key=keys[name], plant=0.0) for name, ids in SETS.items()}


def _check_claim_a(forest, box, mode, n_points=64):
    """claim (a), and R's claim, on every subtree at ``n_points`` dyadic points -> (failures, share of (tree, point) pairs skipped at the
    root, number of (node, point, variable) checks)"""
    v, t, s = forest
    lower, upper = IC.BOXES[box]
    vlo, vhi, vfl, dlo, dhi, dfl = DR.forest_derivative_intervals(v, t, s, lower, upper, [0, 1, 2])
    assert not (vfl & MAL).any()
    pts = DX.dyadic_points(np.random.default_rng([20261019, box]), lower, upper, n_points)
    ex = DX.Exact(mode, 3)
    if mode == "mpmath":
        pts = [[ex.num(c) for c in p] for p in pts]
    bad, skipped, checks = [], 0, 0
    frac = mode == "fraction"
    for r in range(v.shape[0]):
        n = int(s[r, 0])
        vb = DX.exact_bounds(vlo[r, :n], vhi[r, :n], frac)
        db = [DX.exact_bounds(dlo[k, r, :n], dhi[k, r, :n], frac) for k in range(3)]
        for p in pts:
            nodes = ex.evaluate(v[r], t[r], s[r], p)
            skipped += (not nodes[0].alldef) or any(nodes[0].kink)
            for i, nd in enumerate(nodes):
                if not nd.alldef:
                    continue
                if not DX.within(nd.val, vb[i]):
                    bad.append((r, i, "value", float(nd.val), vlo[r, i], vhi[r, i]))
                for k in range(3):
                    if nd.kink[k]:
                        continue
                    checks += 1
                    if not DX.within(nd.der[k], db[k][i]):
                        bad.append((r, i, k, float(nd.der[k]), dlo[k, r, i], dhi[k, r, i]))
                    if nd.dep[k] is False and (dlo[k, r, i], dhi[k, r, i], dfl[k, r, i]) != (0, 0, 0):
                        bad.append((r, i, k, "independent", dlo[k, r, i], dhi[k, r, i], dfl[k, r, i]))
    return bad, skipped / (v.shape[0] * len(pts)), checks


@pytest.mark.parametrize("box", range(3))
@pytest.mark.parametrize("funcs", ["arith", "shapes"])
def test_soundness_exact_fractions(funcs, box, soundness_forests):
    """claim (a) with no tolerance: value and forward-mode derivative in exact rational arithmetic at 64 dyadic points of the box, on
    every subtree, wherever all its nodes are defined and no kink is hit.  The skipped (tree, point) pairs -- kinks plus undefined --
    stay below 5 % on [-1, 1]^3 (measured with the evaluator alone before the keys were fixed: arith 2.00 %, shapes 3.07 %)"""
    bad, skipped, checks = _check_claim_a(soundness_forests[funcs], box, "fraction")
    print(f"{funcs} box {box}: {checks} checks, {100 * skipped:.2f} % of the (tree, point) pairs skipped")
    assert not bad, bad[:5]
    assert checks > 100000
    if box == 0:
        assert skipped <= 0.05


@pytest.mark.parametrize("box", range(3))
def test_soundness_mpmath(box, soundness_forests):
    """claim (a) for all 29 functions: value and derivative with mpmath at 256 bits (its error is far below one float32 ulp, and every
    bound was moved outward by at least that), compared with no tolerance"""
    bad, skipped, checks = _check_claim_a(soundness_forests["all"], box, "mpmath")
    print(f"all box {box}: {checks} checks, {100 * skipped:.2f} % of the (tree, point) pairs skipped")
    assert not bad, bad[:5]
    assert checks > 30000


@pytest.mark.parametrize("box", range(3))
@pytest.mark.parametrize("funcs", ["arith", "shapes"])
def test_claim_b_monotone_roots(funcs, box, soundness_forests):
    """claim (b): a root with JUMP clear, value flags 0 and dlo >= 0 (dhi <= 0) is nondecreasing (nonincreasing) in x_v: the exact values
    at 32 pairs x < x' that differ in coordinate v only are ordered"""
    v, t, s = soundness_forests[funcs]
    lower, upper = IC.BOXES[box]
    vlo, vhi, vfl, dlo, dhi, dfl = DR.forest_derivative_intervals(v, t, s, lower, upper, [0, 1, 2])
    rng = np.random.default_rng([20261020, box])
    ex = DX.Exact("fraction", 3)
    bad, proven, moving = [], 0, 0
    for k in range(3):
        if lower[k] == upper[k]:
            continue
        for r in range(v.shape[0]):
            if vfl[r, 0] != 0 or dfl[k, r, 0] & (JUMP | MAL):
                continue
            up, down = dlo[k, r, 0] >= 0, dhi[k, r, 0] <= 0
            if not (up or down):
                continue
            proven += 1
            moving += bool(dfl[k, r, 0] & DEP) and not (up and down)
            a, b = DX.dyadic_points(rng, lower, upper, 32), DX.dyadic_points(rng, lower, upper, 32)
            for p, q in zip(a, b):
                if p[k] == q[k]:
                    continue
                x = list(p)
                y = list(p)
                x[k], y[k] = min(p[k], q[k]), max(p[k], q[k])
                fx, fy = ex.evaluate(v[r], t[r], s[r], x)[0].val, ex.evaluate(v[r], t[r], s[r], y)[0].val
                assert fx is not None and fy is not None, (r, k)       # value flags 0: defined on the whole box
                if (up and not fx <= fy) or (down and not fx >= fy):
                    bad.append((r, k, x, y, float(fx), float(fy)))
    print(f"{funcs} box {box}: {proven} (tree, variable) pairs proven monotone, {moving} of them strictly depend on the variable")
    assert not bad, bad[:3]
    assert proven > 100 and moving > 10


@pytest.mark.parametrize("box", range(2))
def test_polynomials_have_finite_bounds(box, oracle, rng):
    """non-vacuity: over + - * on a bounded box every endpoint of D is finite and JUMP is never set"""
    v, t, s = IC.oracle_forest(oracle, rng, 200, [R.F_ADD, R.F_SUB, R.F_MUL], key=50 + box, plant=0.0)
    vlo, vhi, vfl, dlo, dhi, dfl = DR.forest_derivative_intervals(v, t, s, *IC.BOXES[box], [0, 1, 2])
    live = np.broadcast_to(np.arange(v.shape[1])[None, :] < s[:, :1], dlo.shape)
    assert np.isfinite(dlo[live]).all() and np.isfinite(dhi[live]).all() and not (dfl & (JUMP | MAL)).any() and not vfl.any()
    assert (dfl[live] & DEP).sum() > 1000 and (dlo <= dhi).all()
    assert np.isfinite(vlo).all() and np.isfinite(vhi).all()


def test_monotone_mask_of_the_restatement():
    exprs = [B(R.F_ADD, V(0), V(1)), B(R.F_SUB, V(1), V(0)), B(R.F_MUL, V(0), V(0)), B(R.F_DIV, V(0), V(1)), B(R.F_LT, V(0), C(0.0)),
             B(R.F_MUL, V(0), C(3.0))]
    v, t, s = IC.rows(exprs, 8)
    o = DR.forest_derivative_intervals(v, t, s, [-1, -1], [1, 1], [0])
    assert DR.monotone(*o, [(0.0, np.inf)]).tolist() == [True, False, False, False, False, True]
    assert DR.monotone(*o, [(-np.inf, 0.0)]).tolist() == [False, True, False, False, False, False]
    assert DR.monotone(*o, [(-2.5, 2.5)]).tolist() == [True, True, True, False, False, False]
    assert DR.monotone(*o, [(0.0, np.inf)], max_abs=2.5).tolist() == [True, False, False, False, False, False]
    assert Fraction(1, 2) == DX.as_fraction(F(0.5))
