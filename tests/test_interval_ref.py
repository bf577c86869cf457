"""CPU: the numpy restatement of the interval pass (tests/interval_ref.py) against hand cases and against the C oracle's evaluations:
attainment for the exact functions and the soundness claim on every subtree of random trees, with no tolerance."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import interval_cases as IC  # noqa: E402
import interval_ref as IR  # noqa: E402
import sr_grad_ref as R  # noqa: E402
from interval_cases import B, C, IF, U, V  # noqa: E402

F = np.float32
INF = F(np.inf)


def _one(expr, lower, upper, L=16, **kw):
    v, t, s = IC.rows([expr], L)
    lo, hi, fl = IR.forest_intervals(v, t, s, lower, upper, **kw)
    return lo[0], hi[0], fl[0]


def _root(expr, lower, upper, **kw):
    lo, hi, fl = _one(expr, lower, upper, **kw)
    return lo[0], hi[0], int(fl[0])


def test_add_and_mul():
    assert _root(B(R.F_ADD, V(0), V(1)), [1, 3], [2, 5]) == (F(4), F(7), 0)
    assert _root(B(R.F_MUL, V(0), V(1)), [-2, -1], [3, 4]) == (F(-8), F(12), 0)
    assert _root(B(R.F_MUL, V(0), V(1)), [-3, -5], [-2, 4]) == (F(-12), F(15), 0)
    # 0 x inf counts as 0 and sets MAY_NAN
    lo, hi, fl = _root(B(R.F_MUL, V(0), C(np.inf)), [0], [1])
    assert (lo, hi, fl) == (F(0), INF, IR.MAY_NAN)


def test_division():
    lo, hi, fl = _root(B(R.F_DIV, V(0), V(1)), [1, 1], [3, 2])
    assert fl == 0 and lo == np.nextafter(F(1) / F(2), -INF) and hi == np.nextafter(F(3) / F(1), INF)
    assert _root(B(R.F_DIV, V(0), V(1)), [1, -1], [3, 1]) == (-INF, INF, IR.MAY_NAN)
    lo, hi, fl = _root(U(R.F_INV, V(0)), [-4], [-2])
    assert fl == 0 and lo == np.nextafter(F(-0.5), -INF) and hi == np.nextafter(F(-0.25), INF)
    # the loose forms substitute +-kDelta and stay NaN-free
    lo, hi, fl = _root(B(R.F_LOOSE_DIV, V(0), V(1)), [1, -1], [1, 1])
    assert fl == 0 and lo == np.nextafter(F(1) / -IR.KDELTA, -INF) and hi == np.nextafter(F(1) / IR.KDELTA, INF)
    lo, hi, fl = _root(U(R.F_LOOSE_INV, V(0)), [2], [4])
    assert fl == 0 and lo == np.nextafter(F(0.25), -INF) and hi == np.nextafter(F(0.5), INF)


def test_no_dependency_tracking():
    """x0 - x0 is [lo - hi, hi - lo], not [0, 0]: the two operands are bounded independently (no dependency tracking)"""
    assert _root(B(R.F_SUB, V(0), V(0)), [1], [4]) == (F(-3), F(3), 0)


def test_sqrt_and_log():
    lo, hi, fl = _root(U(R.F_SQRT, V(0)), [-1], [4])
    assert (lo, hi, fl) == (F(0), F(2), IR.MAY_NAN)
    assert _root(U(R.F_LOOSE_SQRT, V(0)), [-9], [4]) == (F(0), F(3), 0)
    lo, hi, fl = _root(U(R.F_LOG, V(0)), [0], [1])
    assert lo == -INF and fl == 0 and hi == IR.step(F(0), IR.W_ULPS[R.F_LOG])
    assert _root(U(R.F_LOG, V(0)), [-1], [1])[2] == IR.MAY_NAN
    lo, hi, fl = _root(U(R.F_LOOSE_LOG, V(0)), [-1], [2])
    assert lo == -IR.KMAXVAL and fl == 0 and hi == IR.step(np.log(F(2)), IR.W_ULPS[R.F_LOOSE_LOG])
    assert _root(U(R.F_LOOSE_LOG, V(0)), [0], [0]) == (-IR.KMAXVAL, -IR.KMAXVAL, 0)


def test_nan_constants():
    assert _root(C(np.nan), [0], [1]) == (-INF, INF, IR.MAY_NAN)
    for f in (R.F_LT, R.F_GT, R.F_LE, R.F_GE):
        assert _root(B(f, C(np.nan), V(0)), [0], [1]) == (F(-1), F(-1), 0)
        assert _root(B(f, V(0), C(np.nan)), [0], [1]) == (F(-1), F(-1), 0)
    # a comparison stops a NaN that is only possible: the interval includes -1, the flag is clear
    lo, hi, fl = _root(B(R.F_LT, U(R.F_SQRT, V(0)), C(5.0)), [-1], [4])
    assert (lo, hi, fl) == (F(-1), F(1), 0)
    assert _root(B(R.F_MAX, C(np.nan), V(0)), [-2], [3]) == (F(-2), F(3), 0)
    assert _root(B(R.F_MIN, C(np.nan), V(0)), [-2], [3]) == (F(-2), F(3), 0)
    assert _root(B(R.F_MAX, V(0), C(np.nan)), [-2], [3])[2] == IR.MAY_NAN      # a NaN in the second operand is the result
    # max(sqrt(x0), x1): a NaN in the first operand yields the second, so the interval covers all of x1 and the flag is x1's
    assert _root(B(R.F_MAX, U(R.F_SQRT, V(0)), V(1)), [-1, -7], [4, -6]) == (F(-7), F(2), 0)
    assert _root(B(R.F_ADD, C(np.inf), C(-np.inf)), [0], [1])[2] == IR.MAY_NAN


def test_if_cases():
    assert _root(IF(C(1.0), V(0), V(1)), [1, 5], [2, 6]) == (F(1), F(2), 0)           # then only
    assert _root(IF(V(2), V(0), V(1)), [1, 5, -3], [2, 6, 0]) == (F(5), F(6), 0)       # else only (cond.hi <= 0)
    assert _root(IF(V(2), V(0), V(1)), [1, 5, -3], [2, 6, 1]) == (F(1), F(6), 0)       # hull
    assert _root(IF(C(np.nan), V(0), V(1)), [1, 5], [2, 6]) == (F(5), F(6), 0)         # NaN > 0 is false
    # cond.lo > 0 but possibly NaN: the hull, and the OR of the branches' flags
    lo, hi, fl = _root(IF(B(R.F_ADD, U(R.F_SQRT, V(0)), C(1.0)), U(R.F_LOG, V(0)), V(1)), [-1, 5], [4, 6])
    assert fl == IR.MAY_NAN and lo == -INF and hi == F(6)
    assert _root(IF(V(0), V(1), V(2), fid=7), [1, 2, 3], [1, 2, 3]) == (F(2), F(2), 0)  # any id of a ternary node is IF


def test_unknown_ids_malformed_rows_and_dead_words():
    assert _root(U(5, V(0)), [1], [2]) == (F(0), F(0), 0)          # a binary id on a unary node
    assert _root(B(20, V(0), C(np.nan)), [1], [2]) == (F(0), F(0), 0)
    v, t, s = IC.rows([B(R.F_ADD, V(0), V(0)), B(R.F_ADD, V(0), V(0)), B(R.F_ADD, V(0), V(0)), V(0)], 8)
    t[0, 2] = 3            # the stack discipline fails
    s[1, 0] = 2            # a live prefix that is not one tree
    s[2, 1] = 2            # a size word that is not the size of its subtree
    s[3, 0] = 0            # empty
    lo, hi, fl = IR.forest_intervals(v, t, s, [1], [2])
    for r, n in ((0, 3), (1, 2), (2, 3)):
        assert np.all(np.isnan(lo[r, :n])) and np.all(np.isnan(hi[r, :n])) and np.all(fl[r, :n] == 3)
        assert not lo[r, n:].any() and not hi[r, n:].any() and not fl[r, n:].any()
    assert np.isnan(lo[3, 0]) and np.isnan(hi[3, 0]) and fl[3, 0] == 3 and not lo[3, 1:].any() and not fl[3, 1:].any()
    assert not IR.safe(lo, hi, fl).any()


def test_safety():
    v, t, s = IC.rows([B(R.F_ADD, V(0), C(1.0)), B(R.F_DIV, C(1.0), V(0)), U(R.F_EXP, B(R.F_MUL, V(0), C(1e30))), U(R.F_SQRT, V(0))], 8)
    lo, hi, fl = IR.forest_intervals(v, t, s, [-1], [3])
    assert IR.safe(lo, hi, fl).tolist() == [True, False, False, False]
    assert IR.safe(lo, hi, fl, max_abs=3.5).tolist() == [False, False, False, False]
    assert IR.safe(lo, hi, fl, max_abs=4.0).tolist() == [True, False, False, False]


POINT = (np.array([0.7, 1.3, -0.4], np.float32),) * 2


@pytest.mark.parametrize("f", IC.ALL)
def test_point_box(f, oracle):
    """lower == upper: the interval contains the oracle's value and is at most 2 W(f) + 2 ulps wide (0 for the exact functions)"""
    v, t, s = IC.rows([IC.single_op(f)], 8)
    lo, hi, fl = IR.forest_intervals(v, t, s, *POINT)
    val = oracle.batch_evaluate(v, t, s, POINT[0][None, :], 1)[0, 0, 0]
    assert fl[0, 0] == 0 and lo[0, 0] <= val <= hi[0, 0], (f, lo[0, 0], val, hi[0, 0])
    width = int(IC.ulp_key(hi[0, 0]) - IC.ulp_key(lo[0, 0]))
    w = IR.widening(f)
    assert width <= (2 * w + 2 if w else 0), (f, width)


def _grid(lower, upper, n=33):
    axes = []
    for lo, hi in zip(lower, upper):
        a = np.linspace(float(lo), float(hi), n).astype(np.float32)
        a[0], a[-1] = lo, hi
        a[np.argmin(np.abs(a))] = 0.0 if lo <= 0 <= hi else a[np.argmin(np.abs(a))]
        axes.append(a)
    return np.array([[x, y] for x in axes[0] for y in axes[1]], np.float32)


@pytest.mark.parametrize("box", [([-2, -3], [1.5, 2]), ([0.25, -4], [3, -1]), ([-5, 1], [-0.5, 9]), ([-1, -1], [1, 1])])
def test_attainment(box, oracle):
    """single-operation trees over the rule-1 functions: the interval IS the range of the oracle's values on a 33 x 33 grid that holds
    the corners and 0 (the functions are monotone, or piecewise monotone with the break at 0)"""
    exprs = [IC.single_op(f, 2) for f in IC.EXACT_BINARY + IC.EXACT_UNARY]
    v, t, s = IC.rows(exprs, 4)
    lower, upper = np.array(box[0], np.float32), np.array(box[1], np.float32)
    lo, hi, fl = IR.forest_intervals(v, t, s, lower, upper)
    vals = oracle.batch_evaluate(v, t, s, _grid(lower, upper), 1)[:, :, 0]
    for r in range(len(exprs)):
        if np.isnan(vals[r]).all():      # (sqrt of a negative box: no value to attain)
            assert fl[r, 0] & IR.MAY_NAN
            continue
        assert lo[r, 0] == np.nanmin(vals[r]) and hi[r, 0] == np.nanmax(vals[r]), (exprs[r], lo[r, 0], hi[r, 0])
        assert bool(fl[r, 0] & IR.MAY_NAN) == bool(np.isnan(vals[r]).any())


@pytest.mark.parametrize("box", range(3))
@pytest.mark.parametrize("funcs", ["arith", "logic", "all"])
def test_soundness_fuzz(funcs, box, oracle, rng):
    """every subtree of 200 random trees, as a row of its own, on 256 points of the box: every value obeys the claim"""
    ids = {"arith": IC.ARITH, "logic": IC.LOGIC, "all": IC.ALL}[funcs]
    lower, upper = IC.BOXES[box]
    v, t, s = IC.oracle_forest(oracle, rng, 200, ids, key=box)
    lo, hi, fl = IR.forest_intervals(v, t, s, lower, upper)
    assert not (fl & IR.MALFORMED).any()
    sv, st, ss, where = IC.all_subtree_rows(v, t, s)
    X = IC.sample_points(rng, lower, upper)
    vals = oracle.batch_evaluate(sv, st, ss, X, 1)[:, :, 0]
    bad = [(int(a), int(b)) for k, (a, b) in enumerate(where) if not IR.obeys_claim(vals[k], lo[a, b], hi[a, b], fl[a, b])]
    assert not bad, bad[:5]
    assert len(where) > 1000 and 0 < IR.safe(lo, hi, fl).sum()
