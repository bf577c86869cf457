"""TEST-ONLY: the numpy restatement of derivative bounds over SR trees (csrc/sr_deriv.hip) -- and its DEFINITION: the kernels follow this
file.  It builds on the rule functions of tests/interval_ref.py, which it leaves untouched.

``forest_derivative_intervals(value, type, size, lower, upper, wrt, lib="float32", widen=True)`` ->
``(vlo, vhi, vflags, dlo, dhi, dflags)``: the first three (pop, L), the last three (K, pop, L) for the K variable indices ``wrt``.

TWO QUANTITIES PER NODE over the box ``lower[v] <= x[v] <= upper[v]``.

R(i) = [vlo, vhi] with value flags (MAY_NAN = 1, MALFORMED = 2): an enclosure of the REAL value of subtree i.  It is the rule of
interval_ref applied to the children's R, with one more step: the results of + - * sqrt loose_sqrt, whose endpoints interval_ref takes
from round-to-nearest operations, are moved one ulp outward with ``step`` (an outward infinity stays; a lower endpoint of +inf, the
rounding of a real product beyond FLT_MAX, leaves to FLT_MAX, which is what ``step`` does).  Exact and therefore not stepped:
  * an endpoint of a + or - one of whose two terms is 0 (so neither endpoint where an operand is the point [0, 0]; and [0, 1] + [0, 1]
    keeps its lower endpoint 0: x0 * x0 is provably nondecreasing on [0, 1]);
  * a * with a point-zero or point-one operand;
  * an endpoint 0 of a * all of whose zero corner products have a zero factor (0 * y = 0; a product of two nonzero endpoints that
    underflows to 0 is not exact);
  * the square root of an endpoint 0.
Without these exemptions an enclosure that starts at 0 would reach below it, and sqrt or log of it would gain a MAY_NAN that
interval_ref does not have.  The other rules are unchanged: divisions move one ulp outward from a correctly rounded quotient, library
functions W = 2 E + 1 from a value within E ulps of the real one.  R(i) contains the
interval of interval_ref (every rule is inclusion-monotone and the extra step only widens), so R bounds the fp32 value too.

D_v(i) = [dlo, dhi] with derivative flags (JUMP = 1, MALFORMED = 2, DEPENDS = 4), for each requested variable v.
  Claim (a): at every real x of the box at which every node of subtree i has a defined finite real value and the subtree is
  differentiable in x_v, d subtree_i / d x_v lies in [dlo, dhi].
  Claim (b): if JUMP is clear on D_v(i) and the value flags of node i are 0, the subtree is continuous in x_v on the box, so dlo >= 0
  means nondecreasing in x_v and dhi <= 0 nonincreasing.

All interval + - * / on these quantities are the R variants above (``d_add`` .. ``d_div``): outward rounded, the 0 x inf corner is 0, an
endpoint that would be a NaN is the outward infinity, and the value-style NaN flags are dropped: an unbounded derivative is just
[-inf, +inf] (FULL, "the fallback").  Operand order is part of the definition (it decides which of two equal zeros an endpoint is).

Rules (a, b, c the children, Q = R(i) the node's own enclosure, D(.) = D_v(.)); the flags are the OR of JUMP and DEPENDS over the children
that can be taken unless said otherwise:
  CONST [0, 0], 0.  VAR u: [1, 1] with DEPENDS if u == v, else [0, 0], 0.  Unknown function id: [0, 0], 0.
  Independence: a function node none of whose taken children has DEPENDS is [0, 0], 0, whatever the function.
  + - neg: D(a) +- D(b), -D(a).     *: D(a) R(b) + R(a) D(b).     /: (D(a) - Q D(b)) / R(b), FULL when R(b) holds 0.
  inv: -(Q Q) D(a), FULL when R(a) holds 0.   loose_div, loose_inv: as the strict one when the divisor's R does not meet
  [-kDelta, kDelta], else FULL with JUMP.
  abs: D(a) when R(a).lo >= 0, -D(a) when R(a).hi <= 0, else the hull of both.
  max, min: the winner's D and flags when the R intervals are strictly separated and the first operand's value flags are clear; a
  NaN-constant first operand gives the second operand's; else the hull of both with the flags ORed.
  < > <= >=: [0, 0]; JUMP when a DEPENDS child exists and R(i) is not a point.
  IF: interval_ref's decision on R(a): a decided branch gives that child's D and flags; else the hull of D(b), D(c), the flags of all
  three ORed, JUMP added when the condition has DEPENDS.
  sqrt: D(a) / (2 Q) when R(a).lo > 0, else FULL.  loose_sqrt: the same on |a| with the sign of a, FULL when R(a) holds 0.
  exp: Q D(a).  log: D(a) / R(a) when R(a).lo > 0, else FULL.  loose_log: the same when R(a) does not hold 0, else FULL with JUMP.
  sin: cos-rule(R(a)) D(a).  cos: -(sin-rule(R(a))) D(a).  tan: (1 + Q Q) D(a).
  sinh: D(a) cosh-rule(R(a)).  cosh: D(a) sinh-rule(R(a)).  tanh: ((1 - Q Q) cut to [0, 1]) D(a).
  pow, loose_pow: FULL for every DEPENDS case (the closed forms are not built: DESIGN 3.15, out of scope).

Choices this file makes where the rules leave one (all on the sound side: they only add JUMP):
  * max / min whose first operand may be a NaN (the interpreters then yield the second operand) and has DEPENDS: JUMP.
  * tan whose own enclosure Q has an infinite endpoint (a pole may lie inside the box): JUMP.
  * pow / loose_pow with DEPENDS whose base's R holds 0 (x^-1 is NaN-free in fp32 and has a pole): JUMP.
Malformed rows (the value pass decides): NaN bounds and MALFORMED on every live word, on word 0 for an empty row; dead words are 0."""
import numpy as np

import interval_ref as IR
from interval_ref import INF, KDELTA, MALFORMED, MAY_NAN, ONE, ZERO, fmax, fmin, step
from sr_grad_ref import (F_ABS, F_ADD, F_COS, F_COSH, F_DIV, F_EXP, F_GE, F_INV, F_LOG, F_LOOSE_DIV, F_LOOSE_INV, F_LOOSE_LOG, F_LOOSE_POW,
                         F_LOOSE_SQRT, F_LT, F_MAX, F_MIN, F_MUL, F_NEG, F_POW, F_SIN, F_SINH, F_SQRT, F_SUB, F_TAN, F_TANH, T_CONST,
                         decode)
from subtree_ref import live_len, well_formed

JUMP, DEPENDS = 1, 4
CARRY = JUMP | DEPENDS
F = np.float32
TWO = F(2.0)
FULL = (-INF, INF)


def _point(x, c):
    return x[0] == c and x[1] == c


def _out1(lo, hi):
    return step(lo, -1), step(hi, 1)


def r_unary(L, f, a):
    """interval_ref.unary, the results of sqrt / loose_sqrt one ulp outward"""
    lo, hi, fl = IR.unary(L, f, a)
    if f in (F_SQRT, F_LOOSE_SQRT):      # (sqrt(0) = 0 is exact: a zero endpoint stays, so no enclosure of a square root reaches below 0)
        lo, hi = (lo if lo == ZERO else step(lo, -1)), (hi if hi == ZERO else step(hi, 1))
    return lo, hi, fl


def r_binary(L, f, a, b, a_nan_const=False, b_nan_const=False):
    """interval_ref.binary, the results of + - * one ulp outward unless the operation is exact"""
    lo, hi, fl = IR.binary(L, f, a, b, a_nan_const, b_nan_const)
    if f in (F_ADD, F_SUB):      # an endpoint sum one of whose terms is 0 is exact (a point-zero operand makes both exact)
        blo, bhi = (b[0], b[1]) if f == F_ADD else (-b[1], -b[0])
        if not (a[0] == ZERO or blo == ZERO):
            lo = step(lo, -1)
        if not (a[1] == ZERO or bhi == ZERO):
            hi = step(hi, 1)
    elif f == F_MUL:
        if not (_point(a, ZERO) or _point(b, ZERO) or _point(a, ONE) or _point(b, ONE)):
            # an endpoint 0 is exact when every corner product that is 0 has a zero factor (none is an underflow)
            with np.errstate(all="ignore"):
                under = any(x != ZERO and y != ZERO and x * y == ZERO for x in (a[0], a[1]) for y in (b[0], b[1]))
            lo = lo if (lo == ZERO and not under) else step(lo, -1)
            hi = hi if (hi == ZERO and not under) else step(hi, 1)
    return lo, hi, fl


# ---- interval + - * / on derivative quantities: pairs (lo, hi), no flags --------------------------------------------------------------
def d_add(L, x, y):
    return r_binary(L, F_ADD, (x[0], x[1], 0), (y[0], y[1], 0))[:2]


def d_sub(L, x, y):
    return r_binary(L, F_SUB, (x[0], x[1], 0), (y[0], y[1], 0))[:2]


def d_mul(L, x, y):
    return r_binary(L, F_MUL, (x[0], x[1], 0), (y[0], y[1], 0))[:2]


def d_div(L, x, y):
    """FULL when y holds 0"""
    return r_binary(L, F_DIV, (x[0], x[1], 0), (y[0], y[1], 0))[:2]


def d_neg(x):
    return -x[1], -x[0]


def d_hull(x, y):
    return fmin(x[0], y[0]), fmax(x[1], y[1])


def _has_zero(r):
    return r[0] <= ZERO and r[1] >= ZERO


def _isinf(x):
    return x == INF or x == -INF


def d_unary(L, f, ra, q, da):
    """D and flags of a unary node that DEPENDS: ra = R(a), q = R(node), da = (lo, hi, flags) of the child"""
    d, fl = (da[0], da[1]), da[2] & CARRY
    if f == F_NEG:
        return d_neg(d), fl
    if f == F_ABS:
        if ra[0] >= ZERO:
            return d, fl
        if ra[1] <= ZERO:
            return d_neg(d), fl
        return d_hull(d, d_neg(d)), fl
    if f == F_SQRT:
        if ra[0] > ZERO:
            return d_div(L, d, d_mul(L, (TWO, TWO), q)), fl
        return FULL, fl
    if f == F_LOOSE_SQRT:
        if _has_zero(ra):
            return FULL, fl
        r = d_div(L, d, d_mul(L, (TWO, TWO), q))
        return (r if ra[0] > ZERO else d_neg(r)), fl
    if f == F_INV or f == F_LOOSE_INV:
        if f == F_LOOSE_INV and not (ra[0] > KDELTA or ra[1] < -KDELTA):
            return FULL, fl | JUMP
        if _has_zero(ra):
            return FULL, fl
        return d_neg(d_mul(L, d_mul(L, q, q), d)), fl
    if f == F_EXP:
        return d_mul(L, q, d), fl
    if f == F_LOG or f == F_LOOSE_LOG:
        if f == F_LOOSE_LOG and _has_zero(ra):
            return FULL, fl | JUMP
        if ra[0] > ZERO or (f == F_LOOSE_LOG and ra[1] < ZERO):
            return d_div(L, d, ra), fl
        return FULL, fl
    if f == F_SIN:
        return d_mul(L, IR.unary(L, F_COS, (ra[0], ra[1], 0))[:2], d), fl
    if f == F_COS:
        return d_mul(L, d_neg(IR.unary(L, F_SIN, (ra[0], ra[1], 0))[:2]), d), fl
    if f == F_TAN:
        if _isinf(q[0]) or _isinf(q[1]):
            fl |= JUMP
        return d_mul(L, d_add(L, (ONE, ONE), d_mul(L, q, q)), d), fl
    if f == F_SINH:
        return d_mul(L, d, IR.unary(L, F_COSH, (ra[0], ra[1], 0))[:2]), fl
    if f == F_COSH:
        return d_mul(L, d, IR.unary(L, F_SINH, (ra[0], ra[1], 0))[:2]), fl
    if f == F_TANH:
        s = d_sub(L, (ONE, ONE), d_mul(L, q, q))
        return d_mul(L, (fmax(s[0], ZERO), fmin(s[1], ONE)), d), fl
    raise AssertionError(f)


def d_binary(L, f, ra, rb, q, da, db, a_nan_const):
    """(D, flags, taken) of a binary node; the caller applies the independence rule to the children in ``taken``"""
    xa, xb = (da[0], da[1]), (db[0], db[1])
    fa, fb = da[2] & CARRY, db[2] & CARRY
    both = fa | fb
    if f == F_ADD:
        return d_add(L, xa, xb), both
    if f == F_SUB:
        return d_sub(L, xa, xb), both
    if f == F_MUL:
        return d_add(L, d_mul(L, xa, rb), d_mul(L, ra, xb)), both
    if f == F_DIV or f == F_LOOSE_DIV:
        if f == F_LOOSE_DIV and not (rb[0] > KDELTA or rb[1] < -KDELTA):
            return FULL, both | JUMP
        if _has_zero(rb):
            return FULL, both
        return d_div(L, d_sub(L, xa, d_mul(L, q, xb)), rb), both
    if f == F_POW or f == F_LOOSE_POW:
        return FULL, both | (JUMP if _has_zero(ra) else 0)
    if f == F_MAX or f == F_MIN:
        if a_nan_const:
            return xb, fb
        if not (ra[2] & MAY_NAN):
            a_over_b, b_over_a = ra[0] > rb[1], ra[1] < rb[0]
            if (a_over_b if f == F_MAX else b_over_a):
                return xa, fa
            if (b_over_a if f == F_MAX else a_over_b):
                return xb, fb
        return d_hull(xa, xb), both | (JUMP if (ra[2] & MAY_NAN) and (fa & DEPENDS) else 0)
    if F_LT <= f <= F_GE:
        return (ZERO, ZERO), both | (JUMP if (both & DEPENDS) and q[0] != q[1] else 0)
    raise AssertionError(f)


def d_ternary(ra, da, db, dc, a_nan_const):
    if a_nan_const or ra[1] <= ZERO:
        return (dc[0], dc[1]), dc[2] & CARRY
    if ra[0] > ZERO and not (ra[2] & MAY_NAN):
        return (db[0], db[1]), db[2] & CARRY
    fl = (da[2] | db[2] | dc[2]) & CARRY
    return d_hull((db[0], db[1]), (dc[0], dc[1])), fl | (JUMP if da[2] & DEPENDS else 0)


def _children(i, arity, size):
    kids, c = [], i + 1
    for _ in range(arity):
        kids.append(c)
        c += int(size[c])
    return kids, c - i


def tree_enclosures(value, type_, size, lower, upper, lib="float32", widen=True):
    """one row -> (vlo[L], vhi[L], vflags[L]): interval_ref.tree_intervals with the outward rules"""
    Lb = IR._Lib(lib, widen)
    L = len(value)
    var_len = len(lower)
    lo, hi, fl = np.zeros(L, np.float32), np.zeros(L, np.float32), np.zeros(L, np.uint8)
    n = live_len(size, L)
    ok = well_formed(type_, n)
    if ok:
        for i in reversed(range(n)):
            kind, pay, _ = decode(type_[i], value[i], False, var_len, 1)
            span = 1
            if kind == "C":
                v = F(pay)
                r = (-INF, INF, MAY_NAN) if v != v else (v, v, 0)
            elif kind == "V":
                r = (F(lower[pay]), F(upper[pay]), 0)
            else:
                kids, span = _children(i, {"U": 1, "B": 2, "T": 3}[kind], size)
                ops = [(lo[k], hi[k], int(fl[k])) for k in kids]
                nanc = [int(type_[k]) == T_CONST and bool(np.isnan(value[k])) for k in kids]
                if kind == "U":
                    r = r_unary(Lb, pay, ops[0])
                elif kind == "B":
                    r = r_binary(Lb, pay, ops[0], ops[1], nanc[0], nanc[1])
                else:
                    r = IR.ternary(ops[0], ops[1], ops[2], nanc[0])
            if int(size[i]) != span:
                ok = False
                break
            lo[i], hi[i], fl[i] = r
    if not ok:
        m = max(n, 1)
        lo[:m], hi[:m], fl[:m] = np.nan, np.nan, MAY_NAN | MALFORMED
    return lo, hi, fl


def tree_derivatives(value, type_, size, var_len, v, vlo, vhi, vfl, lib="float32", widen=True):
    """one row, one variable -> (dlo[L], dhi[L], dflags[L]) from the row's enclosures"""
    Lb = IR._Lib(lib, widen)
    L = len(value)
    lo, hi, fl = np.zeros(L, np.float32), np.zeros(L, np.float32), np.zeros(L, np.uint8)
    n = live_len(size, L)
    if int(vfl[0]) & MALFORMED:
        m = max(n, 1)
        lo[:m], hi[:m], fl[:m] = np.nan, np.nan, MALFORMED
        return lo, hi, fl
    for i in reversed(range(n)):
        kind, pay, _ = decode(type_[i], value[i], False, var_len, 1)
        if kind == "C":
            d, f = (ZERO, ZERO), 0
        elif kind == "V":
            d, f = ((ONE, ONE), DEPENDS) if pay == v else ((ZERO, ZERO), 0)
        else:
            kids, _ = _children(i, {"U": 1, "B": 2, "T": 3}[kind], size)
            R = [(vlo[k], vhi[k], int(vfl[k])) for k in kids]
            D = [(lo[k], hi[k], int(fl[k])) for k in kids]
            q = (vlo[i], vhi[i])
            nanc = int(type_[kids[0]]) == T_CONST and bool(np.isnan(value[kids[0]]))
            if kind != "T" and pay is None:
                d, f = (ZERO, ZERO), 0
            elif kind == "U":
                d, f = d_unary(Lb, pay, R[0], q, D[0]) if D[0][2] & DEPENDS else ((ZERO, ZERO), 0)
            elif kind == "B":
                d, f = d_binary(Lb, pay, R[0], R[1], q, D[0], D[1], nanc)
            else:
                d, f = d_ternary(R[0], D[0], D[1], D[2], nanc)
            if not (f & DEPENDS):      # independence: no taken child depends on x_v
                d, f = (ZERO, ZERO), 0
        lo[i], hi[i], fl[i] = d[0], d[1], f
    return lo, hi, fl


def forest_enclosures(value, type_, size, lower, upper, lib="float32", widen=True):
    value, type_, size = np.asarray(value, np.float32), np.asarray(type_, np.int16), np.asarray(size, np.int16)
    lower, upper = np.asarray(lower, np.float32).reshape(-1), np.asarray(upper, np.float32).reshape(-1)
    pop, L = value.shape
    lo, hi, fl = np.zeros((pop, L), np.float32), np.zeros((pop, L), np.float32), np.zeros((pop, L), np.uint8)
    for t in range(pop):
        lo[t], hi[t], fl[t] = tree_enclosures(value[t], type_[t], size[t], lower, upper, lib, widen)
    return lo, hi, fl


def forest_derivative_intervals(value, type_, size, lower, upper, wrt, lib="float32", widen=True):
    value, type_, size = np.asarray(value, np.float32), np.asarray(type_, np.int16), np.asarray(size, np.int16)
    lower = np.asarray(lower, np.float32).reshape(-1)
    wrt = [int(v) for v in np.asarray(wrt).reshape(-1)]
    pop, L = value.shape
    vlo, vhi, vfl = forest_enclosures(value, type_, size, lower, upper, lib, widen)
    K = len(wrt)
    dlo, dhi, dfl = np.zeros((K, pop, L), np.float32), np.zeros((K, pop, L), np.float32), np.zeros((K, pop, L), np.uint8)
    for k, v in enumerate(wrt):
        assert 0 <= v < len(lower)
        for t in range(pop):
            dlo[k, t], dhi[k, t], dfl[k, t] = tree_derivatives(value[t], type_[t], size[t], len(lower), v, vlo[t], vhi[t], vfl[t], lib, widen)
    return vlo, vhi, vfl, dlo, dhi, dfl


def monotone(vlo, vhi, vfl, dlo, dhi, dfl, bounds, max_abs=float("inf")):
    """Forest.monotone_mask on the roots: ``bounds`` is one (dmin, dmax) per slice of the derivative outputs"""
    ok = IR.safe(vlo, vhi, vfl, max_abs)
    for k, (dmin, dmax) in enumerate(bounds):
        with np.errstate(invalid="ignore"):
            ok &= ((dfl[k, :, 0] & (JUMP | MALFORMED)) == 0) & (dlo[k, :, 0] >= dmin) & (dhi[k, :, 0] <= dmax)
    return ok
