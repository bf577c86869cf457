"""TEST-ONLY: the numpy restatement of interval arithmetic over SR trees (csrc/sr_interval.hip) -- and its DEFINITION: the kernel follows
this file.

``forest_intervals(value, type, size, lower, upper, lib="float32", widen=True)`` -> ``(lo, hi, flags)``, each (pop, L): for every node
i of the live prefix of every single-output tree a float32 interval [lo, hi] (endpoints in [-inf, +inf]) and a flag byte
(MAY_NAN = 1, MALFORMED = 2) over the box ``lower[v] <= x[v] <= upper[v]``.

THE CLAIM.  For every float32 input vector x inside the box, the float32 value V any of the engine's interpreters computes for the
subtree rooted at i is either a NaN with MAY_NAN set, or lies in [lo, hi] (V is +-inf only where the matching endpoint is).  The
intervals bound the values AS COMPUTED IN FP32, not the real-valued function.

The walk goes from the last live node to node 0; child 1 of i is i + 1, child 2 is i + 1 + size[i + 1], child 3 follows child 2 the
same way.  Operand order is interp.hpp's: the first child is the left operand ``a`` (for IF: the condition), the second ``b`` (then),
the third ``c`` (else).  Every endpoint operation is a float32 round-to-nearest operation, every comparison and every min / max is
written out (``fmin`` / ``fmax`` below pin which of two equal zeros is taken), so that the kernel reproduces the exact tier bit for bit.

Choices this file makes where the issue's rules leave one (all on the sound side):
  * ``step(x, k)``: k times ``nextafter``; -0.0 and +0.0 are one point (the step from either is the smallest denormal, a step that lands
    on zero gives +0.0), +-inf is the end of the line (a step outward stays, a step inward leaves to +-FLT_MAX).
  * A row is MALFORMED when its type words fail the stack discipline of the tape kernels (``subtree_ref.well_formed``) OR a size word of
    the live prefix is not the size of its subtree: the walk finds children from the size words, so it only trusts verified ones (a node
    is verified before any parent uses it, hence no child index ever leaves the live prefix).  A row with no live node (size[0] <= 0)
    marks word 0 alone, so that word 0 of every row tells whether the row is safe.
  * An endpoint operation that would give a NaN (inf - inf) gives the outward infinity, with MAY_NAN.  An interval none of whose values is
    defined (sqrt / log of hi < 0, inf / inf of two point intervals) is [-inf, +inf] with MAY_NAN.
  * ``x * y``: MAY_NAN whenever one operand's interval contains 0 and the other has an infinite endpoint (the 0 need not be an endpoint).
  * A CONST node whose value is a NaN is [-inf, +inf] with MAY_NAN for every consumer but three, which look at the node itself: a
    comparison with such an operand is exactly -1; ``max`` / ``min`` whose FIRST operand is one is exactly its second operand; IF whose
    condition is one is exactly its else child.  (``max(a, b) = a >= b ? a : b``: a NaN in a yields b, a NaN in b yields b = NaN.)
  * ``max`` / ``min`` with MAY_NAN on the first operand: the hull with all of the second operand; the flag is the second operand's.
  * sin / cos / tan of an interval with an infinite endpoint: the full range ([-1, 1] widened, or [-inf, +inf]) with MAY_NAN.
  * The trig tests run in float64 with +, -, /, floor, ceil only: u = (x - phase) / period for both endpoints; an extremum (pole) lies
    inside iff ceil(u_lo) <= floor(u_hi).  |x| <= 2^20 makes |u| < 2^18 with an absolute error below 2^-33; the safety margin 2^-20 on
    "u within the margin of an integer" covers it and the distance from the float32 endpoint to the float64 extremum's true place.
  * exp is widened like the others: its lower endpoint may be a negative denormal (no clamp at 0).
  * log: lo <= 0 gives lower endpoint -inf; MAY_NAN only where lo < 0 (log(-0.0) = log(0.0) = -inf, not a NaN).
  * loose_inv / loose_div: an interval containing 0 may hold either zero, so both copysign branches (+-kDelta) are taken.
  * pow(a, b): (1) a.lo > 0, or a.lo >= 0 and b.lo > 0: a^b is monotone in each argument, so the four corners, widened by W(pow);
    (2) b a point interval holding a finite integer n: even n through |a|; odd n > 0 monotone increasing on the whole line; odd n < 0
    monotone decreasing on either side of 0, [-inf, +inf] (NaN-free) over an interval containing 0; (3) anything else [-inf, +inf] with
    MAY_NAN.  loose_pow: the corners of (|a|, b), hulled with 0 when both intervals contain 0.
  * Library functions (rule 4) are moved outward by W(f) = 2 E(f) + 1 ulps, divisions by 1 ulp; the rule-1 functions not at all.

``lib="float64"`` takes the library functions' endpoint values from float64 numpy rounded once to float32 (the GPU library tier compares
against it: the device's values lie within E(f) ulps of those); ``widen=False`` leaves the library widening (not the divisions') out."""
import numpy as np

from sr_grad_ref import (DELTA, MAXVAL, F_ABS, F_ADD, F_COS, F_COSH, F_DIV, F_EXP, F_GE, F_GT, F_INV, F_LE, F_LOG, F_LOOSE_DIV,
                         F_LOOSE_INV, F_LOOSE_LOG, F_LOOSE_POW, F_LOOSE_SQRT, F_LT, F_MAX, F_MIN, F_MUL, F_NEG, F_POW, F_SIN, F_SINH,
                         F_SQRT, F_SUB, F_TAN, F_TANH, T_CONST, decode)
from subtree_ref import live_len, well_formed

MAY_NAN, MALFORMED = 1, 2
F = np.float32
INF, ZERO, ONE = F(np.inf), F(0.0), F(1.0)
KDELTA, KMAXVAL = F(DELTA), F(MAXVAL)

# documented OCML bounds E(f) in ulps (tests/ulp_bounds.py) and W(f) = 2 E(f) + 1; csrc/sr_interval.hpp holds the same table
E_ULPS = {F_SIN: 4, F_COS: 4, F_TAN: 5, F_SINH: 5, F_COSH: 5, F_TANH: 5, F_LOG: 3, F_LOOSE_LOG: 3, F_EXP: 3, F_POW: 16, F_LOOSE_POW: 16}
W_ULPS = {f: 2 * e + 1 for f, e in E_ULPS.items()}
W_DIV = 1
TRIG_MAX = 1048576.0          # 2^20
TRIG_MARGIN = 2.0 ** -20
PI = float(np.pi)
TWO_PI = 2.0 * PI
HALF_PI = 0.5 * PI


def widening(f):
    """ulps by which function id f moves its endpoints outward (0: exact)"""
    if f in W_ULPS:
        return W_ULPS[f]
    return W_DIV if f in (F_DIV, F_LOOSE_DIV, F_INV, F_LOOSE_INV) else 0


def fmin(a, b):
    return b if b < a else a


def fmax(a, b):
    return b if b > a else a


def step(x, k):
    """x moved by k ulps (k < 0: down), see the module docstring"""
    s = int(np.array(x, np.float32).view(np.int32))
    key = s if s >= 0 else -(s & 0x7FFFFFFF)
    key = min(max(key + k, -0x7F800000), 0x7F800000)
    bits = key if key >= 0 else (0x80000000 | -key)
    return np.array(bits, np.uint32).view(np.float32)[()]


def _isinf(x):
    return x == INF or x == -INF


class _Lib:
    def __init__(self, lib, widen):
        assert lib in ("float32", "float64")
        self.dt = np.float32 if lib == "float32" else np.float64
        self.widen = widen

    def call(self, fn, *xs):
        with np.errstate(all="ignore"):
            return F(fn(*(self.dt(x) for x in xs)))

    def out(self, lo, hi, w):
        return (step(lo, -w), step(hi, w)) if self.widen else (lo, hi)


def iabs(lo, hi):
    if lo >= ZERO:
        return np.abs(lo), np.abs(hi)
    if hi <= ZERO:
        return np.abs(hi), np.abs(lo)
    return ZERO, fmax(np.abs(lo), hi)


def _has_zero(lo, hi):
    return lo <= ZERO and hi >= ZERO


def _inside(u_lo, u_hi):
    """(an integer lies in [u_lo, u_hi], an endpoint lies within the margin of an integer): float64"""
    near = abs(u_lo - np.floor(u_lo + 0.5)) <= TRIG_MARGIN or abs(u_hi - np.floor(u_hi + 0.5)) <= TRIG_MARGIN
    return bool(np.ceil(u_lo) <= np.floor(u_hi)), bool(near)


def _sincos(L, f, lo, hi, fl):
    w = W_ULPS[f]
    full = L.out(-ONE, ONE, w)
    if _isinf(lo) or _isinf(hi):
        return full[0], full[1], fl | MAY_NAN
    dlo, dhi = float(lo), float(hi)
    if dhi - dlo >= TWO_PI or abs(dlo) > TRIG_MAX or abs(dhi) > TRIG_MAX:
        return full[0], full[1], fl
    top, bottom = (HALF_PI, -HALF_PI) if f == F_SIN else (0.0, PI)
    has_max, near1 = _inside((dlo - top) / TWO_PI, (dhi - top) / TWO_PI)
    has_min, near2 = _inside((dlo - bottom) / TWO_PI, (dhi - bottom) / TWO_PI)
    if near1 or near2:
        return full[0], full[1], fl
    fn = np.sin if f == F_SIN else np.cos
    vlo, vhi = L.call(fn, lo), L.call(fn, hi)
    rlo = -ONE if has_min else fmin(vlo, vhi)
    rhi = ONE if has_max else fmax(vlo, vhi)
    rlo, rhi = L.out(rlo, rhi, w)
    return rlo, rhi, fl


def _tan(L, lo, hi, fl):
    if _isinf(lo) or _isinf(hi):
        return -INF, INF, fl | MAY_NAN
    dlo, dhi = float(lo), float(hi)
    if dhi - dlo >= PI or abs(dlo) > TRIG_MAX or abs(dhi) > TRIG_MAX:
        return -INF, INF, fl
    pole, near = _inside((dlo - HALF_PI) / PI, (dhi - HALF_PI) / PI)
    if pole or near:
        return -INF, INF, fl
    rlo, rhi = L.out(L.call(np.tan, lo), L.call(np.tan, hi), W_ULPS[F_TAN])
    return rlo, rhi, fl


def _loose_divisor(lo, hi):
    """the intervals (at most two, neither containing 0) of d = |b| <= kDelta ? copysign(kDelta, b) : b for b in [lo, hi]"""
    parts = []
    if lo <= ZERO:
        parts.append((fmin(lo, -KDELTA), fmin(hi, -KDELTA)))
    if hi >= ZERO:
        parts.append((fmax(lo, KDELTA), fmax(hi, KDELTA)))
    return parts


def _quotients(alo, ahi, dlo, dhi):
    """min and max of the four corner quotients, NaN corners (inf / inf) skipped; None when every corner is a NaN"""
    best = None
    with np.errstate(all="ignore"):
        for x in (alo, ahi):
            for y in (dlo, dhi):
                q = x / y
                if q != q:
                    continue
                best = (q, q) if best is None else (fmin(best[0], q), fmax(best[1], q))
    return best


def _divide(alo, ahi, parts, fl):
    """a / d over the divisor intervals ``parts`` (none contains 0), one ulp outward"""
    rlo = rhi = None
    for dlo, dhi in parts:
        if (_isinf(alo) or _isinf(ahi)) and (_isinf(dlo) or _isinf(dhi)):
            fl |= MAY_NAN
        q = _quotients(alo, ahi, dlo, dhi)
        if q is None:
            return -INF, INF, fl | MAY_NAN
        rlo, rhi = (q[0], q[1]) if rlo is None else (fmin(rlo, q[0]), fmax(rhi, q[1]))
    return step(rlo, -W_DIV), step(rhi, W_DIV), fl


def _pow_corners(L, alo, ahi, blo, bhi):
    """a^b over alo >= +0: monotone in each argument"""
    c = [L.call(np.power, x, y) for x in (alo, ahi) for y in (blo, bhi)]
    lo = fmin(fmin(c[0], c[1]), fmin(c[2], c[3]))
    hi = fmax(fmax(c[0], c[1]), fmax(c[2], c[3]))
    return L.out(lo, hi, W_ULPS[F_POW])


def _pow(L, alo, ahi, blo, bhi, fl):
    if alo > ZERO or (alo >= ZERO and blo > ZERO):
        lo, hi = _pow_corners(L, np.abs(alo), ahi, blo, bhi)
        return lo, hi, fl
    if blo == bhi and not _isinf(blo) and blo == np.trunc(blo):
        n = blo
        half = n * F(0.5)
        if half == np.trunc(half):                      # even
            mlo, mhi = iabs(alo, ahi)
            lo, hi = _pow_corners(L, mlo, mhi, n, n)
            return lo, hi, fl
        if n > ZERO:
            lo, hi = L.out(L.call(np.power, alo, n), L.call(np.power, ahi, n), W_ULPS[F_POW])
            return lo, hi, fl
        if _has_zero(alo, ahi):
            return -INF, INF, fl
        lo, hi = L.out(L.call(np.power, ahi, n), L.call(np.power, alo, n), W_ULPS[F_POW])
        return lo, hi, fl
    return -INF, INF, fl | MAY_NAN


def unary(L, f, a):
    lo, hi, fl = a
    if f is None:
        return ZERO, ZERO, 0
    with np.errstate(all="ignore"):
        if f == F_NEG:
            return -hi, -lo, fl
        if f == F_ABS:
            m = iabs(lo, hi)
            return m[0], m[1], fl
        if f in (F_SQRT, F_LOOSE_SQRT):
            if f == F_LOOSE_SQRT:
                lo, hi = iabs(lo, hi)
            if hi < ZERO:
                return -INF, INF, fl | MAY_NAN
            if lo < ZERO:
                lo, fl = ZERO, fl | MAY_NAN
            return np.sqrt(lo), np.sqrt(hi), fl
        if f == F_INV:
            if _has_zero(lo, hi):
                return -INF, INF, fl | MAY_NAN
            return _divide(ONE, ONE, [(lo, hi)], fl)
        if f == F_LOOSE_INV:
            return _divide(ONE, ONE, _loose_divisor(lo, hi), fl)
        if f in (F_SIN, F_COS):
            return _sincos(L, f, lo, hi, fl)
        if f == F_TAN:
            return _tan(L, lo, hi, fl)
        if f in (F_SINH, F_TANH, F_EXP):
            fn = {F_SINH: np.sinh, F_TANH: np.tanh, F_EXP: np.exp}[f]
            rlo, rhi = L.out(L.call(fn, lo), L.call(fn, hi), W_ULPS[f])
            return rlo, rhi, fl
        if f == F_COSH:
            mlo, mhi = iabs(lo, hi)
            rlo, rhi = L.out(L.call(np.cosh, mlo), L.call(np.cosh, mhi), W_ULPS[f])
            return rlo, rhi, fl
        if f == F_LOG:
            if hi < ZERO:
                return -INF, INF, fl | MAY_NAN
            if lo < ZERO:
                fl |= MAY_NAN
            rlo, rhi = L.out(L.call(np.log, lo) if lo > ZERO else -INF, L.call(np.log, hi), W_ULPS[f])
            return rlo, rhi, fl
        if f == F_LOOSE_LOG:
            zero = _has_zero(lo, hi)
            mlo, mhi = iabs(lo, hi)
            if mhi == ZERO:
                return -KMAXVAL, -KMAXVAL, fl
            rlo, rhi = L.out(-INF if zero else L.call(np.log, mlo), L.call(np.log, mhi), W_ULPS[f])
            return (-KMAXVAL if zero else rlo), rhi, fl      # (log|a| of the smallest denormal is -103.3 > -kMaxVal)
    raise AssertionError(f)


def _compare(f, a, b):
    alo, ahi, afl = a
    blo, bhi, bfl = b
    nan = bool((afl | bfl) & MAY_NAN)
    if f == F_LT:
        can_t, can_f = alo < bhi, not (ahi < blo)
    elif f == F_GT:
        can_t, can_f = ahi > blo, not (alo > bhi)
    elif f == F_LE:
        can_t, can_f = alo <= bhi, not (ahi <= blo)
    else:
        can_t, can_f = ahi >= blo, not (alo >= bhi)
    can_f = can_f or nan
    return (-ONE if can_f else ONE), (ONE if can_t else -ONE), 0


def binary(L, f, a, b, a_nan_const=False, b_nan_const=False):
    alo, ahi, afl = a
    blo, bhi, bfl = b
    if f is None:
        return ZERO, ZERO, 0
    fl = (afl | bfl) & MAY_NAN
    a_inf, b_inf = _isinf(alo) or _isinf(ahi), _isinf(blo) or _isinf(bhi)
    with np.errstate(all="ignore"):
        if f == F_ADD or f == F_SUB:
            if f == F_SUB:
                blo, bhi = -bhi, -blo
            if (ahi == INF and blo == -INF) or (alo == -INF and bhi == INF):
                fl |= MAY_NAN
            lo, hi = alo + blo, ahi + bhi
            return (-INF if lo != lo else lo), (INF if hi != hi else hi), fl
        if f == F_MUL:
            if (_has_zero(alo, ahi) and b_inf) or (_has_zero(blo, bhi) and a_inf):
                fl |= MAY_NAN
            c = []
            for x in (alo, ahi):
                for y in (blo, bhi):
                    c.append(ZERO if (x == ZERO and _isinf(y)) or (y == ZERO and _isinf(x)) else x * y)
            return fmin(fmin(c[0], c[1]), fmin(c[2], c[3])), fmax(fmax(c[0], c[1]), fmax(c[2], c[3])), fl
        if f == F_DIV:
            if _has_zero(blo, bhi):
                return -INF, INF, fl | MAY_NAN
            return _divide(alo, ahi, [(blo, bhi)], fl)
        if f == F_LOOSE_DIV:
            return _divide(alo, ahi, _loose_divisor(blo, bhi), fl)
        if f == F_POW:
            return _pow(L, alo, ahi, blo, bhi, fl)
        if f == F_LOOSE_POW:
            mlo, mhi = iabs(alo, ahi)
            lo, hi = _pow_corners(L, mlo, mhi, blo, bhi)
            if _has_zero(alo, ahi) and _has_zero(blo, bhi):
                lo, hi = fmin(lo, ZERO), fmax(hi, ZERO)
            return lo, hi, fl
        if f == F_MAX or f == F_MIN:
            if a_nan_const:
                return blo, bhi, bfl
            if f == F_MAX:
                lo, hi = fmax(alo, blo), fmax(ahi, bhi)
                if afl & MAY_NAN:
                    lo = fmin(lo, blo)
            else:
                lo, hi = fmin(alo, blo), fmin(ahi, bhi)
                if afl & MAY_NAN:
                    hi = fmax(hi, bhi)
            return lo, hi, bfl & MAY_NAN
        if F_LT <= f <= F_GE:
            if a_nan_const or b_nan_const:
                return -ONE, -ONE, 0
            return _compare(f, a, b)
    raise AssertionError(f)


def ternary(a, b, c, a_nan_const=False):
    alo, ahi, afl = a
    if a_nan_const or ahi <= ZERO:
        return c
    if alo > ZERO and not (afl & MAY_NAN):
        return b
    return fmin(b[0], c[0]), fmax(b[1], c[1]), (b[2] | c[2]) & MAY_NAN


def tree_intervals(value, type_, size, lower, upper, lib="float32", widen=True):
    """one row -> (lo[L], hi[L], flags[L])"""
    Lb = _Lib(lib, widen)
    L = len(value)
    var_len = len(lower)
    lo, hi, fl = np.zeros(L, np.float32), np.zeros(L, np.float32), np.zeros(L, np.uint8)
    n = live_len(size, L)
    ok = well_formed(type_, n)
    if ok:
        for i in reversed(range(n)):
            kind, pay, _ = decode(type_[i], value[i], False, var_len, 1)
            if kind == "C":
                v = F(pay)
                r = (-INF, INF, MAY_NAN) if v != v else (v, v, 0)
                span = 1
            elif kind == "V":
                r = (F(lower[pay]), F(upper[pay]), 0)
                span = 1
            else:
                kids = []
                c = i + 1
                for _ in range({"U": 1, "B": 2, "T": 3}[kind]):
                    kids.append(c)
                    c += int(size[c])
                span = c - i
                ops = [(lo[k], hi[k], int(fl[k])) for k in kids]
                nanc = [int(type_[k]) == T_CONST and bool(np.isnan(value[k])) for k in kids]
                if kind == "U":
                    r = unary(Lb, pay, ops[0])
                elif kind == "B":
                    r = binary(Lb, pay, ops[0], ops[1], nanc[0], nanc[1])
                else:
                    r = ternary(ops[0], ops[1], ops[2], nanc[0])
            if int(size[i]) != span:
                ok = False
                break
            lo[i], hi[i], fl[i] = r
    if not ok:
        m = max(n, 1)      # (an empty row marks word 0, so that the root of every row tells whether it is safe)
        lo[:m], hi[:m], fl[:m] = np.nan, np.nan, MAY_NAN | MALFORMED
    return lo, hi, fl


def forest_intervals(value, type_, size, lower, upper, lib="float32", widen=True):
    value, type_, size = np.asarray(value, np.float32), np.asarray(type_, np.int16), np.asarray(size, np.int16)
    lower, upper = np.asarray(lower, np.float32).reshape(-1), np.asarray(upper, np.float32).reshape(-1)
    pop, L = value.shape
    lo, hi, fl = np.zeros((pop, L), np.float32), np.zeros((pop, L), np.float32), np.zeros((pop, L), np.uint8)
    for t in range(pop):
        lo[t], hi[t], fl[t] = tree_intervals(value[t], type_[t], size[t], lower, upper, lib, widen)
    return lo, hi, fl


def safe(lo, hi, flags, max_abs=float("inf")):
    """rule 8 on the roots: (pop,) bool"""
    l0, h0 = lo[:, 0].astype(np.float64), hi[:, 0].astype(np.float64)
    with np.errstate(invalid="ignore"):
        return (flags[:, 0] == 0) & np.isfinite(l0) & np.isfinite(h0) & (np.maximum(np.abs(l0), np.abs(h0)) <= max_abs)


def obeys_claim(values, lo, hi, flags):
    """does every value (an array of float32 evaluations of one node) obey the claim for that node's (lo, hi, flags)?"""
    values = np.asarray(values, np.float32)
    nan = np.isnan(values)
    if nan.any() and not (int(flags) & MAY_NAN):
        return False
    v = values[~nan]
    return bool(np.all(v >= lo) and np.all(v <= hi))
