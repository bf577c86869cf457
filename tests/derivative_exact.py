"""TEST-ONLY: exact evaluation of SR trees and of their forward-mode partial derivatives, the yardstick of tests/test_derivative_ref.py.

``Exact("fraction")`` computes with ``fractions.Fraction`` (the functions + - * / neg abs max min < > <= >= IF: every value and every
derivative is exact); ``Exact("mpmath")`` with mpmath at 256 bits (all 29 functions).  ``evaluate(value, type, size, x)`` returns one
``Node`` per live node of the row at the point ``x`` (a list of exact numbers):

  val    the real value of the subtree (None where it has none: a division by 0, log or sqrt of a negative number, ...), by the
         interpreters' rules where a real number leaves a choice (IF takes ``then`` where the condition is > 0; max / min / comparisons
         as interp.hpp writes them);
  der    d val / d x_v for every variable v (None where val is);
  alldef every node of the subtree has a defined real value (claim (a) speaks of such points only);
  kink   per variable: a node of the subtree sits on a point where it need not be differentiable in x_v -- abs, sqrt of 0, a max / min
         tie of operands whose derivatives differ, a comparison tie of two different expressions, an IF whose condition is 0, the seams
         of the loose functions and of pow at base 0 -- AND an operand that moves the seam is not locally constant in x_v (``lc``:
         constants, the other variables, functions of locally constant operands, and a comparison away from a tie whose operands have
         no kink, hence are continuous; where all are, the node is locally constant too and its derivative is 0 whatever the tie).

The mpmath evaluator gives up (alldef False, counted with the undefined points) where a magnitude leaves [2^-4096, 2^4096]: the tower
exp(exp(1e20)) has a finite real value that no evaluator can hold."""
from fractions import Fraction

import numpy as np

import sr_grad_ref as R
from sr_grad_ref import decode

DELTA = Fraction(float(np.float32(R.DELTA)))
MAXVAL = Fraction(float(np.float32(R.MAXVAL)))


class Node:
    __slots__ = ("val", "der", "alldef", "kink", "dep", "lc")

    def __init__(self, val, der, alldef, kink, dep, lc=None):
        self.val, self.der, self.alldef, self.kink, self.dep = val, der, alldef, kink, dep
        self.lc = [not d for d in dep] if lc is None else lc


class Exact:
    def __init__(self, mode, nvar):
        self.mode, self.nvar = mode, nvar
        if mode == "mpmath":
            import mpmath

            self.mp = mpmath.mp.clone()
            self.mp.prec = 256
            self.num = lambda c: self.mp.mpf(float(c)) if not isinstance(c, Fraction) else self.mp.mpf(c.numerator) / c.denominator
            self.big, self.tiny = self.mp.mpf(2) ** 4096, self.mp.mpf(2) ** -4096
        else:
            self.mp = None
            self.num = lambda c: c if isinstance(c, Fraction) else Fraction(float(c))
        self.zero, self.one = self.num(0), self.num(1)
        self.delta, self.maxval = self.num(DELTA), self.num(MAXVAL)

    def _undefined(self, kids):
        nv = self.nvar
        return Node(None, None, False, [any(k.kink[v] for k in kids) for v in range(nv)], [any(k.dep[v] for k in kids) for v in range(nv)])

    def _lib(self, f, a, da):
        """(val, [der]) of a library function at a defined operand, or None where it has no real value; seams are the caller's"""
        mp = self.mp
        if f == R.F_SIN:
            return mp.sin(a), mp.cos(a)
        if f == R.F_COS:
            return mp.cos(a), -mp.sin(a)
        if f == R.F_TAN:
            t = mp.tan(a)
            return t, 1 + t * t
        if f == R.F_SINH:
            return mp.sinh(a), mp.cosh(a)
        if f == R.F_COSH:
            return mp.cosh(a), mp.sinh(a)
        if f == R.F_TANH:
            t = mp.tanh(a)
            return t, 1 - t * t
        if f == R.F_EXP:
            e = mp.exp(a)
            return e, e
        raise AssertionError(f)

    def evaluate(self, value, type_, size, x):
        nv = self.nvar
        n = int(size[0])
        out = [None] * n
        zero, one = self.zero, self.one
        for i in reversed(range(n)):
            kind, pay, _ = decode(type_[i], value[i], False, nv, 1)
            if kind == "C":
                c = float(np.float32(pay))
                if c != c or c in (float("inf"), float("-inf")):
                    out[i] = Node(None, None, False, [False] * nv, [False] * nv)
                else:
                    out[i] = Node(self.num(c), [zero] * nv, True, [False] * nv, [False] * nv)
                continue
            if kind == "V":
                out[i] = Node(x[pay], [one if v == pay else zero for v in range(nv)], True, [False] * nv, [v == pay for v in range(nv)])
                continue
            kids, c = [], i + 1
            for _ in range({"U": 1, "B": 2, "T": 3}[kind]):
                kids.append(out[c])
                c += int(size[c])
            same = False
            if kind == "B":      # the two operands are the same expression, word for word
                c1, c2 = i + 1, i + 1 + int(size[i + 1])
                n1, n2 = int(size[c1]), int(size[c2])
                same = n1 == n2 and np.array_equal(type_[c1:c1 + n1], type_[c2:c2 + n2]) and np.array_equal(
                    np.asarray(value[c1:c1 + n1], np.float32).view(np.uint32), np.asarray(value[c2:c2 + n2], np.float32).view(np.uint32))
            out[i] = self._function(kind, pay, kids, same)
            nd = out[i]
            if self.mp is not None and nd.val is not None:
                mags = [abs(nd.val)] + [abs(d) for d in nd.der]
                if any(m > self.big or (m != 0 and m < self.tiny) for m in mags):
                    out[i] = self._undefined(kids)
        return out

    def _function(self, kind, f, kids, same=False):
        nv = self.nvar
        zero, one = self.zero, self.one
        alldef = all(k.alldef for k in kids)
        kink = [any(k.kink[v] for k in kids) for v in range(nv)]
        dep = [any(k.dep[v] for k in kids) for v in range(nv)]
        lc = [all(k.lc[v] for k in kids) for v in range(nv)]
        a = kids[0]

        def seam(who):
            """the node sits on a seam moved by the operands ``who``"""
            for v in range(nv):
                if not all(k.lc[v] for k in who):
                    kink[v] = True

        if kind == "T":
            b, c = kids[1], kids[2]
            if a.val is not None and a.val == 0:
                seam([a])
            take = b if (a.val is not None and a.val > 0) else c      # (a NaN condition takes ``else``, as NaN > 0 is false)
            if take.val is None:
                return self._undefined(kids)
            lc = [take.lc[v] and (a.lc[v] or (a.val is not None and a.val != 0 and not a.kink[v])) for v in range(nv)]
            return Node(take.val, take.der, alldef, kink, dep, lc)
        if f is None:
            return Node(zero, [zero] * nv, alldef, [False] * nv, [False] * nv)
        if any(k.val is None for k in kids):
            # the interpreters' NaN rules, for the VALUE only (alldef is False: claim (a) does not speak of such a point): a comparison
            # with a NaN is false, max / min whose first operand is a NaN yield the second
            if kind == "B" and R.F_LT <= f <= R.F_GE:
                return Node(-one, [zero] * nv, False, kink, dep, [False] * nv)
            if kind == "B" and f in (R.F_MAX, R.F_MIN) and kids[1].val is not None:
                return Node(kids[1].val, kids[1].der, False, kink, dep, [False] * nv)
            return self._undefined(kids)
        av, ad = a.val, a.der
        if kind == "U":
            if f == R.F_NEG:
                val, der = -av, [-d for d in ad]
            elif f == R.F_ABS:
                if av == 0:
                    seam([a])
                val, der = abs(av), [d if av >= 0 else -d for d in ad]
            elif f in (R.F_INV, R.F_LOOSE_INV):
                d = av
                if f == R.F_LOOSE_INV and abs(av) <= self.delta:
                    if av == 0 or abs(av) == self.delta:
                        seam([a])
                    d = self.delta if av >= 0 else -self.delta
                    val, der = 1 / d, [zero] * nv
                elif av == 0:
                    return self._undefined(kids)
                else:
                    val = 1 / d
                    der = [-x * val * val for x in ad]
            elif f in (R.F_SQRT, R.F_LOOSE_SQRT):
                if av < 0 and f == R.F_SQRT:
                    return self._undefined(kids)
                if av == 0:
                    seam([a])
                    val, der = zero, [zero] * nv
                else:
                    val = self.mp.sqrt(abs(av))
                    s = 1 if av > 0 else -1
                    der = [s * x / (2 * val) for x in ad]
            elif f in (R.F_LOG, R.F_LOOSE_LOG):
                if f == R.F_LOG and av <= 0:
                    return self._undefined(kids)
                if av == 0:
                    seam([a])
                    val, der = -self.maxval, [zero] * nv
                else:
                    val, der = self.mp.log(abs(av)), [x / av for x in ad]
            else:
                val, slope = self._lib(f, av, ad)
                der = [slope * x for x in ad]
            return Node(val, der, alldef, kink, dep, lc)
        b = kids[1]
        bv, bd = b.val, b.der
        if f == R.F_ADD:
            val, der = av + bv, [p + q for p, q in zip(ad, bd)]
        elif f == R.F_SUB:
            val, der = av - bv, [p - q for p, q in zip(ad, bd)]
        elif f == R.F_MUL:
            val, der = av * bv, [p * bv + av * q for p, q in zip(ad, bd)]
        elif f in (R.F_DIV, R.F_LOOSE_DIV):
            if f == R.F_LOOSE_DIV and abs(bv) <= self.delta:
                if bv == 0 or abs(bv) == self.delta:
                    seam([b])
                d = self.delta if bv >= 0 else -self.delta
                val, der = av / d, [p / d for p in ad]
            elif bv == 0:
                return self._undefined(kids)
            else:
                val = av / bv
                der = [(p - val * q) / bv for p, q in zip(ad, bd)]
        elif f in (R.F_MAX, R.F_MIN):
            if av == bv:         # a tie with equal derivatives is no kink: max(a, b) is differentiable there, with that derivative
                for v in range(nv):
                    if ad[v] != bd[v]:
                        kink[v] = True
            first = av >= bv if f == R.F_MAX else av <= bv
            val, der = (av, ad) if first else (bv, bd)
        elif R.F_LT <= f <= R.F_GE:
            if av == bv and not same:      # (x < x is a constant)
                seam([a, b])
            t = {R.F_LT: av < bv, R.F_GT: av > bv, R.F_LE: av <= bv, R.F_GE: av >= bv}[f]
            val, der = (one if t else -one), [zero] * nv
            lc = [lc[v] or same or (av != bv and not kink[v]) for v in range(nv)]
        elif f in (R.F_POW, R.F_LOOSE_POW):
            mp = self.mp
            if av == 0:
                seam([a, b])
                if f == R.F_LOOSE_POW and bv == 0:
                    val = zero
                elif bv > 0:
                    val = zero
                elif bv == 0:
                    val = one
                else:
                    return self._undefined(kids)
                der = [zero] * nv
            elif av > 0 or f == R.F_LOOSE_POW:
                val = mp.exp(bv * mp.log(abs(av)))
                der = [val * (q * mp.log(abs(av)) + bv * p / av) for p, q in zip(ad, bd)]
            elif bv == mp.floor(bv) and abs(bv) < 2 ** 20:
                seam([b])                                    # a negative base: defined on integer exponents only
                val = mp.power(av, int(bv))
                der = [bv * val / av * p for p in ad]
            else:
                return self._undefined(kids)
        else:
            raise AssertionError(f)
        return Node(val, der, alldef, kink, dep, lc)


def dyadic_points(rng, lower, upper, n):
    """n points of the box as lists of Fractions: every coordinate a multiple of 2^e, e chosen so that about a thousand of them lie in
    the coordinate's range (the point itself where the range is one point); float32-exact"""
    lower, upper = [Fraction(float(b)) for b in lower], [Fraction(float(b)) for b in upper]
    pts = []
    for _ in range(n):
        p = []
        for lo, hi in zip(lower, upper):
            if lo == hi:
                p.append(lo)
                continue
            w = hi - lo
            e = 0
            while Fraction(2) ** e > w:
                e -= 1
            while Fraction(2) ** (e + 1) <= w:
                e += 1
            s = Fraction(2) ** (e - 10)
            k_lo, k_hi = -((-lo) // s), hi // s
            p.append(int(rng.integers(int(k_lo), int(k_hi) + 1)) * s)
        pts.append(p)
    return pts


def as_fraction(x):
    return Fraction(float(x))


def exact_bounds(lo, hi, fraction):
    """the float32 bounds of one row as a list of (lo, hi) pairs of exact numbers (Fractions, or floats for mpmath to compare with),
    an infinite side as None, a NaN side as the string "nan" (nothing lies within it)"""
    def side(x):
        x = float(x)
        if x != x:
            return "nan"
        if x in (float("inf"), float("-inf")):
            return None
        return Fraction(x) if fraction else x
    return [(side(a), side(b)) for a, b in zip(lo, hi)]


def within(x, bound):
    lo, hi = bound
    if lo == "nan" or hi == "nan":
        return False
    return (lo is None or x >= lo) and (hi is None or x <= hi)
