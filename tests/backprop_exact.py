"""TEST-ONLY: semantic backpropagation in ``fractions.Fraction`` -- a tree evaluator and the inversion of DESIGN.md 3.24 over the
functions whose rules are rational (+ - * / neg inv max min abs IF), the yardstick of tests/test_backprop_ref.py.

A value is a Fraction, or None where the interpreter has a NaN (a division by 0).  ``evaluate(value, type, size, x, replace=None)``
returns the value of every node at the point ``x``; ``replace = (pos, v)`` puts the constant ``v`` in the place of the subtree at ``pos``
(the round trip of the test).  ``desired(value, type, size, x, y, pos)`` -> ``(d, state, status)`` for one row; with ``where=True`` a
fourth entry names the node at which the row left REQUIRED: the operand whose value a FREE row does not depend on (FREE says "any
value of THAT operand": below it a subtree may have no value to give, 1 / (v - v), and under a division "any" leaves out 0)."""
from fractions import Fraction

import sr_grad_ref as R
from backprop_ref import BLOCKED, FREE, IMPOSSIBLE, MALFORMED, OK, POSITION, RATIONAL, REQUIRED, children, path_to
from subtree_ref import live_len, well_formed


def _apply(kind, f, a):
    """the interpreters' rules (interp.hpp) on exact operands; a comparison with a NaN is false"""
    if kind == "T":
        return a[1] if a[0] is not None and a[0] > 0 else a[2]
    if kind == "U":
        x = a[0]
        if x is None:
            return None
        return {R.F_NEG: lambda: -x, R.F_ABS: lambda: abs(x), R.F_INV: lambda: None if x == 0 else 1 / x}[f]()
    x, y = a
    if f == R.F_MAX:
        return x if x is not None and y is not None and x >= y else y
    if f == R.F_MIN:
        return x if x is not None and y is not None and x <= y else y
    if x is None or y is None:
        return None
    if f == R.F_DIV:
        return None if y == 0 else x / y
    return {R.F_ADD: x + y, R.F_SUB: x - y, R.F_MUL: x * y}[f]


def evaluate(value, type_, size, x, replace=None):
    n = live_len(size, len(value))
    assert well_formed(type_, n)
    kids = children(type_, n)
    val = [None] * n
    for i in reversed(range(n)):
        if replace is not None and i == replace[0]:
            val[i] = replace[1]
            continue
        kind, f, _ = R.decode(type_[i], value[i], False, len(x), 1)
        if kind == "C":
            val[i] = Fraction(float(f))
        elif kind == "V":
            val[i] = Fraction(x[f])
        else:
            assert kind == "T" or f in RATIONAL, f"function {f} is not rational"
            val[i] = _apply(kind, f, [val[c] for c in kids[i]])
    return val


def desired(value, type_, size, x, y, pos, where=False):
    out = _desired(value, type_, size, x, y, pos)
    return out if where else out[:3]


def _desired(value, type_, size, x, y, pos):
    n = live_len(size, len(value))
    if not well_formed(type_, n):
        return None, IMPOSSIBLE, MALFORMED, None
    if not 0 <= pos < n:
        return None, IMPOSSIBLE, POSITION, None
    kids = children(type_, n)
    steps = path_to(kids, pos)
    nodes = [R.decode(type_[i], value[i], False, len(x), 1) for i, _ in steps]
    if any(kind == "T" and k == 0 for (kind, _, _), (_, k) in zip(nodes, steps)):
        return None, IMPOSSIBLE, BLOCKED, None
    val = evaluate(value, type_, size, x)
    t, state = Fraction(y), REQUIRED
    for (kind, f, _), (i, k) in zip(nodes, steps):
        s = val[kids[i][1 - k]] if kind == "B" else val[kids[i][0]]
        if t is None or (kind == "B" and s is None):
            return None, IMPOSSIBLE, OK, kids[i][k]
        if kind == "T":
            taken = s is not None and s > 0
            if taken != (k == 1):   # the tree returns the other branch
                other = val[kids[i][3 - k]]
                return None, (FREE if other is not None and other == t else IMPOSSIBLE), OK, kids[i][k]
        elif f == R.F_ADD:
            t = t - s
        elif f == R.F_SUB:
            t = t + s if k == 0 else s - t
        elif f == R.F_MUL:
            if s == 0:
                return None, (FREE if t == 0 else IMPOSSIBLE), OK, kids[i][k]
            t = t / s
        elif f == R.F_DIV and k == 0:
            if s == 0:
                return None, IMPOSSIBLE, OK, kids[i][k]
            t = t * s
        elif f == R.F_DIV:
            if t == 0 or s == 0:
                return None, (FREE if t == 0 and s == 0 else IMPOSSIBLE), OK, kids[i][k]
            t = s / t
        elif f == R.F_MAX:
            if not t >= s:
                return None, IMPOSSIBLE, OK, kids[i][k]
        elif f == R.F_MIN:
            if not t <= s:
                return None, IMPOSSIBLE, OK, kids[i][k]
        elif f == R.F_NEG:
            t = -t
        elif f == R.F_INV:
            if t == 0:
                return None, IMPOSSIBLE, OK, kids[i][k]
            t = 1 / t
        elif f == R.F_ABS:
            if t < 0:
                return None, IMPOSSIBLE, OK, kids[i][k]
            t = -t if s is not None and s < 0 else t
        else:
            raise AssertionError(f"function {f} is not rational")
    return t, state, OK, None
