"""TEST-ONLY: a strict dimensional checker, independent of the restatement (tests/dimension_ref.py, which it must not import).  It knows
no free nodes: every constant comes with an explicit unit, and the question is only whether every operation of the tree is then
consistent.  A unit is a tuple of K plain ints, numerators over 25200; the universe is the in-range units (|n| <= 2^24), so a result
that leaves it -- a product out of range, the square root of an odd numerator, a power that is no integer numerator -- is no unit.

``check(value, type, size, var_units, const_units, label=None)`` -> the list of the units of the live nodes (tuples), or None when the
tree is inconsistent under ``const_units`` ({node index: unit}) or its root differs from ``label``."""
from fractions import Fraction

from sr_grad_ref import decode

DEN = 25200
LIM = 1 << 24

_SAME = {1, 2, 8, 9}                   # + - max min
_COMPARE = {10, 11, 12, 13}
_TRANSCENDENTAL = set(range(14, 23))   # sin .. exp


class Inconsistent(Exception):
    pass


def _unit(u):
    if any(abs(n) > LIM for n in u):
        raise Inconsistent
    return u


def prepare(value, type_, size, var_len):
    """the decoded live nodes of one tree: what ``check`` reads, for a caller that checks one tree under many assignments"""
    return [decode(type_[i], value[i], False, var_len, 1)[:2] + (int(type_[i]), float(value[i])) for i in range(int(size[0]))]


def check(value, type_, size, var_units, const_units, label=None, nodes=None):
    var_len = len(var_units)
    nodes = prepare(value, type_, size, var_len) if nodes is None else nodes
    n = len(nodes)
    K = len(var_units[0])
    one = (0,) * K
    out = [None] * n

    def go(i):
        """-> (unit of the subtree at i, the index past it)"""
        kind, f = nodes[i][:2]
        if kind == "C":
            out[i] = _unit(tuple(const_units[i]))
            return out[i], i + 1
        if kind == "V":
            out[i] = tuple(int(x) for x in var_units[f])
            return out[i], i + 1
        kids, at, c = [], [], i + 1
        for _ in range({"U": 1, "B": 2, "T": 3}[kind]):
            at.append(c)
            u, c = go(c)
            kids.append(u)
        if kind == "T":
            if kids[1] != kids[2]:
                raise Inconsistent
            r = kids[1]
        elif f is None:
            r = one
        elif kind == "U":
            a = kids[0]
            if f in _TRANSCENDENTAL:
                if a != one:
                    raise Inconsistent
                r = one
            elif f in (25, 26):        # neg abs
                r = a
            elif f in (23, 24):        # inv loose_inv
                r = tuple(-x for x in a)
            else:                      # sqrt loose_sqrt
                if any(x % 2 for x in a):
                    raise Inconsistent
                r = tuple(x // 2 for x in a)
        else:
            a, b = kids
            if f in _SAME or f in _COMPARE:
                if a != b:
                    raise Inconsistent
                r = a if f in _SAME else one
            elif f == 3:
                r = _unit(tuple(x + y for x, y in zip(a, b)))
            elif f in (4, 5):
                r = _unit(tuple(x - y for x, y in zip(a, b)))
            else:                      # pow loose_pow
                if b != one:
                    raise Inconsistent
                if a == one:
                    r = one
                else:
                    if nodes[at[1]][2] != 1:        # the exponent of a dimensional base must be a literal number
                        raise Inconsistent
                    cv = nodes[at[1]][3]
                    if cv != cv or cv in (float("inf"), float("-inf")):
                        raise Inconsistent
                    p = [Fraction(cv) * x for x in a]
                    if any(q.denominator != 1 for q in p):
                        raise Inconsistent
                    r = _unit(tuple(int(q) for q in p))
        out[i] = r
        return r, c

    try:
        root, _ = go(0)
    except Inconsistent:
        return None
    if label is not None and root != tuple(int(x) for x in label):
        return None
    return out
