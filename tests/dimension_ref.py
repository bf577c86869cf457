"""TEST-ONLY: the integer restatement of dimensional analysis over SR trees (csrc/sr_dims.hip) -- and its DEFINITION: the kernel follows
this file rule by rule, and since all arithmetic is integer it must give the same words.

``forest_dimensions(value, type, size, var_units, label_units, check_root)`` -> ``(units (pop, L, K) int32, flags (pop, L) uint8,
violations (pop,) int32)``.

UNITS.  K base dimensions, 1 <= K <= 8.  A unit is K int32 numerators over the fixed denominator DEN = 25200 = 2^4 3^2 5^2 7 (four nested
square roots and two cube roots of integer powers stay exact); a numerator is in range when |n| <= LIM = 2^24; all zeros is
"dimensionless".  ``var_units`` (var_len, K) and ``label_units`` (K,) hold in-range numerators (the caller checks).

LEAVES.  A variable carries its unit.  A CONST node is FREE: it may carry whatever unit makes the tree consistent.

THE CLAIM.  ``violations[t] == 0`` iff the constants of tree t can be given units such that every operation is dimensionally consistent
and (``check_root``) the root has ``label_units``; ``units`` then holds one such assignment (the unit of a CONST node is the unit of that
constant, the unit of any other node that of its subtree).  Soundness (violations == 0 => the assignment is consistent) holds always;
completeness holds for every tree without a pow / loose_pow over a free base, within the universe of in-range units.  (pow(c * x, 2)
with x in metres is called inconsistent under a label in square metres although a dimensionless c serves: pass 1 takes a pow over a
free base for dimensionless and so never asks what the base would have to be.)

PASS 1, from the last live node to node 0: every node gets (free?, unit); a free node's unit is 0 for now.  Operand order is
interp.hpp's: the first child is ``a`` (for IF: the condition), the second ``b``, the third ``c``.
  VAR v (index clamped as decode does)   fixed, var_units[v]
  CONST                                  free
  + - max min (a, b); IF's branches      both free: free.  One free: fixed, the other's unit.  Both fixed: fixed, a's unit;
                                         VIOLATION when the two units differ.  IF's condition may have any unit (it is compared with 0).
  < > <= >=                              fixed dimensionless; VIOLATION when both operands are fixed and their units differ
  * / loose_div                          either operand free: free.  Else fixed, the sum / difference; VIOLATION (unit 0) when a
                                         numerator of it leaves the range
  neg abs                                the child's (free?, unit)
  inv loose_inv                          the child's, negated
  sqrt loose_sqrt                        free child: free.  Else fixed, halved; VIOLATION (unit 0) when a numerator is odd
  sin cos tan sinh cosh tanh log loose_log exp
                                         fixed dimensionless; VIOLATION when the child is fixed and not dimensionless
  pow loose_pow (a, b)                   fixed dimensionless -- unless a is fixed with a non-zero unit and b is a CONST LEAF c: then
                                         fixed c * unit(a).  VIOLATION (unit 0) when b is fixed and not dimensionless; when a is fixed
                                         with a non-zero unit and b is no CONST leaf; when c * n is no in-range integer for a numerator
                                         n of a: the product is taken in float64 (exact: 24 x 25 bits) and must satisfy p == rint(p) and
                                         |p| <= LIM, which a NaN or an infinite c never does
  an unknown function id                 fixed dimensionless (the interpreters yield 0)
Every violating node counts 1.  THE ROOT: with ``check_root``, a fixed root whose unit differs from ``label_units`` counts 1 more and node
0 gets ROOT_MISMATCH.

PASS 2, from node 0 to the last live node, only for a tree whose count is still 0: every free node's unit becomes the one it is assigned.
A free root is assigned ``label_units`` (``check_root``) or 0.  A node with final unit D hands demands to its FREE children only:
  + - max min, IF's branches   D                         IF's condition   0
  < > <= >=                    the fixed sibling's unit, 0 when both are free
  a * b                        a free, b fixed: D - u(b);  b free, a fixed: D - u(a);  both free: a gets D, b gets 0
  a / b, loose_div             a free, b fixed: D + u(b);  b free, a fixed: u(a) - D;  both free: a gets D, b gets 0
  neg abs   D        inv loose_inv   -D        sqrt loose_sqrt   2 D
  the transcendentals, both operands of pow / loose_pow, the unknown ids   0
A demand with a numerator out of range becomes 0, marks that child VIOLATION and counts 1.

FLAGS per node: FREE 1 (the node was free in pass 1), VIOLATION 2, MALFORMED 4, ROOT_MISMATCH 8.

MALFORMED ROWS are judged by interval_ref.tree_intervals' rule (stack discipline plus verified size words): flags MALFORMED and unit 0 on
every live word (on word 0 when the row has none), violations = -1.  Words past the live prefix are 0."""
import numpy as np

from sr_grad_ref import (F_ABS, F_ADD, F_DIV, F_GE, F_INV, F_LOOSE_DIV, F_LOOSE_INV, F_LOOSE_POW, F_LOOSE_SQRT, F_LT, F_MAX, F_MIN, F_MUL,
                         F_NEG, F_POW, F_SQRT, F_SUB, T_CONST, decode)
from subtree_ref import live_len, well_formed

DEN = 25200
LIM = 1 << 24
FREE, VIOLATION, MALFORMED, ROOT_MISMATCH = 1, 2, 4, 8
ADDLIKE = (F_ADD, F_SUB, F_MAX, F_MIN)
PRODUCTS = (F_MUL, F_DIV, F_LOOSE_DIV)
POWERS = (F_POW, F_LOOSE_POW)


def in_range(u):
    return all(-LIM <= n <= LIM for n in u)


def addlike(a, b):
    """(free?, unit, violation) of a pair that must share a unit; a and b are (free?, unit)"""
    (fa, ua), (fb, ub) = a, b
    if fa and fb:
        return True, [0] * len(ua), False
    if fa:
        return False, list(ub), False
    if fb:
        return False, list(ua), False
    return False, list(ua), ua != ub


def unary(f, a):
    fa, ua = a
    zero = [0] * len(ua)
    if f is None:
        return False, zero, False
    if f in (F_NEG, F_ABS):
        return fa, list(ua), False
    if f in (F_INV, F_LOOSE_INV):
        return fa, [-n for n in ua], False
    if f in (F_SQRT, F_LOOSE_SQRT):
        if any(n & 1 for n in ua):
            return fa, zero, True
        return fa, [n >> 1 for n in ua], False
    return False, zero, (not fa) and any(ua)


def pow_unit(c, ua):
    """c * unit, or None when a product is no in-range integer (c: the float32 value of the CONST leaf)"""
    out = []
    with np.errstate(all="ignore"):
        for n in ua:
            p = np.float64(np.float32(c)) * np.float64(n)
            if not (p == np.rint(p) and abs(p) <= LIM):
                return None
            out.append(int(p))
    return out


def binary(f, a, b, b_const, c):
    (fa, ua), (fb, ub) = a, b
    zero = [0] * len(ua)
    if f is None:
        return False, zero, False
    if f in ADDLIKE:
        return addlike(a, b)
    if F_LT <= f <= F_GE:
        return False, zero, addlike(a, b)[2]
    if f in PRODUCTS:
        if fa or fb:
            return True, zero, False
        u = [x + y if f == F_MUL else x - y for x, y in zip(ua, ub)]
        return (False, u, False) if in_range(u) else (False, zero, True)
    assert f in POWERS, f
    based = (not fa) and any(ua)
    if ((not fb) and any(ub)) or (based and not b_const):
        return False, zero, True
    if based:
        u = pow_unit(c, ua)
        return (False, zero, True) if u is None else (False, u, False)
    return False, zero, False


def tree_dimensions(value, type_, size, var_units, label_units, check_root):
    """one row -> (units (L, K), flags (L,), violations)"""
    L = len(value)
    var_len, K = var_units.shape
    units, flags = np.zeros((L, K), np.int32), np.zeros(L, np.uint8)
    zero = [0] * K
    label = [int(n) for n in label_units]
    n = live_len(size, L)
    ok = well_formed(type_, n)
    count = 0
    nodes, kids = [None] * n, [None] * n
    if ok:
        free = [False] * n
        unit = [zero] * n
        for i in reversed(range(n)):
            kind, pay, _ = nodes[i] = decode(type_[i], value[i], False, var_len, 1)
            ks = []
            c = i + 1
            for _ in range({"C": 0, "V": 0, "U": 1, "B": 2, "T": 3}[kind]):
                ks.append(c)
                c += int(size[c])
            kids[i] = ks
            ops = [(free[k], unit[k]) for k in ks]
            if kind == "C":
                r = (True, zero, False)
            elif kind == "V":
                r = (False, [int(x) for x in var_units[pay]], False)
            elif kind == "U":
                r = unary(pay, ops[0])
            elif kind == "B":
                r = binary(pay, ops[0], ops[1], int(type_[ks[1]]) == T_CONST, value[ks[1]])
            else:
                r = addlike(ops[1], ops[2])
            if int(size[i]) != c - i:
                ok = False
                break
            free[i], unit[i] = r[0], list(r[1])
            units[i] = r[1]
            flags[i] = (FREE if r[0] else 0) | (VIOLATION if r[2] else 0)
            count += int(r[2])
    if not ok:
        m = max(n, 1)
        units[:], flags[:] = 0, 0
        flags[:m] = MALFORMED
        return units, flags, -1
    if check_root and not free[0] and unit[0] != label:
        flags[0] |= ROOT_MISMATCH
        count += 1
    if count:
        return units, flags, count

    # ---- pass 2 ----
    def demand(k, want):
        nonlocal count
        if not free[k]:
            return
        if not in_range(want):
            want = zero
            flags[k] |= VIOLATION
            count += 1
        unit[k] = list(want)
        units[k] = want

    if free[0]:
        unit[0] = list(label) if check_root else zero
        units[0] = unit[0]
    for i in range(n):
        kind, f, _ = nodes[i]
        ks, D = kids[i], unit[i]
        if kind == "U":
            s = 1 if f in (F_NEG, F_ABS) else -1 if f in (F_INV, F_LOOSE_INV) else 2 if f in (F_SQRT, F_LOOSE_SQRT) else 0
            demand(ks[0], [s * x for x in D])
        elif kind == "T":
            demand(ks[0], zero)
            demand(ks[1], D)
            demand(ks[2], D)
        elif kind == "B":
            a, b = ks
            if f in ADDLIKE:
                demand(a, D)
                demand(b, D)
            elif f is not None and F_LT <= f <= F_GE:
                ua, ub = (zero if free[a] else unit[a]), (zero if free[b] else unit[b])     # (read before either is assigned)
                demand(a, ub)
                demand(b, ua)
            elif f in PRODUCTS:
                sg = -1 if f == F_MUL else 1
                if free[a] and free[b]:
                    demand(a, D)
                    demand(b, zero)
                elif free[a]:
                    demand(a, [x + sg * y for x, y in zip(D, unit[b])])
                elif free[b]:
                    demand(b, [-sg * x + sg * y for x, y in zip(D, unit[a])])
            else:
                demand(a, zero)
                demand(b, zero)
    return units, flags, count


def forest_dimensions(value, type_, size, var_units, label_units=None, check_root=True):
    value, type_, size = np.asarray(value, np.float32), np.asarray(type_, np.int16), np.asarray(size, np.int16)
    var_units = np.asarray(var_units, np.int64)
    assert var_units.ndim == 2 and 1 <= var_units.shape[1] <= 8 and var_units.shape[0] >= 1
    K = var_units.shape[1]
    label_units = np.zeros(K, np.int64) if label_units is None else np.asarray(label_units, np.int64).reshape(K)
    pop, L = value.shape
    units, flags, viol = np.zeros((pop, L, K), np.int32), np.zeros((pop, L), np.uint8), np.zeros(pop, np.int32)
    for t in range(pop):
        units[t], flags[t], viol[t] = tree_dimensions(value[t], type_[t], size[t], var_units, label_units, bool(check_root))
    return units, flags, viol


def const_units(units, type_, size):
    """{node index: unit as a list} of the CONST nodes of one row's live prefix"""
    n = live_len(size, len(size))
    return {i: [int(x) for x in units[i]] for i in range(n) if int(type_[i]) == T_CONST}
