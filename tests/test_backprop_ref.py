"""CPU: the inversion rule of semantic backpropagation (tests/backprop_ref.py restates it, csrc/sr_backprop.hip runs it).

The truth does not descend from the rule table: it is a ROUND TRIP in exact arithmetic (tests/backprop_exact.py).  For every tree over
the rational functions, every position and every row of small integer data the exact desired value is put in the place of the subtree
and the tree is evaluated again: on a REQUIRED row the result IS the label, on a FREE row it is the label for two different values of
the operand at which the row became FREE (below that operand a subtree may have no value to hand up: 1 / (v - v)).  No tolerance, no
excluded row.  Then the float64 restatement against the exact one, a hand-written table with one case per branch of the
rule, and the EXP / LOG rules against float64 log and exp of the target."""
import os
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import backprop_exact as BX  # noqa: E402
import backprop_ref as BR  # noqa: E402
import sr_grad_ref as R  # noqa: E402
from grad_trees import random_forest  # noqa: E402
from interval_cases import B, C, IF, U, V, rows  # noqa: E402

L, POP, D, NVAR = 24, 60, 12, 3
nan, inf = np.float32(np.nan), np.float32(np.inf)


def _draw():
    rng = np.random.default_rng(20261021)
    forest = random_forest(rng, POP, L, BR.RATIONAL, NVAR, 1, max_depth=4, const_range=(-2, 2))
    consts = forest[1] == R.T_CONST
    forest[0][consts] = np.round(forest[0][consts])          # small integer constants: zeros among them
    X = rng.integers(-2, 3, (D, NVAR)).astype(np.float32)
    y = rng.integers(-2, 3, D).astype(np.float32)
    y[:3] = 0
    return forest, X, y


def test_round_trip_in_exact_arithmetic():
    (value, type_, size), X, y = _draw()
    seen = {BR.REQUIRED: 0, BR.FREE: 0, BR.IMPOSSIBLE: 0}
    blocked = 0
    for t in range(POP):
        n = int(size[t, 0])
        for pos in range(n):
            for r in range(D):
                x = [Fraction(float(v)) for v in X[r]]
                d, state, status, left_at = BX.desired(value[t], type_[t], size[t], x, Fraction(float(y[r])), pos, where=True)
                if status == BR.BLOCKED:
                    blocked += r == 0
                    continue
                assert status == BR.OK
                seen[state] += 1
                label = Fraction(float(y[r]))
                if state == BR.REQUIRED:
                    got = BX.evaluate(value[t], type_[t], size[t], x, replace=(pos, d))[0]
                    assert got == label, f"tree {t} pos {pos} row {r}: the desired value {d} gives {got}, the label is {label}"
                elif state == BR.FREE:
                    for v in (Fraction(3), Fraction(-7, 2)):
                        got = BX.evaluate(value[t], type_[t], size[t], x, replace=(left_at, v))[0]
                        assert got == label, f"tree {t} pos {pos} row {r}: FREE, but the value {v} gives {got}, the label is {label}"
    assert all(seen.values()) and blocked, f"the draw misses a state or a blocked tree: {seen}, blocked {blocked}"
    print(f"rows by state {seen}, blocked (tree, position) pairs {blocked}")


def test_float64_restatement_agrees_with_the_exact_one():
    (value, type_, size), X, y = _draw()
    compared = 0
    for t in range(POP):
        for pos in range(int(size[t, 0])):
            d64, st64, status64 = BR.tree_desired(value[t], type_[t], size[t], X, y, pos, np.float64)
            for r in range(D):
                x = [Fraction(float(v)) for v in X[r]]
                d, state, status = BX.desired(value[t], type_[t], size[t], x, Fraction(float(y[r])), pos)
                assert status == status64 and state == st64[r], f"tree {t} pos {pos} row {r}: {status, state} exact, {status64, st64[r]} float64"
                if status == BR.OK and state == BR.REQUIRED:
                    assert abs(d64[r] - float(d)) <= 1e-12 * abs(float(d)), f"tree {t} pos {pos} row {r}: {d64[r]!r} against {d}"
                    compared += 1
                else:
                    assert np.isnan(d64[r])
    assert compared > 1000


def _one(expr, pos, x, y, dtype=np.float32, L_=16, size0=None):
    v, t, s = rows([expr], L_)
    if size0 is not None:
        s[0, 0] = size0
    X = np.array([x], np.float32)
    d, st, status = BR.tree_desired(v[0], t[0], s[0], X, np.array([y], np.float32), pos, dtype)
    return d[0], int(st[0]), status


REQ, FREE, IMP = BR.REQUIRED, BR.FREE, BR.IMPOSSIBLE
X0 = [3.0, 0.0, -2.0]   # x0 = 3, x1 = 0, x2 = -2
# (what, tree, pos, label) -> (desired or None, state, status)
TABLE = [
    ("ADD", B(R.F_ADD, V(0), V(2)), 1, 5.0, (7.0, REQ, 0)),
    ("SUB k=0", B(R.F_SUB, V(2), V(0)), 1, 5.0, (8.0, REQ, 0)),
    ("SUB k=1", B(R.F_SUB, V(0), V(2)), 2, 5.0, (-2.0, REQ, 0)),
    ("MUL", B(R.F_MUL, V(2), V(0)), 2, 5.0, (-2.5, REQ, 0)),
    ("MUL s == 0, t == 0", B(R.F_MUL, V(1), V(0)), 2, 0.0, (None, FREE, 0)),
    ("MUL s == 0, t != 0", B(R.F_MUL, V(1), V(0)), 2, 1.0, (None, IMP, 0)),
    ("DIV k=0", B(R.F_DIV, V(1), V(2)), 1, 5.0, (-10.0, REQ, 0)),
    ("DIV k=0, s == 0", B(R.F_DIV, V(0), V(1)), 1, 5.0, (None, IMP, 0)),
    ("DIV k=1", B(R.F_DIV, V(0), V(1)), 2, 6.0, (0.5, REQ, 0)),
    ("DIV k=1, t == 0, s == 0", B(R.F_DIV, V(1), V(0)), 2, 0.0, (None, FREE, 0)),
    ("DIV k=1, t == 0, s != 0", B(R.F_DIV, V(0), V(1)), 2, 0.0, (None, IMP, 0)),
    ("DIV k=1, t != 0, s == 0", B(R.F_DIV, V(1), V(0)), 2, 2.0, (None, IMP, 0)),
    ("MAX t > s", B(R.F_MAX, V(1), V(2)), 1, 5.0, (5.0, REQ, 0)),
    ("MAX t == s", B(R.F_MAX, V(1), V(0)), 1, 3.0, (3.0, REQ, 0)),
    ("MAX t < s", B(R.F_MAX, V(1), V(0)), 1, 2.0, (None, IMP, 0)),
    ("MIN t < s", B(R.F_MIN, V(0), V(1)), 2, -1.0, (-1.0, REQ, 0)),
    ("MIN t > s", B(R.F_MIN, V(0), V(1)), 2, 4.0, (None, IMP, 0)),
    ("NEG", U(R.F_NEG, V(0)), 1, 5.0, (-5.0, REQ, 0)),
    ("INV", U(R.F_INV, V(0)), 1, 4.0, (0.25, REQ, 0)),
    ("INV t == 0", U(R.F_INV, V(0)), 1, 0.0, (None, IMP, 0)),
    ("SQRT", U(R.F_SQRT, V(0)), 1, 3.0, (9.0, REQ, 0)),
    ("SQRT t < 0", U(R.F_SQRT, V(0)), 1, -1.0, (None, IMP, 0)),
    ("ABS, a positive child", U(R.F_ABS, V(0)), 1, 5.0, (5.0, REQ, 0)),
    ("ABS, a negative child", U(R.F_ABS, V(2)), 1, 5.0, (-5.0, REQ, 0)),
    ("ABS t < 0", U(R.F_ABS, V(2)), 1, -5.0, (None, IMP, 0)),
    ("ABS, a NaN child", U(R.F_ABS, C(nan)), 1, 5.0, (5.0, REQ, 0)),
    ("EXP t <= 0", U(R.F_EXP, V(0)), 1, 0.0, (None, IMP, 0)),
    ("IF k=0", IF(V(0), V(1), V(2)), 1, 5.0, (None, IMP, 3)),
    ("IF k=1 taken", IF(V(0), V(1), V(2)), 2, 5.0, (5.0, REQ, 0)),
    ("IF k=1 not taken, the other branch is the label", IF(V(2), V(1), V(0)), 2, 3.0, (None, FREE, 0)),
    ("IF k=1 not taken, the other branch is not", IF(V(2), V(1), V(0)), 2, 5.0, (None, IMP, 0)),
    ("IF k=2 taken", IF(V(1), V(0), V(2)), 3, 5.0, (5.0, REQ, 0)),
    ("IF k=2 not taken, the other branch is the label", IF(V(0), V(1), V(2)), 3, 0.0, (None, FREE, 0)),
    ("IF k=2 not taken, the other branch is not", IF(V(0), V(1), V(2)), 3, 5.0, (None, IMP, 0)),
    ("IF not taken, a NaN in the other branch", IF(V(0), C(nan), V(2)), 3, 5.0, (None, IMP, 0)),
    ("IF, a NaN condition is not > 0", IF(C(nan), V(1), V(2)), 3, 5.0, (5.0, REQ, 0)),
    ("a NaN sibling", B(R.F_ADD, C(nan), V(0)), 2, 5.0, (None, IMP, 0)),
    ("a NaN label below the root", U(R.F_NEG, V(0)), 1, nan, (None, IMP, 0)),
    ("float32 alone: overflow to inf", B(R.F_MUL, V(0), C(1e-30)), 1, 1e30, (None, IMP, 0)),
    ("an infinite sibling", B(R.F_ADD, C(inf), V(0)), 2, 5.0, (None, IMP, 0)),
    ("FREE is absorbing", B(R.F_MUL, V(1), B(R.F_ADD, V(0), V(2))), 3, 0.0, (None, FREE, 0)),
    ("IMPOSSIBLE is absorbing", B(R.F_MUL, V(1), B(R.F_ADD, V(0), V(2))), 3, 1.0, (None, IMP, 0)),
    ("two steps", B(R.F_MUL, V(2), B(R.F_ADD, V(0), V(1))), 4, 5.0, (-5.5, REQ, 0)),
    ("pos == 0", B(R.F_ADD, V(0), V(2)), 0, 5.0, (5.0, REQ, 0)),
    ("pos == 0, a NaN label is REQUIRED as it is", V(0), 0, nan, (None, REQ, 0)),
    ("pos at the last leaf", B(R.F_ADD, V(0), B(R.F_MUL, V(2), V(0))), 4, 5.0, (-1.0, REQ, 0)),
    ("pos == len", B(R.F_ADD, V(0), V(2)), 3, 5.0, (None, IMP, 2)),
    ("pos < 0", B(R.F_ADD, V(0), V(2)), -1, 5.0, (None, IMP, 2)),
    ("sin is blocked", U(R.F_SIN, V(0)), 1, 0.5, (None, IMP, 3)),
    ("pow is blocked", B(R.F_POW, V(0), V(2)), 1, 0.5, (None, IMP, 3)),
    ("a comparison is blocked", B(R.F_LT, V(0), V(2)), 2, 1.0, (None, IMP, 3)),
    ("the loose division is blocked", B(R.F_LOOSE_DIV, V(0), V(2)), 1, 1.0, (None, IMP, 3)),
    ("blocked above, a rule below", B(R.F_POW, B(R.F_ADD, V(0), V(1)), V(2)), 2, 0.5, (None, IMP, 3)),
]


def test_one_case_per_branch_of_the_rule():
    for dtype in (np.float32, np.float64):
        for what, tree, pos, label, (want, state, status) in TABLE:
            if what.startswith("float32 alone") and dtype is np.float64:
                continue
            d, st, stat = _one(tree, pos, X0, label, dtype)
            assert (st, stat) == (state, status), f"{what} ({dtype.__name__}): state {st}, status {stat}"
            if want is None:
                assert np.isnan(d), f"{what}: desired {d!r}"
            else:
                assert d == dtype(want) and np.signbit(d) == np.signbit(dtype(want)), f"{what} ({dtype.__name__}): desired {d!r}, expected {want!r}"


def test_a_malformed_row():
    d, st, status = _one(B(R.F_ADD, V(0), V(2)), 1, X0, 5.0, size0=2)   # x0 + <nothing>
    assert np.isnan(d) and (st, status) == (IMP, 1)
    d, st, status = _one(B(R.F_ADD, V(0), V(2)), 0, X0, 5.0, size0=0)
    assert np.isnan(d) and (st, status) == (IMP, 1)


def test_exp_and_log_rules_are_the_float64_functions_of_the_target():
    rng = np.random.default_rng(7)
    t = np.concatenate([rng.uniform(1e-3, 50.0, 200), [1.0, 1e-30, 3e38]]).astype(np.float32)
    v, ty, s = rows([U(R.F_EXP, V(0)), U(R.F_LOG, V(0))], 8)
    X = np.ones((len(t), 1), np.float32)
    for dtype, tol in ((np.float32, 2.0 ** -24), (np.float64, 2.0 ** -52)):
        d, st, status = BR.tree_desired(v[0], ty[0], s[0], X, t, 1, dtype)
        assert status == 0 and (st == REQ).all()
        want = np.log(t.astype(np.float64))
        assert (np.abs(d - want) <= tol * np.abs(want) + 1e-45).all()   # exp(x) = t  <=>  x = log t
        d, st, status = BR.tree_desired(v[1], ty[1], s[1], X, t, 1, dtype)
        with np.errstate(over="ignore"):
            want = np.exp(t.astype(np.float64))
        fits = want <= float(np.finfo(dtype).max)
        assert status == 0 and ((st == REQ) == fits).all() and (st[~fits] == IMP).all()
        assert (np.abs(d[fits] - want[fits]) <= tol * want[fits]).all()   # log(x) = t  <=>  x = exp t


def test_match_of_the_restatement():
    desired = np.array([[1.0, 2.0, np.nan, 4.0], [np.nan] * 4, [5.0, np.nan, np.nan, np.nan]])
    state = np.array([[0, 0, 1, 0], [2, 2, 2, 2], [0, 2, 1, 1]], np.uint8)
    status = np.array([0, 3, 0], np.int32)
    lib = np.array([[1.0, 2.0, 9.0, 5.0], [1.0, 2.0, np.inf, 4.0], [np.inf, 0.0, 0.0, 0.0], [1.0, 2.0, 7.0, 4.0]])
    best, dist, const, const_dist, counts = BR.match(desired, state, status, lib)
    assert best.tolist() == [1, -1, 0] and dist[0].tolist() == [1.0, 0.0, np.inf, 0.0] and not dist[1].any()
    assert dist[2].tolist() == [16.0, 16.0, np.inf, 16.0]
    assert const[0] == 7 / 3 and np.isnan(const[1]) and const[2] == 5.0 and const_dist[2] == 0.0
    assert abs(const_dist[0] - (1 + 4 + 16 - 49 / 3)) < 1e-12 and counts.tolist() == [[3, 1, 0], [0, 0, 4], [1, 2, 1]]
