"""CPU: the midpoint rule of approximately geometric semantic crossover (tests/agx_ref.py restates it, csrc/sr_backprop.hip
with MID runs it).

The truth does not descend from the rule table: it is the ROUND TRIP of tests/test_backprop_ref.py in exact arithmetic
(tests/backprop_exact.py, which takes the target as an argument), with the target (a + b) / 2 of the recipient's and its mate's exact
values.  On every REQUIRED row the exact desired value, put in the subtree's place, makes the recipient return exactly (a + b) / 2 -- so
the offspring is equidistant from both parents there; on every FREE row the same holds for two different values of the operand at which
the row became FREE; a pair with a NaN parent on a row is IMPOSSIBLE there.  No tolerance, no excluded row.  Then the float64 restatement
against the exact one, and a hand-written table of the start state and of the order of the status codes."""
import os
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import agx_ref as AR  # noqa: E402
import backprop_exact as BX  # noqa: E402
import backprop_ref as BR  # noqa: E402
import sr_grad_ref as R  # noqa: E402
from interval_cases import B, C, U, V, rows  # noqa: E402
from test_backprop_ref import D, POP, _draw  # noqa: E402  (60 trees over BR.RATIONAL, L 24, 12 rows of small integers, seed 20261021)

nan, inf = np.float32(np.nan), np.float32(np.inf)
REQ, FREE, IMP = BR.REQUIRED, BR.FREE, BR.IMPOSSIBLE


def _mate_of(t):
    return (7 * t + 3) % POP


def _exact(forest, X, t, pos, r):
    """(a, b, mid, d, state, status, left_at) of recipient t at pos on row r in Fractions; a value is None where the interpreter has a NaN"""
    value, type_, size = forest
    m = _mate_of(t)
    x = [Fraction(float(v)) for v in X[r]]
    a = BX.evaluate(value[t], type_[t], size[t], x)[0]
    b = BX.evaluate(value[m], type_[m], size[m], x)[0]
    mid = None if a is None or b is None else (a + b) / 2
    d, state, status, left_at = BX.desired(value[t], type_[t], size[t], x, Fraction(0) if mid is None else mid, pos, where=True)
    if status == BR.OK and mid is None:
        d, state, left_at = None, IMP, None
    return x, a, b, mid, d, state, status, left_at


def test_round_trip_to_the_exact_midpoint():
    forest, X, _ = _draw()
    value, type_, size = forest
    seen = {REQ: 0, FREE: 0, IMP: 0}
    blocked = 0
    nan_mid = set()
    for t in range(POP):
        for pos in range(int(size[t, 0])):
            for r in range(D):
                x, a, b, mid, d, state, status, left_at = _exact(forest, X, t, pos, r)
                if status == BR.BLOCKED:
                    blocked += 1
                    continue
                assert status == BR.OK
                seen[state] += 1
                if mid is None:
                    nan_mid.add((t, r))
                    assert state == IMP, f"tree {t} pos {pos} row {r}: a NaN parent, but the state is {state}"
                elif state == REQ:
                    got = BX.evaluate(value[t], type_[t], size[t], x, replace=(pos, d))[0]
                    assert got == mid, f"tree {t} pos {pos} row {r}: the desired value {d} gives {got}, the midpoint is {mid}"
                    assert got - a == b - got   # equidistant from both parents
                elif state == FREE:
                    for v in (Fraction(3), Fraction(-7, 2)):
                        got = BX.evaluate(value[t], type_[t], size[t], x, replace=(left_at, v))[0]
                        assert got == mid, f"tree {t} pos {pos} row {r}: FREE, but the value {v} gives {got}, the midpoint is {mid}"
    print(f"rows by state {seen}, NaN-midpoint (pair, row) {len(nan_mid)}, blocked rows {blocked}")
    assert seen[REQ] >= 1000 and seen[FREE] >= 1 and seen[IMP] >= 1 and blocked >= 1 and len(nan_mid) >= 1, (seen, blocked, len(nan_mid))


def test_float64_restatement_agrees_with_the_exact_one():
    forest, X, _ = _draw()
    value, type_, size = forest
    mate = [_mate_of(t) for t in range(POP)]
    compared = 0
    for t in range(POP):
        for pos in range(int(size[t, 0])):
            d64, st64, status64 = AR.tree_desired_mid(value[t], type_[t], size[t], value, type_, size, X, pos, mate[t], np.float64)
            for r in range(D):
                _, _, _, _, d, state, status, _ = _exact(forest, X, t, pos, r)
                assert status == status64 and state == st64[r], f"tree {t} pos {pos} row {r}: {status, state} exact, {status64, st64[r]} float64"
                if status == BR.OK and state == REQ:
                    assert abs(d64[r] - float(d)) <= 1e-12 * abs(float(d)), f"tree {t} pos {pos} row {r}: {d64[r]!r} against {d}"
                    compared += 1
                else:
                    assert np.isnan(d64[r])
    assert compared > 1000


# ---- a hand table: the start state and the order of the status codes ----------------------------------------------------------------
X2 = np.array([[3.0, 0.0, -2.0], [1.0, 2.0, 4.0]], np.float32)   # two rows: x1 is 0 on the first only
GOOD = [V(0), B(R.F_DIV, V(0), V(1)), C(inf), C(-inf), C(3e38), B(R.F_ADD, V(0), V(2))]   # the mates; a seventh, malformed one is appended
SUM = B(R.F_ADD, V(0), V(2))      # 1 and 5 on the two rows
# (what, recipient, pos, mate) -> (desired per row or None, state per row, status)
TABLE = [
    ("mid at pos = 0", SUM, 0, 0, ([2.0, 3.0], [REQ, REQ], 0)),
    ("mid one step down", SUM, 1, 0, ([4.0, -1.0], [REQ, REQ], 0)),
    ("a pair of one tree with itself: its own predictions", SUM, 0, 5, ([1.0, 5.0], [REQ, REQ], 0)),
    ("an infinite mate, pos = 0", SUM, 0, 2, (None, [IMP, IMP], 0)),
    ("an infinite mate, below the root", SUM, 2, 2, (None, [IMP, IMP], 0)),
    ("an infinite recipient", C(inf), 0, 0, (None, [IMP, IMP], 0)),
    ("inf and -inf", C(inf), 0, 3, (None, [IMP, IMP], 0)),
    ("a NaN mate on one row only, pos = 0", SUM, 0, 1, ([None, 2.75], [IMP, REQ], 0)),
    ("a NaN mate on one row only, below the root", SUM, 2, 1, ([None, 1.75], [IMP, REQ], 0)),
    ("a NaN recipient on one row only", B(R.F_DIV, V(2), V(1)), 0, 0, ([None, 1.5], [IMP, REQ], 0)),
    ("mate index -1", SUM, 0, -1, (None, [IMP, IMP], 4)),
    ("mate index n_mates", SUM, 0, 7, (None, [IMP, IMP], 4)),
    ("a malformed mate", SUM, 0, 6, (None, [IMP, IMP], 4)),
    ("a bad position with a bad mate: 2 wins", SUM, 3, -1, (None, [IMP, IMP], 2)),
    ("a bad position with a malformed mate: 2 wins", SUM, -1, 6, (None, [IMP, IMP], 2)),
    ("a blocked path with a good mate", U(R.F_SIN, V(0)), 1, 0, (None, [IMP, IMP], 3)),
    ("a blocked path with a bad mate: 4 wins", U(R.F_SIN, V(0)), 1, 7, (None, [IMP, IMP], 4)),
    ("a blocked path with a malformed mate: 4 wins", U(R.F_SIN, V(0)), 1, 6, (None, [IMP, IMP], 4)),
]


def _mates():
    v, t, s = rows(GOOD + [B(R.F_ADD, V(0), V(2))], 16)
    s[6, 0] = 2   # x0 + <nothing>
    return v, t, s


def _check(what, dtype, got, want):
    d, st, status = got
    desired, state, want_status = want
    assert status == want_status and st.tolist() == state, f"{what} ({dtype.__name__}): state {st.tolist()}, status {status}"
    for r, s in enumerate(state):
        w = None if desired is None else desired[r]
        if w is None:
            assert np.isnan(d[r]), f"{what}: desired {d[r]!r} on row {r}"
        else:
            assert s == REQ and d[r] == dtype(w), f"{what} ({dtype.__name__}): desired {d[r]!r} on row {r}, expected {w!r}"


def test_the_start_state_and_the_order_of_the_status_codes():
    mv, mt, ms = _mates()
    for dtype in (np.float32, np.float64):
        for what, tree, pos, mate, want in TABLE:
            v, t, s = rows([tree], 16)
            _check(what, dtype, AR.tree_desired_mid(v[0], t[0], s[0], mv, mt, ms, X2, pos, mate, dtype), want)
        # a malformed recipient with a bad mate: 1 wins
        v, t, s = rows([SUM], 16)
        s[0, 0] = 2
        for mate in (-1, 6, 0):
            _check("a malformed recipient", dtype, AR.tree_desired_mid(v[0], t[0], s[0], mv, mt, ms, X2, 0, mate, dtype), (None, [IMP, IMP], 1))


def test_the_midpoint_does_not_overflow_where_the_sum_does():
    """0.5 * a + 0.5 * b, not 0.5 * (a + b): two values of 3e38 have a float32 midpoint, their float32 sum is inf"""
    mv, mt, ms = _mates()
    v, t, s = rows([C(3e38)], 16)
    d, st, status = AR.tree_desired_mid(v[0], t[0], s[0], mv, mt, ms, X2, 0, 4, np.float32)
    assert status == 0 and st.tolist() == [REQ, REQ] and (d == np.float32(3e38)).all()
    with np.errstate(over="ignore"):
        assert np.isinf(np.float32(3e38) + np.float32(3e38))
    assert AR.midpoint(np.float32(3.0), np.float32(4.0), np.float32) == np.float32(3.5)


def test_forest_form_and_match():
    mv, mt, ms = _mates()
    v, t, s = rows([SUM, SUM, U(R.F_SIN, V(0))], 16)
    d, st, status = AR.forest_desired_mid(v, t, s, mv, mt, ms, X2, [0, 2, 1], [0, 1, 9])
    assert status.tolist() == [0, 0, 4] and st.tolist() == [[REQ, REQ], [IMP, REQ], [IMP, IMP]] and d.dtype == np.float32
    best, dist, const, const_dist, counts = BR.match(d, st, status, np.array([[2.0, 3.0], [0.0, 1.75]], np.float32))
    assert best.tolist() == [0, 1, -1] and dist[0, 0] == 0.0 and dist[1, 1] == 0.0 and counts.tolist() == [[2, 0, 0], [1, 0, 1], [0, 0, 2]]
