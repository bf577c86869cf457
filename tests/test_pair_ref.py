"""CPU: the numpy restatement of the pairwise semantic moments (tests/pair_ref.py) held to hand-computed plants on the CPU oracle's
predictions, the exact (Fraction) sums against the long-double ones, the rule of the unusable tree, the four criteria and the arg-min
rule on hand values, and the condition on the inputs of every GPU case (tests/pair_cases.py SHAPES), checked here where no GPU is needed."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_cases as PC  # noqa: E402
import pair_ref as PR  # noqa: E402
import semantic_ref as S  # noqa: E402
import sr_grad_ref as R  # noqa: E402
from interval_cases import B, C, U, V, rows  # noqa: E402
from oracle.pyoracle import Oracle  # noqa: E402

oracle = Oracle("port")
D = 24


def _data():
    """small integers without zeros: every sum and product below is exact in float32"""
    rng = np.random.default_rng(11)
    return rng.choice(np.setdiff1d(np.arange(-8, 9), [0]), (D, 3)).astype(np.float32)


def _predict(exprs, X, width=16):
    f = rows(exprs, width)
    with np.errstate(all="ignore"):
        P, formed = S.oracle_predictions(oracle, *f, X)
    return P, PR.usable(P, formed)


TREE = B(R.F_ADD, B(R.F_MUL, V(0), V(1)), V(2))   # T = x0 x1 + x2


def _all(first, cand, P, u, y, exact=True):
    return PR.pair_moments(P, u, P, u, y, np.array(first), np.array(cand), exact=exact)


def test_a_tree_against_itself():
    X = _data()
    P, u = _predict([TREE, V(0)], X)
    y = (X[:, 0] - 1).astype(np.float32)
    own, mom, _, _ = _all([0, 1], [[0], [1]], P, u, y)
    for e in range(2):
        saa = float(sum((Fraction(float(p)) - Fraction(float(q))) ** 2 for p, q in zip(P[e], y)))
        assert own[e] == saa and mom[e, 0].tolist() == [saa, saa, 0.0]
    assert own[1] == D, "x0 - (x0 - 1) = 1 on every row"


def test_a_tree_against_its_negation_without_labels():
    X = _data()
    P, u = _predict([TREE, U(R.F_NEG, TREE)], X)
    own, mom, _, mag = _all([0], [[1]], P, u, None)
    saa = float((P[0].astype(np.float64) ** 2).sum())   # integers: exact
    assert own[0] == saa and mom[0, 0].tolist() == [saa, -saa, 4 * saa] and mag[0, 0].tolist() == [saa, saa, 4 * saa]


def test_t_plus_one_against_t_minus_one_has_a_midpoint_error_of_zero():
    X = _data()
    P, u = _predict([B(R.F_ADD, TREE, C(1.0)), B(R.F_SUB, TREE, C(1.0)), TREE], X)
    y = P[2].copy()
    own, mom, _, _ = _all([0], [[1]], P, u, y)
    assert own[0] == D and mom[0, 0].tolist() == [D, -D, 4 * D]
    for exact in (True, False):
        own, mom, _, _ = _all([0], [[1, 0, 2]], P, u, y, exact=exact)
        s = PR.scores("midpoint", own, mom)
        assert s[0].tolist() == [0.0, D, D / 4] and PR.choose(s, np.array([[1, 0, 2]]))[0].tolist() == [1]


def test_the_unusable_tree():
    X = _data()
    exprs = [TREE, B(R.F_DIV, V(0), C(0.0)), B(R.F_MUL, V(0), C(3e38)), V(1), V(2)]
    f = rows(exprs, 16)
    f[2][4, 0] = 0   # malformed
    with np.errstate(all="ignore"):
        P, formed = S.oracle_predictions(oracle, *f, X)
    u = PR.usable(P, formed)
    assert u.tolist() == [True, False, False, True, False], "NaN everywhere, inf somewhere, malformed"
    first = [0, 1, 0, 4, 5, -1, 3]
    cand = [[0, 3], [0, 3], [1, 3], [0, 0], [0, 0], [0, 0], [2, 7]]
    own, mom, own_mag, mag = _all(first, cand, P, u, X[:, 0].copy())
    assert np.isnan(own).tolist() == [False, True, False, True, True, True, False]
    assert np.isnan(mom[..., 0]).tolist() == [[False, False], [True, True], [True, False], [True, True], [True, True], [True, True], [True, True]]
    assert (np.isnan(mom) == np.isnan(mom[..., :1])).all() and (np.isnan(mag) == np.isnan(mom)).all() and (np.isnan(own_mag) == np.isnan(own)).all()


def test_exact_and_long_double_sums_agree_within_the_bound():
    rng = np.random.default_rng(3)
    for D_ in (1, 7, 65):
        P = (rng.normal(0, 1, (6, D_)) * 10.0 ** rng.integers(-3, 4, (6, 1))).astype(np.float32)
        y = rng.normal(0, 1, D_).astype(np.float32)
        u = np.ones(6, bool)
        first, cand = rng.integers(0, 6, 9), rng.integers(0, 6, (9, 3))
        a = PR.pair_moments(P, u, P, u, y, first, cand, exact=True)
        b = PR.pair_moments(P, u, P, u, y, first, cand, exact=False)
        assert (np.abs(a[0] - b[0]) <= PR.bound(D_, a[2])).all() and (np.abs(a[1] - b[1]) <= PR.bound(D_, a[3])).all()
        assert (a[3][..., 1] >= np.abs(a[1][..., 1])).all() and np.array_equal(a[3][..., [0, 2]], a[1][..., [0, 2]])
        swap = PR.pair_moments(P, u, P, u, y, cand[:, 0], first[:, None], exact=True)
        assert np.array_equal(swap[1][:, 0, 1:], a[1][:, 0, 1:]) and np.array_equal(swap[0], a[1][:, 0, 0]), "Sab, Sdd are symmetric; Sbb is the other's own"


def test_the_criteria_on_hand_values():
    nan, inf = np.nan, np.inf
    own = np.array([4.0, 4.0, 0.0, nan])
    #               Sbb  Sab  Sdd
    mom = np.array([[[4.0, -4.0, 16.0], [1.0, 2.0, 1.0], [4.0, 4.0, 0.0], [nan, nan, nan]],     # the opposite, a better one behind, itself, unusable
                    [[16.0, 0.0, 20.0], [0.0, 0.0, 4.0], [9.0, 6.0, 1.0], [1.0, -2.0, 9.0]],
                    [[1.0, 0.0, 1.0], [0.0, 0.0, 0.0], [4.0, 0.0, 4.0], [nan, nan, nan]],
                    [[1.0, 1.0, 1.0]] * 4])
    s = PR.scores("midpoint", own, mom)
    assert s[0].tolist() == [0.0, 2.25, 4.0, inf] and s[1].tolist() == [5.0, 1.0, 6.25, 0.25] and s[3].tolist() == [inf] * 4
    s = PR.scores("blend", own, mom)
    # row 0: alpha = clamp((4 + 4) / 16) = 0.5 -> 1 - 2 + 1 = 0; alpha = clamp(-1) = 0 -> Sbb = 1; Sdd = 0 -> alpha 0 -> Sbb = 4
    assert s[0].tolist() == [0.0, 1.0, 4.0, inf]
    # row 1: alpha = 16/20 -> 0.64 * 4 + 0 + 0.04 * 16 = 3.2; alpha = 0 -> 0; alpha = clamp(3) = 1 -> Saa = 4; alpha = 3/9 -> 4/9 - 8/9 + 4/9 = 0
    assert np.allclose(s[1], [3.2, 0.0, 4.0, 0.0], rtol=0, atol=1e-15)
    s = PR.scores("angle", own, mom)
    assert s[0].tolist() == [-1.0, 1.0, 1.0, inf] and s[1].tolist() == [0.0, 1.0, 1.0, -1.0] and s[2].tolist() == [1.0, 1.0, 1.0, inf]
    s = PR.scores("competent", own, mom)
    assert s[0].tolist() == [0.5, 2.0, inf, inf] and s[2].tolist() == [2.0, inf, 3.0, inf]
    with pytest.raises(ValueError):
        PR.scores("nearest", own, mom)


def test_ties_go_to_the_lowest_slot_and_all_inf_takes_slot_zero():
    inf = np.inf
    score = np.array([[2.0, 1.0, 1.0], [inf, inf, inf], [inf, 3.0, 3.0], [0.0, -0.0, 0.0]])
    cand = np.array([[7, 8, 9]] * 4)
    right, best, slot = PR.choose(score, cand)
    assert slot.tolist() == [1, 0, 1, 0] and right.tolist() == [8, 7, 8, 7] and best.tolist() == [1.0, inf, 3.0, 0.0]


@pytest.mark.parametrize("shape", PC.SHAPES, ids=PC.shape_id)
def test_the_gpu_cases_meet_the_condition_on_the_inputs(shape):
    """on the CPU oracle's predictions (the device's may differ in the last bits of a transcendental function; the test on the device
    asserts the same condition on its own)"""
    funcs, gp_len, pop, E, M, D_, var_len, labels = shape
    f = PC.pair_forest(funcs, gp_len, pop, var_len)
    X, y = PC.pair_data(D_, var_len)
    first, cand = PC.case_events(shape)
    with np.errstate(all="ignore"):
        P, formed = S.oracle_predictions(oracle, *f, X)
    u = PR.usable(P, formed)
    if pop >= 63:
        assert not formed[list(PC.MALFORMED)].any() and formed[[PC.DEEP_ROW, PC.NAN_ROW, PC.INF_LAST_ROW]].all()
        assert not u[PC.NAN_ROW] and not u[PC.INF_LAST_ROW] and np.isfinite(P[PC.INF_LAST_ROW, :-1]).all() and u[PC.DEEP_ROW] and u[PC.T_ROW]
    assert u[0]
    own, mom, _, _ = PR.pair_moments(P, u, P, u, y if labels else None, first, cand)
    PC.check_condition(shape, mom)
