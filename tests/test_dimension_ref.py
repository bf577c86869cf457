"""CPU: the restatement of dimensional analysis (tests/dimension_ref.py, the definition the kernel csrc/sr_dims.hip follows) against an
independent strict checker (tests/dimension_exact.py) -- soundness on every tree it calls consistent, completeness by brute force on
the trees it calls inconsistent -- and against a hand table with one row per rule and per cause of a violation."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dimension_cases as DC  # noqa: E402
import dimension_exact as DX  # noqa: E402
import dimension_ref as DR  # noqa: E402
import sr_grad_ref as R  # noqa: E402

N_TREES = 5000
# the 7 x 7 grid of exponents a constant is tried with, as numerators
GRID = [tuple(int(e * DC.DEN) for e in pair) for pair in itertools.product([-2, -1, -0.5, 0, 0.5, 1, 2], repeat=2)]


def _pow_over_free_base(type_, value, size, flags):
    """does the tree hold a pow / loose_pow whose first operand was free in pass 1?"""
    n = int(size[0])
    return any(int(type_[i]) == R.T_BFUNC and int(value[i]) in (R.F_POW, R.F_LOOSE_POW) and flags[i + 1] & DR.FREE for i in range(n - 1))


@pytest.fixture(scope="module")
def census():
    """N_TREES random trees (depth <= 3, all operator classes, K = 2, x0 m, x1 s, x2 m/s, x3 1, the label drawn from none, m, m/s^2, 1):
    every one judged by the restatement, then held against the strict checker"""
    rng = np.random.default_rng(20261019)
    var_units = np.array(DC.VARS, np.int64)
    out = dict(consistent=0, unsound=[], brute=0, incomplete=[], pow_gap=0, many_consts=0, malformed=0)
    for t in range(N_TREES):
        expr = DC.random_expr(rng)
        label = DC.LABELS[int(rng.integers(len(DC.LABELS)))]
        value, type_, size = (a[0] for a in DC.rows([expr], 40))
        units, flags, viol = DR.tree_dimensions(value, type_, size, var_units, np.array(label or (0, 0)), label is not None)
        consts = sorted(i for i in range(int(size[0])) if int(type_[i]) == R.T_CONST)
        if viol < 0:
            out["malformed"] += 1
        elif viol == 0:
            out["consistent"] += 1
            got = DX.check(value, type_, size, DC.VARS, DR.const_units(units, type_, size), label)
            if got is None or [tuple(int(x) for x in units[i]) for i in range(int(size[0]))] != got:
                out["unsound"].append((t, expr, label))
        elif len(consts) > 2:
            out["many_consts"] += 1
        else:
            out["brute"] += 1
            nodes = DX.prepare(value, type_, size, len(DC.VARS))
            for pick in itertools.product(GRID, repeat=len(consts)):
                if DX.check(value, type_, size, DC.VARS, dict(zip(consts, pick)), label, nodes) is not None:
                    if _pow_over_free_base(type_, value, size, flags):
                        out["pow_gap"] += 1      # the documented incompleteness, counted apart
                    else:
                        out["incomplete"].append((t, expr, label, pick))
                    break
    return out


def test_soundness(census):
    """every tree with violations == 0 passes the strict checker under the constant units of pass 2, node by node; at least 20 % of the
    trees are such (the prototype of the rule set: 37 %)"""
    print(f"consistent {census['consistent']} of {N_TREES}")
    assert census["malformed"] == 0
    assert census["consistent"] >= 0.2 * N_TREES
    assert not census["unsound"], census["unsound"][:3]


def test_completeness(census):
    """for every tree with violations > 0 and at most 2 constants no assignment from the 7 x 7 grid passes the strict checker -- but where
    the tree holds a pow / loose_pow over a free base (the documented gap), counted apart: at most 5 % of the brute-forced trees
    (prototype: 0.03 %); at least 20 % of all trees are brute-forced (prototype: 56 %)"""
    print(f"brute-forced {census['brute']}, assignment found behind a pow over a free base {census['pow_gap']}, more than 2 constants {census['many_consts']}")
    assert census["brute"] >= 0.2 * N_TREES
    assert census["pow_gap"] <= 0.05 * census["brute"]
    assert not census["incomplete"], census["incomplete"][:3]


def test_the_gap_is_real():
    """the documented incompleteness: pow(c * x0, 2) under the label m^2 is called inconsistent although a dimensionless c serves"""
    c = next(c for c in DC.TABLE if c["name"].startswith("the gap"))
    value, type_, size = (a[0] for a in DC.rows([c["expr"]], 8))
    assert DR.tree_dimensions(value, type_, size, np.array(DC.VARS), np.array(c["label"]), True)[2] == 1
    assert DX.check(value, type_, size, DC.VARS, {2: DC.ONE, 4: DC.ONE}, c["label"]) is not None


@pytest.mark.parametrize("k", range(len(DC.TABLE)), ids=[c["name"] for c in DC.TABLE])
def test_hand_table(k):
    c, value, type_, size, var_units, label, check_root = DC.table_rows()[k]
    units, flags, viol = DR.forest_dimensions(value, type_, size, var_units, label, check_root)
    n = int(size[0, 0])
    assert viol[0] == c["viol"], (viol[0], units[0, :n].tolist(), flags[0, :n].tolist())
    if c["root"] is not None:
        assert tuple(units[0, 0]) == tuple(c["root"])
    for i, u in c["consts"].items():
        assert tuple(units[0, i]) == tuple(u), (i, units[0, :n].tolist())
    for i, f in c["flags"].items():
        assert flags[0, i] == f, (i, flags[0, :n].tolist())
    assert not units[0, n:].any() and not flags[0, n:].any()
    if c["viol"] == 0:    # the strict checker agrees with every consistent row of the table
        got = DX.check(value[0], type_[0], size[0], [tuple(int(x) for x in u) for u in var_units], DR.const_units(units[0], type_[0], size[0]),
                       tuple(label) if check_root else None)
        assert got == [tuple(int(x) for x in units[0, i]) for i in range(n)]


def test_malformed_rows():
    """a bad size word, a stack underflow, an empty row, a length beyond the row: flags 4 and unit 0 on every live word (word 0 of the
    empty row), violations -1; a full row (n == L) is judged like any other and has no dead word"""
    L = 8
    value, type_, size = DC.malformed_rows(L)
    units, flags, viol = DR.forest_dimensions(value, type_, size, np.array(DC.VARS), np.array(DC.M), True)
    assert viol.tolist() == [0, -1, -1, -1, -1, 0]
    assert flags[1].tolist() == [4] * 5 + [0] * 3 and flags[2].tolist() == [4] * 5 + [0] * 3
    assert flags[3].tolist() == [4] + [0] * 7 and flags[4].tolist() == [4] * 8
    assert not units[1:5].any()
    assert (units[5] == np.array(DC.M)).all() and not flags[5].any()
    assert units[0, :5].tolist() == [list(DC.M), list(DC.M), list(DC.M), [0, 0], list(DC.M)] and flags[0].tolist() == [0, 1, 0, 1, 0, 0, 0, 0]


def test_every_k_and_no_input_is_written(rng):
    for K in (1, 3, 8):
        value, type_, size = DC.random_dim_forest(rng, 40, 32, 5)
        var_units, label = DC.random_units(rng, 5, K), DC.random_units(rng, 1, K)[0]
        keep = [a.copy() for a in (value, type_, size, var_units, label)]
        units, flags, viol = DR.forest_dimensions(value, type_, size, var_units, label, True)
        assert units.shape == (40, 32, K) and units.dtype == np.int32 and flags.dtype == np.uint8 and viol.dtype == np.int32
        for a, b in zip(keep, (value, type_, size, var_units, label)):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
        assert (viol == 0).any() and (viol > 0).any()
