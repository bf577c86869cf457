"""CPU: whole-tree evaluation held to a truth that is not ours -- the value of the reference's own `Tree.to_sympy_expr` under mpmath at 50
digits (tests/golden/sympy_truth_*.npz, written by tests/golden/make_sympy_truth.py).  The oracle's evaluate / batch_evaluate / sr_fitness
meet, entry by entry, 1e-5 |T| + 2 B with B the running float32 error bound of tests/exact_eval_ref.py; that helper's own values agree with
the truth to 1e-12.  This is the proof that the fixture and the bounds are sound before a GPU sees them (tests/test_gpu_sympy_truth.py).

The conditions on the fixture keep a test from hiding a failure: the share of entries compared per group, the share whose grant is the 1e-5
bar itself, the functions covered, the trees left out at export."""
import numpy as np
import pytest

import exact_eval_ref as ex


@pytest.fixture(scope="module", params=ex.GROUPS)
def grp(request):
    return ex.group(request.param)


def test_the_fixture_compares_enough(grp):
    """The floors are taken over the entries that are evidence: the trees that have a truth (the ones left out at export are capped on their
    own, from the header) and, in a multi-output tree, the outputs that at least one OUT node writes -- an output nobody writes is 0 on both
    sides, compared exactly, and counts for nothing here."""
    g = grp
    left = g.header["left_out"]
    assert left["export_failed"] == int((~g.exported).sum()) and left["export_failed"] <= 0.1 * left["considered"], left
    assert g.exported[g.hand].all() and g.compared[g.hand].all(), "a hand-written operand-order / branch row is not fully compared"
    assert len(np.unique(g.X, axis=0)) == 100
    assert (g.forest[2][~g.hand, 0] >= 3).all(), "a drawn tree is a lone leaf"
    if g.out_len > 1:
        assert (g.written[~g.hand].sum(1) >= 2).all(), "a drawn multi-output tree writes fewer than two outputs"
    share, tight = g.shares()
    assert share >= ex.FLOORS[g.name], f"{g.name}: {share:.3f} of the entries are compared"
    assert tight >= 0.9, f"{g.name}: the grant is the 1e-5 bar itself (at most twice it) for only {tight:.1%} of the compared entries"
    live = g.compared & g.counted
    assert (g.T[live] != 0).mean() >= 0.9, f"{g.name}: the compared entries are mostly zeros"
    for D in (8, 100, 600):
        for mse in (True, False):
            assert g.fitness_truth(g.rows(D)[1], mse)[2].mean() >= 0.4


def test_every_function_of_the_truth_is_covered():
    census = {}
    for name in ex.GROUPS:
        for f, n in ex.function_census(ex.group(name)).items():
            census[f] = census.get(f, 0) + n
    few = {ex.NAMES[f]: census.get(f, 0) for f in ex.TRUTH_FUNCS if census.get(f, 0) < 10}
    assert not few, f"functions in fewer than 10 trees with half their rows compared: {few}"
    assert sum(len(ex.group(name).exported) for name in ex.GROUPS) >= 400


@pytest.mark.parametrize("name", ["wide_pos", "wide_signed"])
def test_if_rows_take_both_branches(name):
    """every `if` node of the hand-written rows, the nested ones too, sees a condition of either sign on rows where the node's value is
    the one that reaches the root: each branch of each `if` is the tree's value somewhere"""
    g = ex.group(name)
    value, type_, size = g.forest
    seen = 0

    def walk(k, i, active):
        nonlocal seen
        t = int(type_[k, i]) & 0x7F
        kids, j = [], i + 1
        for _ in range(t - 1 if t >= 2 else 0):
            kids.append(j); j += int(size[k, j])
        if t == 4:
            cond = ex.evaluate(value[k:k + 1, kids[0]:], type_[k:k + 1, kids[0]:], size[k:k + 1, kids[0]:], g.X, 1)[0][0, :, 0]
            assert (active & (cond > 0)).any() and (active & (cond < 0)).any(), f"{name}: tree {k} node {i}: one branch is never the value"
            seen += 1
            walk(k, kids[0], active); walk(k, kids[1], active & (cond > 0)); walk(k, kids[2], active & ~(cond > 0))
        else:
            for c in kids:
                walk(k, c, active)

    for k in np.flatnonzero(g.hand):
        walk(k, 0, np.ones(len(g.X), bool))
    assert seen == 7   # two plain rows, a row with an `if` in either branch (3 nodes), a row with an `if` as the condition (2)


def test_the_float64_helper_agrees_with_the_truth(grp):
    """1e-12 relative on every regular entry that carries digits (B <= 1e-3 |T|: the compared ones).  The helper rounds each operation
    to 2^-64 where B counts 2^-24, so its own error is below 2^-40 B < 1e-10 B (a hundred times what that ratio gives); for the few regular
    entries next to a pole, whose B is many times |T|, that is the bound, and nothing else is granted.  One formula for both: the larger
    of the two, which is 1e-12 |T| wherever B <= 1e-2 |T|."""
    g = grp
    with np.errstate(all="ignore"):
        ok = np.abs(g.V - g.T) <= np.maximum(1e-12 * np.abs(g.T), 1e-10 * g.B)
    bad = np.argwhere(g.regular & ~ok)
    assert len(bad) == 0, f"{g.name}: tree {bad[0][0]} row {bad[0][1]}: {g.V[tuple(bad[0])]!r} against {g.T[tuple(bad[0])]!r}; {len(bad)} regular entries off"
    assert (1e-10 * g.B[g.compared] <= 1e-12 * np.abs(g.T[g.compared])).all()


@pytest.mark.parametrize("D", [8, 100, 600])
def test_oracle_evaluation_meets_the_truth(grp, oracle, D):
    g = grp
    X, idx = g.rows(D)
    ex.assert_entries(oracle.batch_evaluate(*g.forest, X, g.out_len), g, idx, f"{g.name} batch_evaluate D={D}")
    forest, rows = ex.copies(g, idx)
    ex.assert_entries(oracle.evaluate(*forest, rows, g.out_len), g, idx, f"{g.name} evaluate D={D}")


@pytest.mark.parametrize("D", [8, 100, 600])
@pytest.mark.parametrize("mse", [True, False], ids=["mse", "mae"])
def test_oracle_fitness_meets_the_truth(grp, oracle, D, mse):
    g = grp
    X, idx = g.rows(D)
    ex.assert_fitness(oracle.sr_fitness(*g.forest, X, g.labels(idx), mse), g, idx, mse, f"{g.name} sr_fitness D={D} {'mse' if mse else 'mae'}")
