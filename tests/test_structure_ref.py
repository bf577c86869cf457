"""CPU: the integer restatement of the structural pass (tests/structure_ref.py, the definition csrc/sr_structure.hip follows) held to an
independent checker that does not share its walk (tests/structure_exact.py: a recursive parse into nested tuples, every quantity from
its textbook statement), to the hand table (tests/structure_cases.py) and to the closed forms of a long chain.  All integer: every
comparison is an equality."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dimension_cases as DC  # noqa: E402
import interval_cases as IC  # noqa: E402
import sr_grad_ref as R  # noqa: E402
import structure_cases as SC  # noqa: E402
import structure_exact as SE  # noqa: E402
import structure_ref as SR  # noqa: E402

NAMES = ("complexity", "height", "depth", "nest", "flags")


def _held_to_exact(value, type_, size, p, what):
    """every row of the forest: the restatement's words are the exact checker's; returns the violations"""
    got = SR.forest_structure(value, type_, size, *p)
    cost, oplim, rules = SR.as_tables(*p[:5])
    assert [g.dtype for g in got] == [np.int32, np.int16, np.int16, np.uint8, np.uint8, np.int32]
    for t in range(value.shape[0]):
        want = SE.check_row(value[t], type_[t], size[t], cost, oplim, rules, p[5], p[6])
        if want is None:
            n = max(min(max(int(size[t, 0]), 0), value.shape[1]), 1)
            assert got[5][t] == -1 and (got[4][t, :n] == SR.MALFORMED).all() and not got[4][t, n:].any(), (what, t)
            assert not any(got[k][t].any() for k in range(4)), (what, t)
            continue
        for k, name in enumerate(NAMES):
            assert np.array_equal(got[k][t].astype(np.int64), want[name]), (what, t, name, got[k][t].tolist(), want[name].tolist())
        assert got[5][t] == want["violations"], (what, t)
    return got[5]


def test_random_trees_against_the_exact_checker(rng):
    """about 5000 random trees over all 29 functions, unknown ids among them, under random costs, 0 .. 8 random rules and random limits"""
    seen = np.zeros(0, np.int64)
    rules_seen = set()
    for block in range(50):
        value, type_, size = SC.random_forest(rng, 100, 64)
        p = SC.random_params(rng, tight=block % 2 == 0)
        rules_seen.add(len(p[2]))
        seen = np.concatenate([seen, _held_to_exact(value, type_, size, p, f"block {block}")])
    assert (seen == 0).sum() > 500 and (seen > 0).sum() > 500 and rules_seen >= {0, 8}


def test_paths_are_what_the_nesting_count_counts(rng):
    """the nesting count as a maximum over explicitly enumerated paths, on small trees"""
    value, type_, size = SC.random_forest(rng, 200, 32, max_depth=4)
    inner = SR.mask_word([R.F_SIN, R.F_ADD, SR.VAR, R.F_IF]) & 0xFFFFFFFF
    p = SC.params(rules=[([R.F_SIN], [R.F_SIN, R.F_ADD, SR.VAR, R.F_IF], 1)])
    nest = SR.forest_structure(value, type_, size, *p)[3]
    for t in range(200):
        for node in SE.nodes_of(SE.parse(value[t], type_[t], size[t])):
            best = max(sum((inner >> s) & 1 for s in path) for path in SE.paths_down(node))     # the node itself included
            assert nest[t, node[1], 0] == best, (t, node[1])


def test_hand_table():
    for c, value, type_, size in SC.table_rows():
        cx, ht, dp, nest, flags, viol = SR.forest_structure(value, type_, size, *c["params"])
        n = int(size[0, 0])
        assert viol[0] == c["viol"], (c["name"], int(viol[0]))
        assert flags[0, :n].tolist() == [c["flags"].get(i, 0) for i in range(n)], (c["name"], flags[0, :n].tolist())
        if c["cx"] is not None:
            assert cx[0, 0] == c["cx"], (c["name"], int(cx[0, 0]))
        if c["height"] is not None:
            assert ht[0, 0] == c["height"], (c["name"], int(ht[0, 0]))
        for i, want in c["nest"].items():
            assert nest[0, i].tolist() == want, (c["name"], i, nest[0, i].tolist())
        _held_to_exact(value, type_, size, c["params"], c["name"])
    causes = {f for c in SC.TABLE for f in c["flags"].values()}
    assert {1, 2, 3, 8, 16} <= causes      # each flag alone, NEST and OPERAND on one node


def test_depth_by_hand():
    value, type_, size = IC.rows([IC.IF(IC.V(0), IC.B(R.F_ADD, IC.V(0), IC.U(R.F_NEG, IC.V(1))), IC.C(1.0))], 12)
    cx, ht, dp, _, _, viol = SR.forest_structure(value, type_, size, *SC.params())
    assert dp[0].tolist() == [0, 1, 1, 2, 2, 3, 1] + [0] * 5 and ht[0].tolist() == [4, 1, 3, 1, 2, 1, 1] + [0] * 5
    assert cx[0].tolist() == [7, 1, 4, 1, 2, 1, 1] + [0] * 5 and viol[0] == 0


def test_unit_costs_give_the_subtree_size(rng):
    value, type_, size = SC.random_forest(rng, 300, 64)
    cx, _, _, _, flags, viol = SR.forest_structure(value, type_, size, *SC.params())
    live = np.arange(64)[None, :] < size[:, :1]
    assert (viol == 0).all() and np.array_equal(cx[live], size[live].astype(np.int32)) and not cx[~live].any() and not flags.any()


def test_malformed_rows():
    value, type_, size = DC.malformed_rows(8)
    p = SC.params(rules=[([R.F_ADD], [R.F_MUL], 0)], max_depth=2)
    cx, ht, dp, nest, flags, viol = SR.forest_structure(value, type_, size, *p)
    assert viol.tolist() == [2, -1, -1, -1, -1, 1]      # the good row: the product inside the sum, and three levels
    assert flags[0].tolist() == [9, 0, 0, 0, 0, 0, 0, 0] and flags[5, 0] == 8 and ht[5, 0] == 8 and dp[5].tolist() == list(range(8))
    assert flags[1].tolist() == [4] * 5 + [0] * 3 and flags[3].tolist() == [4] + [0] * 7 and flags[4].tolist() == [4] * 8
    for a in (cx, ht, dp, nest):
        assert not a[1:5].any()
    _held_to_exact(value, type_, size, p, "malformed rows")


def test_a_chain_of_1024_nodes():
    """sin(sin(.. sin(x) ..)), 1023 sines over a variable: nest saturates at 255, height is 1024 and depth reaches 1023"""
    value, type_, size = IC.rows([SC.unary_chain(1024)], 1024)
    p = SC.params(cost={R.F_SIN: 65535, SR.VAR: 65535}, rules=[([R.F_SIN], [R.F_SIN], 254), ([R.F_SIN], [R.F_SIN], 100), ([R.F_COS], [R.F_SIN], 0)],
                  max_depth=1023, max_complexity=65535 * 1024 - 1)
    cx, ht, dp, nest, flags, viol = SR.forest_structure(value, type_, size, *p)
    i = np.arange(1024)
    assert np.array_equal(ht[0], 1024 - i) and np.array_equal(dp[0], i) and np.array_equal(cx[0], 65535 * (1024 - i))
    assert cx[0, 0] == 65535 * 1024 and cx.dtype == np.int32
    want = np.minimum(255, 1023 - i)
    assert np.array_equal(nest[0, :, 0], want) and np.array_equal(nest[0, :, 1], want) and np.array_equal(nest[0, :, 2], want)
    # node i has 1022 - i sines strictly below it (saturated at 255): rule 0 fails where that exceeds 254, rule 1 where it exceeds 100
    below = np.minimum(255, np.maximum(1022 - i, 0))
    want_flags = np.where((below > 100) & (i < 1023), 1, 0)
    want_flags[0] |= 8 | 16
    assert np.array_equal(flags[0], want_flags) and viol[0] == int((below > 100).sum()) + 2
    assert (below > 254).sum() == 768 and (below > 100).sum() == 922
