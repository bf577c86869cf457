"""CPU: the claim behind the arithmetic line's Z rule (evogp_amd/csrc/sr_tc.hip, compile_pack_arith; tests/zero_or_nan_trees.py restates
it), held against the oracle: every tree the rule marks -- a NaN constant, or a division whose divisor is +-0 or NaN in every row -- has
a NaN fitness, whatever the data (finite columns, -0, +-inf and NaN in the columns and labels) under both error measures: NOT ONE marked
tree may have a finite fitness.  Also: the rule marks every tree the rule before it marked (tests/nan_trees.py), the share of the
headline forest its census gives, and the single cases it is meant for -- and leaves alone the ones it must."""
import numpy as np
import pytest

from helpers import c2_dataset, depth2leaf, roulette_uniform
from nan_trees import crafted_forest, poisoned, special_dataset
from zero_or_nan_trees import ROUNDS, proved_nan

V, C, U, B = 0, 1, 2, 3
ADD, SUB, MUL, DIV = 1, 2, 3, 4


@pytest.fixture(scope="module")
def headline(oracle):
    """the first 20 k trees of the headline forest (bench.py sr_inputs: keys [42, 0], six layers, + - * /, constants -1 0 1)"""
    return oracle.generate(20_000, 64, 10, 1, 0.5, 0.5, [42, 0], depth2leaf(6), roulette_uniform([1, 2, 3, 4]), [-1.0, 0.0, 1.0])


def _check(oracle, forest, X, y, what):
    pz = proved_nan(*forest)
    old = poisoned(*forest)
    missed = np.nonzero(old & ~pz)[0]
    assert len(missed) == 0, f"{what}: trees {missed[:5]} are marked by the NaN-constant rule but not by the Z rule"
    for mse in (True, False):
        fit = oracle.sr_fitness(*forest, X, y, mse)
        bad = np.nonzero(pz & ~np.isnan(fit))[0]
        assert len(bad) == 0, f"{what} mse={mse}: trees {bad[:5]} are marked NaN in every row but their fitness is {fit[bad[:5]]}"
    return pz, old


def test_headline_trees(oracle, headline):
    X, y = c2_dataset()
    pz, old = _check(oracle, headline, X, y, "headline")
    # the census of these 20 000 trees: 0.2731 marked by the NaN-constant rule; with the Z rule 0.3466 after two rounds, 0.3526 after
    # three (the rule as built), 0.3542 at the fixed point
    print(f"marked: {old.mean():.4f} by the NaN-constant rule, {pz.mean():.4f} by the Z rule ({ROUNDS} rounds)")
    assert 0.272 < old.mean() < 0.274
    assert ROUNDS == 3 and abs(pz.mean() - 0.3526) < 0.0005, f"{pz.mean():.4f} of the headline trees marked, the census says 0.3526"
    for r, share in ((2, 0.3466), (8, 0.3542)):
        got = proved_nan(*headline, rounds=r).mean()
        assert abs(got - share) < 0.0005, f"{r} rounds mark {got:.4f}, the census says {share}"


def test_headline_trees_on_special_data(oracle, headline):
    X, y = special_dataset(300, 10, 7)
    _check(oracle, headline, X, y, "headline, special data")


@pytest.mark.parametrize("D", [1, 8, 100, 600])
def test_crafted_trees(oracle, D):
    """the crafted forest joined with generated trees over constants -1 0 1 inf nan"""
    cv, ct, cs = crafted_forest()
    hv, ht, hs = oracle.generate(3000, 64, 6, 1, 0.5, 0.5, [100, 3], depth2leaf(6), roulette_uniform([1, 2, 3, 4]), [-1.0, 0.0, 1.0, np.inf, np.nan])
    forest = tuple(np.concatenate(p) for p in ((cv, hv), (ct, ht), (cs, hs)))
    X, y = special_dataset(D, 6, D)
    pz, old = _check(oracle, forest, X, y, f"crafted D={D}")
    assert 100 < pz[:len(cv)].sum() < len(cv) - 100, "the crafted forest must hold marked and unmarked trees"
    assert pz.sum() > old.sum(), "the Z rule must find trees the NaN-constant rule does not"


def _forest(trees):
    v = np.zeros((len(trees), 64), np.float32); t = np.zeros((len(trees), 64), np.int16); s = np.zeros((len(trees), 64), np.int16)
    for i, nodes in enumerate(trees):
        for j, (ty, val, sz) in enumerate(nodes):
            t[i, j], v[i, j], s[i, j] = ty, val, sz
    return v, t, s


def _sized(tree):
    """nested tuples (op, left, right) / ('v', i) / ('c', x) / ('nofn', operand) -> prefix nodes with subtree sizes"""
    if tree[0] == "v":
        return [(V, tree[1], 1)]
    if tree[0] == "c":
        return [(C, tree[1], 1)]
    if tree[0] == "nofn":
        a = _sized(tree[1])
        return [(U, 29, 1 + len(a))] + a
    a, b = _sized(tree[1]), _sized(tree[2])
    return [(B, tree[0], 1 + len(a) + len(b))] + a + b


x, y_, z = ("v", 0), ("v", 1), ("v", 2)
c0, cm0, c1 = ("c", 0.0), ("c", -0.0), ("c", 1.0)


def _nested(rounds_needed):
    """x / (... ((y - y) * x) * x ...): the divisor enters Z after `rounds_needed` rounds (y - y itself needs none)"""
    d = (SUB, y_, y_)
    for _ in range(rounds_needed):
        d = (MUL, d, x)
    return (DIV, x, d)


MARKED = {
    "x / (y * 0)": (DIV, x, (MUL, y_, c0)),
    "x / (0 * y)": (DIV, x, (MUL, c0, y_)),
    "x / (y - y)": (DIV, x, (SUB, y_, y_)),
    "x / (0 / y)": (DIV, x, (DIV, c0, y_)),
    "x / ((y * 0) + (0 * z))": (DIV, x, (ADD, (MUL, y_, c0), (MUL, c0, z))),
    "x / ((1 - 1) * y)": (DIV, x, (MUL, (SUB, c1, c1), y_)),
    "x / (-0 * y)": (DIV, x, (MUL, cm0, y_)),
    "x / ((y * 0) - (z - z))": (DIV, x, (SUB, (MUL, y_, c0), (SUB, z, z))),
    "x / (((1 - 1) * (1 + 1)) * y)": (DIV, x, (MUL, (MUL, (SUB, c1, c1), (ADD, c1, c1)), y_)),   # a second-round constant 0
    "z + (x / (y * 0))": (ADD, z, (DIV, x, (MUL, y_, c0))),
    f"nested, {ROUNDS} rounds": _nested(ROUNDS),
}
UNMARKED = {
    "x / (y - z)": (DIV, x, (SUB, y_, z)),
    "x / (y + 0)": (DIV, x, (ADD, y_, c0)),
    "x / ((y * 0) + 1)": (DIV, x, (ADD, (MUL, y_, c0), c1)),
    "x * (y * 0)": (MUL, x, (MUL, y_, c0)),
    "(y - y) / x": (DIV, (SUB, y_, y_), x),
    "x / ((y / y) - 1)": (DIV, x, (SUB, (DIV, y_, y_), c1)),
    "x / (y + y)": (DIV, x, (ADD, y_, y_)),
    "(0 / y) / x": (DIV, (DIV, c0, y_), x),
    f"nested, {ROUNDS + 1} rounds (NaN, but more rounds than the rule runs)": _nested(ROUNDS + 1),
}


def test_rule_cases():
    """single cases of the rule: what it marks and what it leaves alone"""
    for name, tree in MARKED.items():
        assert proved_nan(*_forest([_sized(tree)]))[0], f"{name} must be marked"
    for name, tree in UNMARKED.items():
        assert not proved_nan(*_forest([_sized(tree)]))[0], f"{name} must not be marked"
    for name, tree in MARKED.items():   # behind "no function" (which drops its operand): not this line's rule
        assert not proved_nan(*_forest([_sized(("nofn", tree))]))[0], f"{name} behind a 'no function' node must not be marked"
        assert not proved_nan(*_forest([_sized((ADD, x, ("nofn", tree)))]))[0], f"x + nofn({name}) must not be marked"


@pytest.mark.parametrize("D", [1, 8, 100])
def test_rule_cases_against_the_oracle(oracle, D):
    """the marked cases are NaN by the oracle on data with -0, +-inf and NaN in it; those of the unmarked ones that are not NaN in truth
    (all but the one that needs more rounds, and x / ((y / y) - 1)) have a finite fitness on finite data"""
    forest = _forest([_sized(t) for t in list(MARKED.values()) + list(UNMARKED.values())])
    X, y = special_dataset(D, 6, D)
    _check(oracle, forest, X, y, f"cases D={D}")
    r = np.random.default_rng(D)
    Xf = r.uniform(1, 3, (D, 6)).astype(np.float32); yf = r.uniform(-3, 3, (D, 1)).astype(np.float32)
    fit = oracle.sr_fitness(*forest, Xf, yf, True)
    names = list(MARKED) + list(UNMARKED)
    for i, name in enumerate(names):
        if name in MARKED or "more rounds than" in name or name == "x / ((y / y) - 1)":
            assert np.isnan(fit[i]), f"{name}: {fit[i]}"
        else:
            assert np.isfinite(fit[i]), f"{name}: {fit[i]} on finite, positive data"
