"""CPU: the claim behind the arithmetic line's NAN_TREE programs (evogp_amd/csrc/sr_tc.hip, compile_pack_arith), held against the
oracle: every tree the compiler's rule marks (tests/nan_trees.py restates it) has a NaN fitness, whatever the data -- finite columns,
-0, +-inf and NaN in the columns and labels -- under both error measures.  Also: the rule marks what the census of the headline
forest says it should (about one tree in four), and never a tree whose fitness is a number."""
import numpy as np
import pytest

from helpers import c2_dataset, depth2leaf, roulette_uniform
from nan_trees import crafted_forest, poisoned, special_dataset


@pytest.fixture(scope="module")
def headline(oracle):
    """the first 20 k trees of the headline forest (bench.py sr_inputs: keys [42, 0], six layers, + - * /, constants -1 0 1)"""
    return oracle.generate(20_000, 64, 10, 1, 0.5, 0.5, [42, 0], depth2leaf(6), roulette_uniform([1, 2, 3, 4]), [-1.0, 0.0, 1.0])


def _check(oracle, forest, X, y, what):
    pz = poisoned(*forest)
    for mse in (True, False):
        fit = oracle.sr_fitness(*forest, X, y, mse)
        bad = np.nonzero(pz & ~np.isnan(fit))[0]
        assert len(bad) == 0, f"{what} mse={mse}: trees {bad[:5]} are marked NaN-poisoned but their fitness is {fit[bad[:5]]}"
    return pz


def test_headline_trees(oracle, headline):
    X, y = c2_dataset()
    pz = _check(oracle, headline, X, y, "headline")
    share = pz.mean()
    assert 0.23 < share < 0.32, f"{share:.3f} of the headline trees marked (23.4 % hold a literal x / 0; divisors that fold to 0 add more)"


def test_headline_trees_on_special_data(oracle, headline):
    X, y = special_dataset(300, 10, 7)
    _check(oracle, headline, X, y, "headline, special data")


@pytest.mark.parametrize("D", [1, 8, 100])
def test_crafted_trees(oracle, D):
    forest = crafted_forest()
    X, y = special_dataset(D, 6, D)
    pz = _check(oracle, forest, X, y, f"crafted D={D}")
    assert 100 < pz.sum() < len(pz) - 100, "the crafted forest must hold marked and unmarked trees"


def test_rule_cases():
    """single cases of the rule: what it marks and what it leaves alone"""
    V, C, B = 0, 1, 3

    def one(*nodes):
        v = np.zeros((1, 64), np.float32); t = np.zeros((1, 64), np.int16); s = np.zeros((1, 64), np.int16)
        for j, (ty, val, sz) in enumerate(nodes):
            t[0, j], v[0, j], s[0, j] = ty, val, sz
        return bool(poisoned(v, t, s)[0])

    assert one((B, 4, 3), (V, 0, 1), (C, 0.0, 1))                       # x / 0
    assert one((B, 4, 3), (V, 0, 1), (C, -0.0, 1))                      # x / -0
    assert not one((B, 4, 3), (C, 0.0, 1), (V, 0, 1))                   # 0 / x: a number where x is one
    assert one((B, 4, 5), (V, 0, 1), (B, 2, 3), (C, 1.0, 1), (C, 1.0, 1))   # x / (1 - 1)
    assert one((B, 1, 3), (V, 0, 1), (C, np.nan, 1))                    # x + NaN
    assert one((B, 1, 5), (V, 0, 1), (B, 2, 3), (C, np.inf, 1), (C, np.inf, 1))   # x + (inf - inf)
    assert not one((B, 1, 3), (V, 0, 1), (C, np.inf, 1))                # x + inf: NaN only where x is -inf
    assert not one((B, 3, 3), (V, 0, 1), (C, 0.0, 1))                   # x * 0: NaN only where x is not finite
    assert not one((B, 4, 3), (V, 0, 1), (V, 1, 1))                     # x / y: data-dependent
    assert one((C, np.nan, 1))
    assert not one((2, 29, 2), (B, 4, 3), (V, 0, 1), (C, 0.0, 1))      # behind "no function": not this line's rule
