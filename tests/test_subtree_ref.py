"""CPU: the numpy restatement of the per-subtree pass and of the rewrite rule (tests/subtree_ref.py) -- the yardstick of the GPU tests.
Its node_err agrees with the C oracle's sr_fitness of every subtree extracted into a row of its own; the rewrite rule yields
well-formed prefix trees with consistent sizes, lets the outermost foldable node win, breaks ties in error by size and then by index,
and is idempotent."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sr_grad_ref as R  # noqa: E402
import subtree_ref as S  # noqa: E402
from grad_trees import ALL_FUNCS, ARITH, random_forest  # noqa: E402
from helpers import per_tree_tolerance  # noqa: E402

NAN = np.float32(np.nan)


@pytest.mark.parametrize("use_mse", [True, False])
@pytest.mark.parametrize("funcs", ["arith", "all"])
def test_node_err_matches_oracle_on_extracted_subtrees(rng, oracle, funcs, use_mse):
    value, type_, size = random_forest(rng, 16, 64, ARITH if funcs == "arith" else ALL_FUNCS, 3, 1, max_depth=5)
    X = rng.uniform(0.5, 1.5, (70, 3)).astype(np.float32)
    y = rng.uniform(-1, 1, (70, 1)).astype(np.float32)
    size[5, 0] = 0   # malformed
    err, const = S.forest_subtree_errors(value, type_, size, X, y, use_mse)
    assert np.isnan(err[5]).all() and np.isnan(const[5]).all()
    compared = live = 0
    for t in range(16):
        if t == 5:
            continue
        n = int(size[t, 0])
        assert np.isnan(err[t, n:]).all() and np.isnan(const[t, n:]).all()
        sub = S.extract_subtrees(value, type_, size, t)
        want, tol, unstable = per_tree_tolerance(oracle, sub, X, y, use_mse=use_mse)
        got = err[t, :n]
        # the reference evaluates in float64, the oracle in float32: a node is compared when its float32 result is finite and
        # ulp-stable (the oracle's probe) and well conditioned at float32 resolution -- the same tree evaluated by this module in
        # float32 moves its error by at most 2e-6 relative
        v32 = S.node_values(value[t], type_[t], size[t], X, np.float32)
        with np.errstate(all="ignore"):
            d32 = [y[:, 0].astype(np.float64) - v.astype(np.float64) for v in v32]
            e32 = np.array([np.mean(d * d if use_mse else np.abs(d)) for d in d32])
            ok = np.isfinite(want) & ~unstable & (tol <= 1e-4 * np.abs(want) + 1e-6) & (np.abs(e32 - got) <= 2e-6 * np.abs(got) + 1e-9)
        live += n
        compared += int(ok.sum())
        bad = np.flatnonzero(ok & ~(np.abs(got - want) <= tol))
        assert bad.size == 0, (t, bad[:5], got[bad[:5]], want[bad[:5]], tol[bad[:5]])
        cls = ~unstable
        assert np.array_equal(np.isnan(got[cls]), np.isnan(want[cls]))
        # node 0 is the tree itself
        assert np.isnan(got[0]) or got[0] == pytest.approx(R.forest_grad(value[t:t + 1], type_[t:t + 1], size[t:t + 1], X, y, use_mse)[0][0], rel=1e-12)
    assert compared >= 0.8 * live, (compared, live)


def test_node_const_of_planted_subtrees():
    B, V, C = R.T_BFUNC, R.T_VAR, R.T_CONST
    # ((1.5 + 2.0) * x0) + ((x1 - x1) + (x2 * 0))
    value = np.array([[R.F_ADD, R.F_MUL, R.F_ADD, 1.5, 2.0, 0, R.F_ADD, R.F_SUB, 1, 1, R.F_MUL, 2, 0.0]], np.float32)
    type_ = np.array([[B, B, B, C, C, V, B, B, V, V, B, V, C]], np.int16)
    size = np.array([[13, 5, 3, 1, 1, 1, 7, 3, 1, 1, 3, 1, 1]], np.int16)
    rng = np.random.default_rng(5)
    X = rng.uniform(0.5, 1.5, (40, 4)).astype(np.float32)
    X[:, 3] = 0.25
    y = (3.5 * X[:, :1]).astype(np.float32)
    err, const = S.forest_subtree_errors(value, type_, size, X, y, value_dtype=np.float32)
    assert S.check_prefix_tree(type_[0], size[0])
    want = [NAN, NAN, 3.5, 1.5, 2.0, NAN, 0.0, 0.0, NAN, NAN, 0.0, NAN, 0.0]
    assert np.array_equal(np.isnan(const[0]), np.isnan(want)) and np.array_equal(const[0][~np.isnan(want)], np.array(want)[~np.isnan(want)])
    assert err[0, 0] == 0.0 and err[0, 1] == 0.0 and err[0, 5] > 0
    # a variable is constant only if its column is
    v2 = np.array([[3.0]], np.float32), np.array([[V]], np.int16), np.array([[1]], np.int16)
    assert S.forest_subtree_errors(*v2, X, y)[1][0, 0] == np.float32(0.25)
    # a NaN is never constant: x0 / 0
    v3 = (np.array([[R.F_DIV, 0, 0.0]], np.float32), np.array([[B, V, C]], np.int16), np.array([[3, 1, 1]], np.int16))
    e3, c3 = S.forest_subtree_errors(*v3, X, y)
    assert np.isnan(c3[0, 0]) and np.isnan(e3[0, 0]) and c3[0, 2] == 0.0
    # hoist takes node 1 (the smaller of the two zero-error nodes), fold makes 1.5 + 2.0 one constant
    ov, ot, os_, root, loss = S.prune_rows(value, type_, size, err.astype(np.float32), const)
    assert root[0] == 1 and loss[0] == 0.0
    assert list(ot[0, :3]) == [B, C, V] and list(os_[0, :4]) == [3, 1, 1, 0] and list(ov[0, :3]) == [R.F_MUL, 3.5, 0.0]
    # fold alone: the whole right operand folds to one 0 (outermost wins over x1 - x1 and x2 * 0)
    ov, ot, os_, root, loss = S.prune_rows(value, type_, size, err.astype(np.float32), const, hoist=False)
    assert root[0] == 0 and list(ot[0, :6]) == [B, B, C, V, C, 0] and list(os_[0, :6]) == [5, 3, 1, 1, 1, 0]
    assert list(ov[0, :5]) == [R.F_ADD, R.F_MUL, 3.5, 0.0, 0.0]


def _random_marks(rng, value, type_, size):
    """hand-made node_err / node_const on a real forest: NaNs, infs, exact ties in error, nested foldable nodes"""
    pop, L = value.shape
    err = rng.choice(np.array([0.0, 0.25, 0.25, 1.0, 3.0, np.nan, np.inf], np.float32), (pop, L))
    const = np.where(rng.random((pop, L)) < 0.35, rng.choice(np.array([0.0, -0.0, 2.5, np.inf], np.float32), (pop, L)), NAN).astype(np.float32)
    return err, const


@pytest.mark.parametrize("hoist,fold", [(True, True), (True, False), (False, True), (False, False)])
def test_prune_rule_properties(rng, hoist, fold):
    value, type_, size = random_forest(rng, 200, 64, ALL_FUNCS, 3, 1, max_depth=5)
    size[3, 0] = 0
    type_[4, :] = R.T_CONST
    size[4, 0] = 5
    err, const = _random_marks(rng, value, type_, size)
    err[7] = NAN   # no finite error anywhere: the root stays
    ov, ot, os_, root, loss = S.prune_rows(value, type_, size, err, const, hoist, fold)
    for t in (3, 4):   # malformed: copied through
        assert np.array_equal(ov[t].view(np.uint32), value[t].view(np.uint32)) and np.array_equal(ot[t], type_[t]) and np.array_equal(os_[t], size[t])
        assert root[t] == 0 and np.isnan(loss[t])
    assert root[7] == 0
    for t in range(200):
        if t in (3, 4):
            continue
        n = int(size[t, 0])
        r = int(root[t])
        assert S.check_prefix_tree(ot[t], os_[t]), t
        assert not np.any(ov[t, int(os_[t, 0]):].view(np.uint32))
        assert os_[t, 0] <= size[t, r] <= n
        assert np.array_equal(loss[t:t + 1].view(np.uint32), err[t, r:r + 1].view(np.uint32))
        fin = np.isfinite(err[t, :n])
        if not hoist or not fin.any():
            assert r == 0
        else:
            # the tie order: no finite node beats the chosen one in (error, size, index)
            key = lambda i: (float(err[t, i]), int(size[t, i]), i)   # noqa: E731
            assert fin[r] and all(key(r) <= key(i) for i in np.flatnonzero(fin))
        # outermost wins: walking the old subtree, a foldable function node becomes one CONST and its inside is gone
        want_v, want_t, j = [], [], r
        while j < r + size[t, r]:
            if fold and type_[t, j] not in (R.T_VAR, R.T_CONST) and np.isfinite(const[t, j]):
                want_v.append(const[t, j]); want_t.append(R.T_CONST)
                j += size[t, j]
            else:
                want_v.append(value[t, j]); want_t.append(type_[t, j])
                j += 1
        k = len(want_v)
        assert os_[t, 0] == k and np.array_equal(ot[t, :k], np.array(want_t, np.int16))
        assert np.array_equal(ov[t, :k].view(np.uint32), np.array(want_v, np.float32).view(np.uint32))
        if not fold:
            assert np.array_equal(os_[t, :k], size[t, r:r + k])


@pytest.mark.parametrize("funcs", ["arith", "all"])
def test_prune_twice_is_the_identity(rng, funcs):
    value, type_, size = random_forest(rng, 120, 64, ARITH if funcs == "arith" else ALL_FUNCS, 3, 1, max_depth=5, const_range=(0.0, 1.0))
    X = rng.uniform(0.5, 1.5, (33, 3)).astype(np.float32)
    X[:, 2] = 1.0
    y = rng.uniform(-1, 1, (33, 1)).astype(np.float32)
    err, const = S.forest_subtree_errors(value, type_, size, X, y, value_dtype=np.float32)
    once = S.prune_rows(value, type_, size, err.astype(np.float32), const)
    assert (once[2][:, 0] < size[:, 0]).any() and (once[2][:, 0] <= size[:, 0]).all()
    err2, const2 = S.forest_subtree_errors(*once[:3], X, y, value_dtype=np.float32)
    twice = S.prune_rows(*once[:3], err2.astype(np.float32), const2)
    assert np.all(twice[3] == 0)
    for a, b in zip(once[:3], twice[:3]):
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    assert np.array_equal(once[4].view(np.uint32), twice[4].view(np.uint32))
