"""GPU: the per-subtree pass (csrc/sr_subtree.hip sr_subtree_kernel) against the C oracle on every subtree extracted into a row of its
own and against batch_forward for constancy, the rewrite kernel (prune_rows_kernel) bit for bit against the numpy rule
(tests/subtree_ref.py), and Forest.simplify's invariants on the device."""
import os
import sys

import numpy as np
import pytest
import torch

import evogp_amd  # noqa: F401  (registers the ops)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sr_grad_ref as R  # noqa: E402
import subtree_ref as S  # noqa: E402
from grad_trees import ALL_FUNCS, ARITH, random_forest  # noqa: E402
from helpers import assert_within_sensitivity, fbits, per_tree_tolerance  # noqa: E402

pytestmark = pytest.mark.gpu

B, U, V, C = R.T_BFUNC, R.T_UFUNC, R.T_VAR, R.T_CONST


def _dev(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _subtree(value, type_, size, X, y, use_mse=True):
    v, t, s, Xd, yd = _dev(value, type_, size, X, y)
    pop, L = value.shape
    err, const = torch.ops.evogp_hip.tree_SR_subtree_errors(pop, X.shape[0], L, X.shape[1], 1, use_mse, v, t, s, Xd, yd)
    return err.cpu().numpy(), const.cpu().numpy()


def _prune(value, type_, size, err, const, hoist=True, fold=True):
    out = torch.ops.evogp_hip.tree_prune(1, hoist, fold, *_dev(value, type_, size, err, const))
    return [a.cpu().numpy() for a in out]


def _case(rng, funcs, gp_len, D, pop=24, var_len=3):
    value, type_, size = random_forest(rng, pop, gp_len, ARITH if funcs == "arith" else ALL_FUNCS, var_len, 1, max_depth=5)
    X = rng.uniform(0.5, 1.5, (D, var_len)).astype(np.float32)
    y = rng.uniform(-1, 1, (D, 1)).astype(np.float32)
    return value, type_, size, X, y


def _all_subtrees(value, type_, size, trees=None):
    """every subtree of every (well-formed) tree as a row of its own -> (forest, tree index, node index)"""
    parts, owner, node = [], [], []
    for t in (range(value.shape[0]) if trees is None else trees):
        parts.append(S.extract_subtrees(value, type_, size, t))
        n = parts[-1][0].shape[0]
        owner += [t] * n
        node += list(range(n))
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(3)), np.array(owner), np.array(node)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return np.array_equal(a.view(np.uint32), b.view(np.uint32)) if a.dtype == np.float32 else np.array_equal(a, b)


def _malform(value, type_, size):
    """the three malformed trees of test_gpu_sr_grad.test_layout_determinism_and_malformed_trees"""
    type_[7, :] = C                  # leaves only, size says 5: not one value on the stack at the end
    size[7, 0] = 5
    size[9, 0] = 0                   # empty tree
    value[11, 0], type_[11, 0] = R.F_ADD, B   # the root pops a missing operand
    size[11, 0] = 1
    return (7, 9, 11)


# ---- 1. node_err against the oracle on extracted subtrees ---------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 63, 1024, 5000])
@pytest.mark.parametrize("gp_len", [64, 1024])
@pytest.mark.parametrize("funcs", ["arith", "all"])
def test_node_err_matches_oracle_on_extracted_subtrees(rng, oracle, funcs, gp_len, D):
    value, type_, size, X, y = _case(rng, funcs, gp_len, D)
    sub, owner, node = _all_subtrees(value, type_, size)
    live = np.arange(gp_len)[None, :] < size[:, :1]
    for use_mse in (True, False):
        err, const = _subtree(value, type_, size, X, y, use_mse)
        assert np.isnan(err[~live]).all() and np.isnan(const[~live]).all()   # the tails
        got = err[owner, node].astype(np.float64)
        want, tol, unstable = per_tree_tolerance(oracle, sub, X, y, use_mse=use_mse)
        with np.errstate(all="ignore"):
            cmp = np.isfinite(want) & ~unstable & (tol <= 1e-4 * np.abs(want) + 1e-6)
            off = np.abs(got - want.astype(np.float64))
        print(f"{funcs} L{gp_len} D{D} mse={use_mse}: {cmp.sum()} of {cmp.size} nodes compared, "
              f"worst |got-want|/tol {np.max(off[cmp] / tol[cmp]) if cmp.any() else 0:.3g}")
        assert cmp.mean() >= 0.9, f"only {cmp.sum()} of {cmp.size} live nodes are comparable"
        bad = np.flatnonzero(cmp & ~(off <= tol))
        assert bad.size == 0, (bad.size, owner[bad[:5]], node[bad[:5]], got[bad[:5]], want[bad[:5]], tol[bad[:5]])
        rest = ~cmp & ~unstable   # outside the rule: the NaN / inf class still agrees unless the probe marks it unstable
        assert np.array_equal(np.isnan(got[rest]), np.isnan(want[rest])) and np.array_equal(np.isinf(got[rest]), np.isinf(want[rest]))


@pytest.mark.parametrize("funcs", ["arith", "all"])
def test_root_entry_is_the_loss_of_the_tree(rng, oracle, funcs):
    value, type_, size, X, y = _case(rng, funcs, 64, 300, pop=200)
    err, _ = _subtree(value, type_, size, X, y)
    v, t, s, Xd, yd = _dev(value, type_, size, X, y)
    loss, _ = torch.ops.evogp_hip.tree_SR_gradient(200, 300, 64, 3, 1, True, v, t, s, Xd, yd)
    assert _same_bits(fbits(err[:, 0]), fbits(loss.cpu().numpy()))   # the same sums in the same order
    want, tol, unstable = per_tree_tolerance(oracle, (value, type_, size), X, y)
    assert_within_sensitivity(err[:, 0], want, tol, unstable, "node_err[:, 0] vs the oracle")
    assert_within_sensitivity(err[:, 0], loss.cpu().numpy().astype(np.float64), tol, unstable, "node_err[:, 0] vs tree_SR_gradient")
    fit = torch.ops.evogp_cuda.tree_SR_fitness(200, 300, 64, 3, 1, True, v, t, s, Xd, yd, 4).cpu().numpy()
    assert_within_sensitivity(err[:, 0], fit.astype(np.float64), tol, unstable, "node_err[:, 0] vs tree_SR_fitness")


# ---- 2. node_const -------------------------------------------------------------------------------------------------------------------
def _plant(value, type_, size, t, nodes):
    value[t], type_[t], size[t] = 0, 0, 0
    for i, (v, ty, s) in enumerate(nodes):
        value[t, i], type_[t, i], size[t, i] = v, ty, s


def _join(value, type_, size, t, src, parts):
    """row t = parts[0] + (parts[1] + (... + parts[-1])), the parts being rows of the forest `src`"""
    lens = [int(src[2][p, 0]) for p in parts]
    value[t], type_[t], size[t] = 0, 0, 0
    at = 0
    for k, p in enumerate(parts):
        if k + 1 < len(parts):
            value[t, at], type_[t, at], size[t, at] = R.F_ADD, B, sum(lens[k:]) + len(parts) - 1 - k
            at += 1
        value[t, at:at + lens[k]], type_[t, at:at + lens[k]], size[t, at:at + lens[k]] = (a[p, :lens[k]] for a in src)
        at += lens[k]


@pytest.mark.parametrize("gp_len", [64, 1024])
def test_node_const_is_what_batch_forward_shows(rng, gp_len):
    from evogp_amd.tree import Forest

    value, type_, size, X, y = _case(rng, "arith", gp_len, 777, pop=200, var_len=4)
    X[:, 3] = 0.75                                                       # one constant column
    _plant(value, type_, size, 0, [(R.F_MUL, B, 5), (R.F_ADD, B, 3), (1.5, C, 1), (2.0, C, 1), (0, V, 1)])          # (1.5 + 2.0) * x0
    _plant(value, type_, size, 1, [(R.F_ADD, B, 5), (R.F_SUB, B, 3), (1, V, 1), (1, V, 1), (0, V, 1)])              # (x1 - x1) + x0
    _plant(value, type_, size, 2, [(R.F_SUB, B, 5), (R.F_MUL, B, 3), (2, V, 1), (0.0, C, 1), (1, V, 1)])            # x2 * 0 - x1
    _plant(value, type_, size, 3, [(R.F_DIV, B, 3), (0, V, 1), (0.0, C, 1)])                                        # x0 / 0: a NaN is not constant
    _, const = _subtree(value, type_, size, X, y)
    assert const[0, 1] == 3.5 and np.isnan(const[0, 0]) and const[1, 1] == 0.0 and const[2, 1] == 0.0 and np.isnan(const[3, 0])
    sub, owner, node = _all_subtrees(value, type_, size)
    f = Forest(4, 1, *_dev(*sub))
    pred = f.batch_forward(torch.from_numpy(X).cuda()).cpu().numpy()[:, :, 0]   # (subtrees, D)
    bits = np.ascontiguousarray(pred).view(np.uint32)
    is_const = (bits == bits[:, :1]).all(1) & ~np.isnan(pred[:, 0])
    got = const[owner, node]
    assert np.array_equal(~np.isnan(got), is_const)
    assert np.array_equal(got[is_const].view(np.uint32), bits[is_const, 0])
    inner = is_const & (sub[2][:, 0] > 1)
    assert inner.sum() >= 20, f"only {inner.sum()} constant subtrees that are not leaves"
    assert (is_const & (sub[1][:, 0] == V)).any() and (~is_const & (sub[1][:, 0] == V)).any()   # the constant column, and the others


# ---- 3. tree_prune against the numpy rule -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gp_len", [64, 1024])
def test_prune_is_the_numpy_rule_bit_for_bit(rng, gp_len):
    value, type_, size = random_forest(rng, 300, gp_len, ALL_FUNCS, 3, 1, max_depth=6, const_range=(0.0, 1.0))
    if gp_len > 64:   # rows of several 64-node chunks: twenty of the trees under a comb of additions
        src = (value.copy(), type_.copy(), size.copy())
        for t in range(20, 60):
            _join(value, type_, size, t, src, [(t + 7 * k) % 300 for k in range(20)])
        assert size[:, 0].max() > 128
    X = rng.uniform(0.5, 1.5, (200, 3)).astype(np.float32)
    X[:, 2] = 1.0
    y = rng.uniform(-1, 1, (200, 1)).astype(np.float32)
    bad = _malform(value, type_, size)
    err, const = _subtree(value, type_, size, X, y)
    # hand-made marks on the same forest: NaNs, infs, exact ties in error, -0.0, nested foldable nodes
    err2 = rng.choice(np.array([0.0, 0.25, 0.25, 1.0, 3.0, np.nan, np.inf], np.float32), value.shape)
    const2 = np.where(rng.random(value.shape) < 0.35, rng.choice(np.array([0.0, -0.0, 2.5, np.inf], np.float32), value.shape),
                      np.float32(np.nan)).astype(np.float32)
    err2[5] = np.nan
    for e, c in ((err, const), (err2, const2)):
        for hoist in (True, False):
            for fold in (True, False):
                got = _prune(value, type_, size, e, c, hoist, fold)
                want = S.prune_rows(value, type_, size, e, c, hoist, fold)
                for name, a, b in zip(("value", "type", "size", "root_pos", "loss"), got, want):
                    assert _same_bits(a, b), (name, hoist, fold, np.argwhere(np.atleast_2d(fbits(a) if a.dtype == np.float32 else a)
                                                                                   != np.atleast_2d(fbits(b) if b.dtype == np.float32 else b))[:3])
                for t in bad:   # malformed: unchanged
                    assert _same_bits(got[0][t], value[t]) and np.array_equal(got[1][t], type_[t]) and np.array_equal(got[2][t], size[t])
                    assert got[3][t] == 0 and np.isnan(got[4][t])
    rewritten = _prune(value, type_, size, err, const)
    assert (rewritten[2][:, 0] < size[:, 0]).mean() > 0.2   # (the check is not about trees that stay as they are)


# ---- 4. Forest.simplify ------------------------------------------------------------------------------------------------------------
def _check_simplified(f0, keep, f1, loss, Xd, yd, oracle, X, y, name):
    for a, b in zip(keep, f0._tensors()):
        assert torch.equal(a, b)   # the input forest is untouched
    s0 = f0.batch_subtree_size[:, 0].clamp(0, f0.max_tree_len)
    s1 = f1.batch_subtree_size[:, 0]
    assert bool((s1 <= s0).all()), "a tree grew"
    node_err, node_const = f0.SR_subtree_errors(Xd, yd)
    value, ntype, size = f0._tensors()
    _, _, _, root, _ = torch.ops.evogp_hip.tree_prune(1, True, True, value, ntype, size, node_err, node_const)
    at_root = node_err.gather(1, root.long()[:, None])[:, 0]
    assert torch.equal(at_root.view(torch.int32), loss.view(torch.int32))   # the returned loss is node_err at root_pos, bitwise
    trees = tuple(a.cpu().numpy() for a in f1._tensors())
    want, tol, unstable = per_tree_tolerance(oracle, trees, X, y)
    fit = f1.SR_fitness(Xd, yd).cpu().numpy()
    lossn = loss.cpu().numpy()
    with np.errstate(all="ignore"):
        off = np.abs(fit.astype(np.float64) - lossn)
        ok = ~unstable & np.isfinite(lossn)
        print(f"{name}: SR_fitness vs returned loss: {int((off[ok] > tol[ok]).sum())} of {int(ok.sum())} stable finite entries beyond "
              f"their tolerance, worst ratio {np.max(off[ok] / np.maximum(tol[ok], 1e-300)):.3g}; {int(unstable.sum())} unstable")
    assert_within_sensitivity(fit, lossn.astype(np.float64), tol, unstable, f"{name}: SR_fitness of the simplified forest vs its returned loss")
    f2, loss2 = f1.simplify(Xd, yd)
    for a, b in zip(f1._tensors(), f2._tensors()):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
    assert torch.equal(loss.view(torch.int32), loss2.view(torch.int32))


def test_simplify_invariants_on_random_trees(rng, oracle):
    from evogp_amd.tree import Forest

    value, type_, size, X, y = _case(rng, "all", 64, 500, pop=400)
    size[5, 0] = 0
    _plant(value, type_, size, 6, [(R.F_MUL, B, 5), (R.F_DIV, B, 3), (0, V, 1), (0.0, C, 1), (1, V, 1)])   # (x0 / 0) * x1: NaN as a whole
    v, t, s, Xd, yd = _dev(value, type_, size, X, y)
    f0 = Forest(3, 1, v, t, s)
    keep = [a.clone() for a in (v, t, s)]
    assert np.isnan(float(f0.SR_fitness(Xd, yd)[6]))
    f1, loss = f0.simplify(Xd, yd)
    _check_simplified(f0, keep, f1, loss, Xd, yd, oracle, X, y, "400 random trees")
    assert np.isnan(float(loss[5])) and torch.equal(f1.batch_node_value[5].view(torch.int32), v[5].view(torch.int32))
    # the tree that is NaN as a whole but has a finite subtree comes back finite
    assert np.isfinite(float(loss[6])) and int(f1.batch_subtree_size[6, 0]) == 1 and np.isfinite(float(f1.SR_fitness(Xd, yd)[6]))
    for tt in range(400):
        if tt != 5:
            assert S.check_prefix_tree(f1.batch_node_type[tt].cpu().numpy(), f1.batch_subtree_size[tt].cpu().numpy())


def test_simplify_configs1_forest(oracle):
    from evogp_amd.tree import Forest, GenerateDescriptor

    desc = GenerateDescriptor(max_tree_len=64, input_len=10, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=6,
                              const_samples=[-1, 0, 1])
    f0 = Forest.random_generate(100_000, desc, keys=torch.tensor([42, 0], dtype=torch.uint32, device="cuda"))
    rng = np.random.default_rng(1234)
    X = rng.uniform(-5, 5, (1024, 10)).astype(np.float32)
    y = (X[:, 0] * X[:, 1] + X[:, 2] * X[:, 3] - X[:, 4] + 0.5 * X[:, 5] ** 2).astype(np.float32)[:, None]
    Xd, yd = _dev(X, y)
    keep = [a.clone() for a in f0._tensors()]
    f1, loss = f0.simplify(Xd, yd)
    assert f1.func_mask == f0.func_mask != 0
    _check_simplified(f0, keep, f1, loss, Xd, yd, oracle, X, y, "configs[1] forest")
    before = f0.batch_subtree_size[:, 0].float().mean().item()
    after = f1.batch_subtree_size[:, 0].float().mean().item()
    print(f"configs[1] forest: mean tree size {before:.3f} -> {after:.3f}")
    assert after < before
    # no tree got worse: the returned loss is at most the tree's own loss wherever that is finite
    own = f0.SR_subtree_errors(Xd, yd)[0][:, 0]
    fin = torch.isfinite(own)
    assert bool((loss[fin] <= own[fin]).all())


# ---- 5. planted cases ---------------------------------------------------------------------------------------------------------------
def test_planted_cases():
    from evogp_amd.tree import Forest

    rng = np.random.default_rng(3)
    X = rng.uniform(0.5, 1.5, (300, 4)).astype(np.float32)
    y = (X[:, 0] * X[:, 1]).astype(np.float32)[:, None]
    value, type_, size = (np.zeros((2, 64), np.float32), np.zeros((2, 64), np.int16), np.zeros((2, 64), np.int16))
    _plant(value, type_, size, 0, [(R.F_MUL, B, 5), (R.F_MUL, B, 3), (0, V, 1), (1, V, 1), (3.0, C, 1)])                 # (x0 * x1) * 3
    _plant(value, type_, size, 1, [(R.F_ADD, B, 9), (R.F_MUL, B, 3), (0, V, 1), (1, V, 1), (R.F_MUL, B, 5), (R.F_SUB, B, 3), (2, V, 1),
                                   (2, V, 1), (3, V, 1)])                                                                # x0 * x1 + (x2 - x2) * x3
    v, t, s, Xd, yd = _dev(value, type_, size, X, y)
    f0 = Forest(4, 1, v, t, s)
    f1, loss = f0.simplify(Xd, yd)
    v1, t1, s1 = (a.cpu().numpy() for a in f1._tensors())
    for k in range(2):   # both come back as x0 * x1 with loss 0 (in the second tree the product alone is as good as the sum, and smaller)
        assert list(t1[k, :4]) == [B, V, V, 0] and list(s1[k, :4]) == [3, 1, 1, 0] and list(v1[k, :3]) == [R.F_MUL, 0, 1]
        assert float(loss[k]) == 0.0 and not v1[k, 3:].any() and not s1[k, 3:].any()
    # folding alone turns the second into x0 * x1 + 0
    f2, loss2 = f0.simplify(Xd, yd, hoist=False)
    v2, t2, s2 = (a.cpu().numpy() for a in f2._tensors())
    assert list(t2[1, :6]) == [B, B, V, V, C, 0] and list(s2[1, :6]) == [5, 3, 1, 1, 1, 0] and list(v2[1, :5]) == [R.F_ADD, R.F_MUL, 0, 1, 0.0]
    assert float(loss2[1]) == 0.0 and float(loss2[0]) > 0.0 and np.array_equal(s2[0], size[0])
    assert float(f2.SR_fitness(Xd, yd)[1]) == 0.0
    # constancy is about bit patterns: where x3 changes sign, 0 * x3 is 0.0 on some rows and -0.0 on others, so only x2 - x2 folds
    X[::2, 3] *= -1
    f3, loss3 = f0.simplify(torch.from_numpy(X).cuda(), yd, hoist=False)
    assert list(f3.batch_node_type[1, :8].cpu().numpy()) == [B, B, V, V, B, C, V, 0] and float(loss3[1]) == 0.0


# ---- 6. determinism, malformed trees, argument errors ---------------------------------------------------------------------------------
@pytest.mark.parametrize("gp_len", [64, 1024])
def test_determinism_and_malformed_trees(rng, gp_len):
    value, type_, size, X, y = _case(rng, "all", gp_len, 777, pop=300)
    bad = _malform(value, type_, size)
    a = _subtree(value, type_, size, X, y)
    b = _subtree(value, type_, size, X, y)
    assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1])
    for t in bad:
        assert np.isnan(a[0][t]).all() and np.isnan(a[1][t]).all()
    p1 = _prune(value, type_, size, *a)
    p2 = _prune(value, type_, size, *a)
    for x, z in zip(p1, p2):
        assert _same_bits(x, z)
    for t in bad:
        assert _same_bits(p1[0][t], value[t]) and np.array_equal(p1[1][t], type_[t]) and np.array_equal(p1[2][t], size[t])
        assert p1[3][t] == 0 and np.isnan(p1[4][t])
    # a population that fills the device gets one wave per tree instead of four: the same rows through another split of the row tiles.
    # The constancy verdicts agree exactly, the errors to rounding
    reps = 4200 // 300
    c = _subtree(np.tile(value, (reps, 1)), np.tile(type_, (reps, 1)), np.tile(size, (reps, 1)), X, y)
    for k in (0, reps - 1):
        ck = (c[0][k * 300:(k + 1) * 300], c[1][k * 300:(k + 1) * 300])
        assert np.array_equal(fbits(ck[1]), fbits(a[1]))
        with np.errstate(all="ignore"):
            fin = np.isfinite(ck[0]) & np.isfinite(a[0])
            assert np.array_equal(np.isnan(ck[0]), np.isnan(a[0]))
            assert np.allclose(ck[0][fin], a[0][fin], rtol=1e-5)


def test_argument_errors_without_launch():
    from evogp_amd import _lib

    L = _lib.lib
    p, q = 8, 16  # (never dereferenced: the checks come first)
    assert L.evogp_hip_sr_subtree_errors(0, 8, 32, 3, 1, 1, p, p, p, p, p, p, p, None) == -1
    assert L.evogp_hip_sr_subtree_errors(4, 8, 2000, 3, 1, 1, p, p, p, p, p, p, p, None) == -1
    assert L.evogp_hip_sr_subtree_errors(4, 8, 32, 3, 1, 1, None, p, p, p, p, p, p, None) == -2
    assert L.evogp_hip_sr_subtree_errors(4, 8, 32, 3, 3, 1, p, p, p, p, p, p, p, None) == -1
    assert L.evogp_hip_prune_rows(0, 32, 1, 1, 1, p, p, p, p, p, q, q, q, q, q, None) == -1
    assert L.evogp_hip_prune_rows(4, 2000, 1, 1, 1, p, p, p, p, p, q, q, q, q, q, None) == -1
    assert L.evogp_hip_prune_rows(4, 32, 1, 1, 1, None, p, p, p, p, q, q, q, q, q, None) == -2
    assert L.evogp_hip_prune_rows(4, 32, 3, 1, 1, p, p, p, p, p, q, q, q, q, q, None) == -1
    z = _dev(np.zeros((4, 32), np.float32), np.zeros((4, 32), np.int16), np.zeros((4, 32), np.int16))
    with pytest.raises(RuntimeError):
        torch.ops.evogp_hip.tree_SR_subtree_errors(4, 8, 32, 3, 3, True, *z, *_dev(np.zeros((8, 3), np.float32), np.zeros((8, 3), np.float32)))
    with pytest.raises(RuntimeError):
        torch.ops.evogp_hip.tree_prune(3, True, True, *z, *_dev(np.zeros((4, 32), np.float32), np.zeros((4, 32), np.float32)))
    with pytest.raises(RuntimeError):
        torch.ops.evogp_hip.tree_prune(1, True, True, *z, *_dev(np.zeros((4, 31), np.float32), np.zeros((4, 32), np.float32)))
