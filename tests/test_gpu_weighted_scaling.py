"""GPU: linear scaling under sample weights with held-out scoring (csrc/sr_wscale.hip) against the numpy restatement
(tests/weighted_scaling_ref.py) on the device's own batch_forward predictions, the rules that decide a value exactly, the new call next
to tree_SR_linear_scaling, and the problem / pipeline on the device."""
import os
import sys

import numpy as np
import pytest
import torch

import evogp_amd  # noqa: F401  (registers the ops)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import linear_scaling_ref as LS  # noqa: E402
import sr_grad_ref as R  # noqa: E402
import test_gpu_binding_contract as BC  # noqa: E402
import weighted_scaling_ref as WS  # noqa: E402
from test_gpu_linear_scaling import _case, _dev, _plant  # noqa: E402
from test_gpu_subtree import _malform  # noqa: E402

from evogp_amd.tree import Forest  # noqa: E402

pytestmark = pytest.mark.gpu

B, V, C = R.T_BFUNC, R.T_VAR, R.T_CONST
TILE = 1024   # rows per workgroup tile of sr_wscale_kernel: 64 lanes x 4 rows x 4 waves; a wave's tile is 256 rows

# The new op joins the binding-contract table (tests/test_gpu_binding_contract.py: one row per op, every argument faulted in turn; its
# test_the_table_covers_every_op reads the table when it runs).  The row is checked below, by that module's own test body.
_OP = "evogp_hip::tree_SR_weighted_scaling"
BC.TABLE[_OP] = lambda: dict(args=BC._data_head(1, use_mse=False) + BC._forest() + BC._xy() + [BC._f("weights", 2, BC.D)],
                             outs=[((BC.POP, 2), BC.F32), ((BC.POP, 2), BC.F32)], scalars=dict(BC.SIZES, out_len=(0, 2)),
                             tensors={"weights": [("of no rows", torch.zeros(0, BC.D)), ("of nine rows", torch.zeros(9, BC.D))]},
                             also=[("no weights", {"weights": None}, [((BC.POP, 1), BC.F32), ((BC.POP, 2), BC.F32)])])


def test_binding_contract_of_the_new_op():
    BC.test_valid_call_and_one_fault_at_a_time(_OP)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _scaled(value, type_, size, X, y, W):
    """the op itself: loss (pop, K) float32 (K = 1 without weights), intercept, slope"""
    v, t, s, Xd, yd = _dev(value, type_, size, X, y)
    Wd = None if W is None else _dev(np.asarray(W, np.float32).reshape(-1, X.shape[0]))[0]
    pop, L = value.shape
    loss, coef = torch.ops.evogp_hip.tree_SR_weighted_scaling(pop, X.shape[0], L, X.shape[1], 1, v, t, s, Xd, yd, Wd)
    assert loss.shape == (pop, 1 if W is None else Wd.shape[0]) and coef.shape == (pop, 2) and loss.dtype == coef.dtype == torch.float32
    coef = coef.cpu().numpy()
    return loss.cpu().numpy(), coef[:, 0].copy(), coef[:, 1].copy()


def _predictions(value, type_, size, X):
    v, t, s, Xd = _dev(value, type_, size, X)
    pop, L = value.shape
    return torch.ops.evogp_hip.tree_batch_evaluate(pop, X.shape[0], L, X.shape[1], 1, v, t, s, Xd)[:, :, 0].cpu().numpy()


def _weights(rng, K, D):
    """uniform(0.5, 2) with 30 % of the entries exactly 0; a row that came out with fewer than two weighted entries gets them back where
    D allows, so that every row can be used (the unusable rows and the one-row column are rules of their own, below)"""
    W = rng.uniform(0.5, 2, (K, D)).astype(np.float32)
    W[rng.random((K, D)) < 0.3] = 0
    for k in range(K):
        for d in range(min(D, 2)):
            if np.count_nonzero(W[k]) < min(D, 2) and W[k, d] == 0:
                W[k, d] = np.float32(rng.uniform(0.5, 2))
    return W


def _check(value, type_, size, X, y, W, what, P=None):
    P = _predictions(value, type_, size, X) if P is None else P
    loss, a, b = _scaled(value, type_, size, X, y, W)
    ref = WS.scaling(P, y, W)
    excluded = WS.check_against(ref, loss, a, b, X.shape[0], what=what)
    assert excluded <= 0.10, what
    return ref, loss, a, b


# ---- 1. against the restatement on the device's own predictions ------------------------------------------------------------------------
# D: a lane tile (1, 2), a wave tile (63 .. 257 around 64 and 256), the workgroup tile (1023 .. 1025), several tiles per wave (5000: rows
# and weights reloaded per tree); var_len on both sides of the two register-tuple widths (<= 12, 13 .. 32) and past them (the
# scratch-stack kernel alone); 'arith' forests stay in the LEAN build, 'all' forests send trees to the FULL one, the chains _case plants
# (20 operations at gp_len 64, up to 400 at 1024) go on to the scratch stack; K = None (nothing loaded), 1 and 2 (the 2-column build),
# 3 and 8 (the 8-column build).
CASES = [
    ("arith", 64, 3, 63, 1, None), ("all", 64, 3, 257, 2, 1), ("arith", 1024, 3, 63, 63, 2), ("all", 64, 40, 63, 64, 3),
    ("all", 1024, 3, 257, 65, 8), ("arith", 64, 13, 257, 255, 2), ("all", 64, 3, 257, 257, 3), ("all", 64, 13, 63, 1023, 8),
    ("arith", 64, 3, 257, 1024, 2), ("all", 1024, 13, 63, 1025, None), ("all", 64, 3, 63, 5000, 2), ("arith", 1024, 40, 63, 5000, 3),
    ("all", 64, 13, 257, 5000, 8), ("all", 64, 3, 1, 64, 2), ("arith", 1024, 40, 1, 65, 1), ("all", 64, 40, 257, 1023, 8),
    ("all", 64, 3, 257, 1024, 8), ("arith", 64, 13, 63, 1, 3), ("all", 64, 3, 63, 2, 8), ("all", 1024, 40, 63, 257, 2),
    ("all", 64, 3, 257, 1025, 1), ("arith", 64, 3, 63, 255, None),
]


@pytest.mark.parametrize("funcs,gp_len,var_len,pop,D,K", CASES)
def test_matches_reference_on_batch_forward_predictions(rng, funcs, gp_len, var_len, pop, D, K):
    value, type_, size, X, y = _case(rng, funcs, gp_len, var_len, pop, D)
    W = None if K is None else _weights(rng, K, D)
    ref, loss, a, b = _check(value, type_, size, X, y, W, f"{funcs} L{gp_len} v{var_len} pop{pop} D{D} K={K}")
    assert pop < 24 or np.isfinite(ref["a"]).sum() >= pop // 4
    assert pop < 24 or np.all(np.isfinite(ref["loss"]).sum(axis=0) >= pop // 4)


# ---- 2. weight rows that leave whole units without weight --------------------------------------------------------------------------------
@pytest.mark.parametrize("funcs,var_len", [("arith", 3), ("all", 13), ("all", 40)])
def test_units_without_weight_join_as_nothing(rng, funcs, var_len):
    pop = 63
    # D = 1024: column 0 zero on a whole wave's rows (256 .. 511); 0/1 complement masks
    value, type_, size, X, y = _case(rng, funcs, 64, var_len, pop, TILE)
    P = _predictions(value, type_, size, X)
    W = _weights(rng, 3, TILE)
    W[0, 256:512] = 0
    m = (rng.random(TILE) < 0.3).astype(np.float32)
    _check(value, type_, size, X, y, W, f"{funcs} v{var_len}: a wave's tile without weight", P)
    _check(value, type_, size, X, y, np.stack([1 - m, m]), f"{funcs} v{var_len}: complement masks", P)
    _check(value, type_, size, X, y, np.stack([m, 1 - m, np.ones_like(m)]), f"{funcs} v{var_len}: complement masks, swapped", P)
    # D = 5000: column 0 zero on a whole workgroup tile (1024 .. 2047), a score column zero on everything but one tile
    value, type_, size, X, y = _case(rng, funcs, 64, var_len, pop, 5000)
    W = _weights(rng, 2, 5000)
    W[0, TILE:2 * TILE] = 0
    W[1, :4 * TILE] = 0
    _check(value, type_, size, X, y, W, f"{funcs} v{var_len}: a workgroup tile without weight")


# ---- 3. the rules that decide a value exactly ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,var_len", [(300, 3), (TILE + 7, 13), (300, 40), (TILE + 7, 32)])
def test_exact_rules(rng, D, var_len):
    pop = 40
    value, type_, size, X, y = _case(rng, "all", 64, var_len, pop, D)
    held = rng.random(D) < 0.3
    held[[0, 1, 2, 3]] = [True, False, False, True]
    train = ~held
    X[train, 0] = np.float32(0.875)   # x0 is one value on the training rows and varies on the held-out rows
    h, r = int(np.flatnonzero(held)[len(np.flatnonzero(held)) // 2]), int(np.flatnonzero(train)[3])
    bad = _malform(value, type_, size)
    _plant(value, type_, size, 0, [(0.75, C, 1)])                                      # a CONST tree
    _plant(value, type_, size, 1, [(R.F_SUB, B, 3), (0, V, 1), (0, V, 1)])             # x0 - x0
    _plant(value, type_, size, 3, [(0, V, 1)])                                         # x0: flat on column 0 only
    # 1 / (x0 - c): a division by zero on ONE held-out row (4), on the training rows (5)
    _plant(value, type_, size, 4, [(R.F_DIV, B, 5), (1.0, C, 1), (R.F_SUB, B, 3), (0, V, 1), (X[h, 0], C, 1)])
    _plant(value, type_, size, 5, [(R.F_DIV, B, 5), (1.0, C, 1), (R.F_SUB, B, 3), (0, V, 1), (X[r, 0], C, 1)])
    P = _predictions(value, type_, size, X)
    assert not np.isfinite(P[4, h]) and np.isfinite(np.delete(P[4], h)).all() and not np.isfinite(P[5, r])
    wt = _weights(rng, 1, D)[0]
    wt[[0, 1, 2, 3, h, r]] = 1.0   # (the rows the planted trees are about carry weight)
    W = np.stack([wt * train, wt * held]).astype(np.float32)
    ref, loss, a, b = _check(value, type_, size, X, y, W, f"rules D{D} v{var_len}", P)
    # flat trees: slope +0, and one intercept and one pair of losses for all of them, bit for bit (they share every sum but zeros)
    for t in (0, 1, 3):
        assert _bits(b[t]) == 0 and _bits(a[t]) == _bits(a[0]) and np.array_equal(_bits(loss[t]), _bits(loss[0])), (t, loss[t], a[t], b[t])
    assert np.isfinite(loss[3]).all() and np.isfinite(a[0]), "x0: flat on the training rows, finite and scored on the held-out rows"
    yt = y[train, 0].astype(np.float64)
    wtt = wt[train].astype(np.float64)
    assert abs(a[0] - (wtt * yt).sum() / wtt.sum()) <= 1e-6 * abs(a[0])
    # a division by zero where only column 1 looks: column 0 and the coefficients are finite, column 1 is NaN; the converse: all NaN
    assert np.isfinite(loss[4, 0]) and np.isfinite(a[4]) and np.isfinite(b[4]) and np.isnan(loss[4, 1])
    assert np.isnan(loss[5]).all() and np.isnan(a[5]) and np.isnan(b[5])
    swapped = _scaled(value, type_, size, X, y, W[::-1].copy())
    assert np.isnan(swapped[0][4]).all() and np.isnan(swapped[1][4]) and np.isnan(swapped[2][4])
    for t in bad:
        assert np.isnan(loss[t]).all() and np.isnan(a[t]) and np.isnan(b[t]), t
    assert np.isfinite(loss).all(axis=1).sum() >= 10
    # a column with one weighted row: as a score column the squared residual of that row; as column 0 every tree is flat, the intercept
    # is that row's label and the training loss 0, exactly
    one = np.zeros(D, np.float32)
    one[r] = 1.5
    ref1, l1, a1, b1 = _check(value, type_, size, X, y, np.stack([W[0], one]), f"one row scored D{D} v{var_len}", P)
    ref2, l2, a2, b2 = _check(value, type_, size, X, y, np.stack([one, W[1]]), f"one row fitted D{D} v{var_len}", P)
    ok = np.isfinite(a2)
    assert ok.sum() >= 10 and np.all(_bits(b2[ok]) == 0) and np.all(_bits(a2[ok]) == _bits(y[r, 0])) and np.all(_bits(l2[ok, 0]) == 0)
    # weight rows that may not be used: in column 0 everything is NaN for every tree; in a score column that column alone
    zero, neg, inf = np.zeros(D, np.float32), W[0].copy(), W[0].copy()
    neg[r], inf[r] = -0.5, np.inf
    for row in (zero, neg, inf):
        first = _scaled(value, type_, size, X, y, np.stack([row, W[1]]))
        assert all(np.isnan(x).all() for x in first)
        third = _scaled(value, type_, size, X, y, np.stack([W[0], row, W[1]]))
        assert np.isnan(third[0][:, 1]).all() and np.array_equal(_bits(third[0][:, [0, 2]]), _bits(loss))
        assert np.array_equal(_bits(third[1]), _bits(a)) and np.array_equal(_bits(third[2]), _bits(b))


# ---- 4. bits: columns, weight scale, runs, dedup ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,var_len", [(300, 3), (TILE + 7, 13), (5000, 3), (300, 40)])
def test_column_independence_weight_scale_and_determinism(rng, D, var_len):
    pop = 40
    value, type_, size, X, y = _case(rng, "all", 64, var_len, pop, D)
    W3 = _weights(rng, 3, D)
    three = _scaled(value, type_, size, X, y, W3)
    assert np.isfinite(three[0]).all(axis=1).sum() >= 10
    # column k of the 3-row call (the 8-column build) is column 1 of the 2-row call with rows (0, k) (the 2-column build)
    for k in (1, 2):
        two = _scaled(value, type_, size, X, y, W3[[0, k]])
        assert np.array_equal(_bits(two[0][:, 1]), _bits(three[0][:, k])) and np.array_equal(_bits(two[0][:, 0]), _bits(three[0][:, 0])), k
        assert np.array_equal(_bits(two[1]), _bits(three[1])) and np.array_equal(_bits(two[2]), _bits(three[2]))
    alone = _scaled(value, type_, size, X, y, W3[0])
    assert np.array_equal(_bits(alone[0][:, 0]), _bits(three[0][:, 0])) and np.array_equal(_bits(alone[1]), _bits(three[1]))
    # a power of two on a weight row moves no bit
    for f, rows in ((4.0, [0]), (2.0 ** -7, [2]), (2.0 ** 9, [0, 1, 2])):
        Ws = W3.copy()
        Ws[rows] *= np.float32(f)
        for g, w in zip(_scaled(value, type_, size, X, y, Ws), three):
            assert np.array_equal(_bits(g), _bits(w)), (f, rows)
    # no weights is a row of ones, and two identical calls give equal bits
    ones = _scaled(value, type_, size, X, y, np.ones(D, np.float32))
    for g, w in zip(_scaled(value, type_, size, X, y, None), ones):
        assert np.array_equal(_bits(g), _bits(w))
    for g, w in zip(_scaled(value, type_, size, X, y, W3), three):
        assert np.array_equal(_bits(g), _bits(w))
    # dedup=True gives the plain call's bits on a forest with duplicate rows
    value2, type2, size2 = (np.concatenate([x, x[:17]]) for x in (value, type_, size))
    forest = Forest(var_len, 1, *_dev(value2, type2, size2))
    Xd, yd, Wd = _dev(X, y, W3)
    plain = [x.cpu().numpy() for x in forest.SR_weighted_scaled_fitness(Xd, yd, Wd)]
    dedup = [x.cpu().numpy() for x in forest.SR_weighted_scaled_fitness(Xd, yd, Wd, dedup=True)]
    assert plain[0].shape == (pop + 17, 3) and plain[1].shape == (pop + 17,)
    for g, w in zip(dedup, plain):
        assert np.array_equal(_bits(g), _bits(w))
    assert np.array_equal(_bits(plain[0][:pop]), _bits(three[0])) and np.array_equal(_bits(plain[0][pop:]), _bits(three[0][:17]))
    assert np.array_equal(_bits(plain[1][:pop]), _bits(three[2])) and np.array_equal(_bits(plain[2][:pop]), _bits(three[1]))
    flat = forest.SR_weighted_scaled_fitness(Xd, yd, Wd[1])
    assert flat[0].shape == (pop + 17,)


def test_graph_capture_replays_the_call(rng):
    value, type_, size, X, y = _case(rng, "arith", 64, 3, 200, 300)
    v, t, s, Xd, yd, Wd = _dev(value, type_, size, X, y, _weights(rng, 2, 300))
    args = (200, 300, 64, 3, 1, v, t, s, Xd, yd, Wd)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        eager = torch.ops.evogp_hip.tree_SR_weighted_scaling(*args)   # (the stream's counter ring is made outside the capture)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            out = torch.ops.evogp_hip.tree_SR_weighted_scaling(*args)
        for _ in range(2):
            out[0].fill_(7.0)
            out[1].fill_(7.0)
            g.replay()
            side.synchronize()
            assert np.array_equal(_bits(out[0].cpu().numpy()), _bits(eager[0].cpu().numpy()))
            assert np.array_equal(_bits(out[1].cpu().numpy()), _bits(eager[1].cpu().numpy()))


# ---- 5. next to what exists ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("funcs,gp_len,var_len,pop,D", [("all", 64, 3, 257, 300), ("arith", 1024, 13, 100, TILE + 7), ("all", 64, 40, 24, 70)])
def test_unit_weights_agree_with_linear_scaling(rng, funcs, gp_len, var_len, pop, D):
    value, type_, size, X, y = _case(rng, funcs, gp_len, var_len, pop, D)
    v, t, s, Xd, yd = _dev(value, type_, size, X, y)
    l0, coef0 = torch.ops.evogp_hip.tree_SR_linear_scaling(pop, D, gp_len, var_len, 1, v, t, s, Xd, yd)
    l0, a0, b0 = l0.cpu().numpy().astype(np.float64), coef0[:, 0].cpu().numpy().astype(np.float64), coef0[:, 1].cpu().numpy().astype(np.float64)
    ref = LS.scaling(_predictions(value, type_, size, X), y)
    rtol, atol = LS.tolerance(ref["kappa"], D, ref["syy_D"])
    with np.errstate(invalid="ignore"):
        cmp = np.isfinite(ref["loss"]) & (ref["kappa"] < 1e8)
    assert cmp.sum() >= pop // 4
    for W in (None, np.ones((1, D), np.float32)):
        loss, a, b = _scaled(value, type_, size, X, y, W)
        for name, got, want, at in (("loss", loss[:, 0], l0, atol), ("a", a, a0, 0.0), ("b", b, b0, 0.0)):
            assert np.array_equal(np.isnan(got), np.isnan(want)), name
            off = np.abs(got.astype(np.float64) - want)
            assert np.all(off[cmp] <= (rtol * np.abs(want) + at)[cmp]), (name, np.flatnonzero(cmp & ~(off <= rtol * np.abs(want) + at))[:5])


def test_problem_and_pipeline_on_the_device(rng):
    from evogp_amd.algorithm import DefaultCrossover, DefaultMutation, DefaultSelection, GeneticProgramming
    from evogp_amd.pipeline import StandardPipeline
    from evogp_amd.problem import SymbolicRegression
    from evogp_amd.tree import GenerateDescriptor

    D, pop = 300, 257
    value, type_, size, X, y = _case(rng, "all", 64, 3, pop, D)
    forest = Forest(3, 1, *_dev(value, type_, size))
    Xd, yd = _dev(X, y)
    w = _weights(rng, 1, D)[0]
    m = rng.random(D) < 0.3
    wd, md = torch.from_numpy(w).cuda(), torch.from_numpy(m).cuda()
    opts = dict(datapoints=Xd, labels=yd, linear_scaling=True, scaling_loss="problem", sample_weights=wd, validation_mask=md)
    prob, twin = SymbolicRegression(**opts), SymbolicRegression(**opts, execute_mode="torch")
    rows = np.stack([w * ~m, w * m]).astype(np.float32)
    ref = WS.scaling(_predictions(value, type_, size, X), y, rows)
    for p, what in ((prob, "problem on the device"), (twin, "its torch twin")):
        loss, slope, icpt = p.scaled_fitness(forest)
        both = np.stack([loss.cpu().numpy(), p.last_validation_loss.cpu().numpy()], axis=1)
        assert WS.check_against(ref, both, icpt.cpu().numpy(), slope.cpu().numpy(), D, what=what) <= 0.10
    assert np.isfinite(ref["loss"]).all(axis=1).sum() >= pop // 4
    # scores is the scrubbed column 0, validation_scores the scrubbed column 1, both columns of ONE call of the op
    direct, coef = torch.ops.evogp_hip.tree_SR_weighted_scaling(pop, D, 64, 3, 1, *forest._tensors(), Xd, yd, torch.from_numpy(rows).cuda())
    sc = prob.scores(forest)
    vs = prob.validation_scores(forest, sc)
    ninf = torch.full_like(sc, float("-inf"))
    assert torch.equal(sc, torch.where(torch.isnan(direct[:, 0]), ninf, -direct[:, 0]))
    assert torch.equal(vs, torch.where((sc == float("-inf")) | torch.isnan(direct[:, 1]), ninf, -direct[:, 1]))
    # three generations of the pipeline: the validation tree is reported with its train-fitted coefficients written in
    d = GenerateDescriptor(max_tree_len=32, input_len=3, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=4,
                           const_samples=[-1, 0, 1])
    algo = GeneticProgramming(Forest.random_generate(200, d, keys=torch.tensor([1, 2], dtype=torch.uint32, device="cuda")),
                              DefaultCrossover(), DefaultMutation(0.2, d), DefaultSelection(0.3, 2))
    pipe = StandardPipeline(algo, SymbolicRegression(**opts), generation_limit=3, is_show_details=False)
    best = pipe.run()
    assert best is pipe.best_tree and best.node_value.shape == (36,) and pipe.best_validation_tree.node_value.shape == (36,)
    assert np.isfinite(float(pipe.best_fitness)) and np.isfinite(float(pipe.best_validation_fitness))
    # the reported validation tree IS the model: its plain weighted MSE on the held-out rows is the stated validation loss, up to the
    # float32 evaluation of b p + a inside the tree (linear_scaling_ref.refit_bound) and the float32 rounding of the two losses
    tree = pipe.best_validation_tree
    one = Forest(3, 1, *(x[None].contiguous() for x in (tree.node_value, tree.node_type, tree.subtree_size)))
    mse = float(one.SR_weighted_loss(Xd, yd, torch.from_numpy(rows[1]).cuda(), "mse")[0])
    stated = -float(pipe.best_validation_fitness)
    Pw = one.batch_forward(Xd)[:, :, 0].cpu().numpy().astype(np.float64)   # = fl(fl(p b) + a): bounds max |b p| + |a| within 2^-22
    bound = 2.0 * np.sqrt(stated) * 2.0 ** -21 * np.abs(Pw).max() + (2.0 ** -21 * np.abs(Pw).max()) ** 2 + 2e-6 * stated
    print(f"pipeline: validation loss stated {stated:.6g}, of the reported tree {mse:.6g}, bound {bound:.3g}")
    assert abs(mse - stated) <= bound
