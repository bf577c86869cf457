"""GPU: linear scaling (csrc/sr_scale.hip) against the numpy restatement (tests/linear_scaling_ref.py) on the device's own
batch_forward predictions and on the C oracle's, the exact rules, the rewrite kernel bit for bit, and the problem / pipeline on the
device."""
import os
import sys

import numpy as np
import pytest
import torch

import evogp_amd  # noqa: F401  (registers the ops)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import linear_scaling_ref as LS  # noqa: E402
import sr_grad_ref as R  # noqa: E402
from grad_trees import ALL_FUNCS, ARITH, random_forest  # noqa: E402
from test_gpu_subtree import _malform  # noqa: E402

from evogp_amd.tree import Forest  # noqa: E402

pytestmark = pytest.mark.gpu

B, V, C = R.T_BFUNC, R.T_VAR, R.T_CONST
TILE = 1024   # rows per workgroup tile of sr_scale_kernel: 64 lanes x 4 rows x 4 waves


def _dev(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _plant(value, type_, size, t, nodes):
    value[t], type_[t], size[t] = 0, 0, 0
    for i, (v, ty, s) in enumerate(nodes):
        value[t, i], type_[t, i], size[t, i] = v, ty, s


def _chain(rng, n_ops, var_len, funcs=(R.F_ADD, R.F_SUB, R.F_MUL)):
    """a left-nested chain of n_ops binary functions: its operand stack is n_ops + 1 high"""
    nodes = [(float(rng.choice(funcs)), B, 2 * (n_ops - k) + 1) for k in range(n_ops)]
    for _ in range(n_ops + 1):
        nodes.append((float(rng.integers(var_len)), V, 1) if rng.random() < 0.6 else (np.float32(rng.uniform(0.5, 1.5)), C, 1))
    return nodes


def _case(rng, funcs, gp_len, var_len, pop, D):
    fs = {"arith": ARITH, "all": ALL_FUNCS, "exact": [R.F_ADD, R.F_SUB, R.F_MUL]}[funcs]
    value, type_, size = random_forest(rng, pop, gp_len, fs, var_len, 1, max_depth=7 if gp_len > 64 else 5)
    # trees too deep for the 16-entry register stack: the scratch-stack kernel
    for k, t in enumerate(range(2, pop, 7)):
        ops = (20 if gp_len == 64 else (20, 100, 400)[k % 3])
        _plant(value, type_, size, t, _chain(rng, ops, var_len, (R.F_ADD, R.F_SUB, R.F_MUL) if funcs != "arith" else ARITH))
    X = rng.uniform(0.5, 1.5, (D, var_len)).astype(np.float32)
    y = (1.5 * X[:, 0] ** 2 - X[:, -1] + 0.3).astype(np.float32)[:, None]
    return value, type_, size, X, y


def _scaled(value, type_, size, X, y):
    v, t, s, Xd, yd = _dev(value, type_, size, X, y)
    pop, L = value.shape
    loss, coef = torch.ops.evogp_hip.tree_SR_linear_scaling(pop, X.shape[0], L, X.shape[1], 1, v, t, s, Xd, yd)
    coef = coef.cpu().numpy()
    return loss.cpu().numpy(), coef[:, 0].copy(), coef[:, 1].copy()


def _predictions(value, type_, size, X):
    v, t, s, Xd = _dev(value, type_, size, X)
    pop, L = value.shape
    return torch.ops.evogp_hip.tree_batch_evaluate(pop, X.shape[0], L, X.shape[1], 1, v, t, s, Xd)[:, :, 0].cpu().numpy()


# Every value the issue lists, D below, at and above the rows-per-workgroup tile, and var_len on both sides of the kernel's own
# thresholds: <= 12 and 13..32 are the two register-tuple widths of sr_scale_kernel (each in a LEAN and a FULL build: 'arith' trees
# stay in the LEAN one, 'all' forests send their transcendental trees to the FULL one, the planted chains go on to the scratch
# stack), > 32 runs on the scratch-stack kernel alone.
CASES = [
    ("arith", 64, 3, 24, 1), ("all", 64, 1, 257, 2), ("arith", 1024, 3, 24, 63), ("all", 64, 40, 24, 64), ("all", 1024, 3, 257, 65),
    ("arith", 64, 1, 1, 5000), ("all", 1024, 40, 24, 5000), ("all", 64, 3, 257, TILE - 1), ("arith", 64, 3, 257, TILE),
    ("all", 1024, 1, 24, TILE + 1), ("all", 64, 3, 1, 64), ("arith", 1024, 40, 1, 65), ("all", 64, 3, 24, 5000),
    ("all", 64, 12, 257, 300), ("all", 64, 13, 257, TILE - 1), ("all", 1024, 13, 24, TILE + 1), ("arith", 64, 13, 257, 65),
    ("all", 64, 32, 257, TILE + 1), ("all", 1024, 32, 24, TILE), ("arith", 1024, 32, 24, 5000), ("all", 64, 33, 24, 300),
]


# ---- 1. against the reference on the device's own predictions ------------------------------------------------------------------------
@pytest.mark.parametrize("funcs,gp_len,var_len,pop,D", CASES)
def test_matches_reference_on_batch_forward_predictions(rng, funcs, gp_len, var_len, pop, D):
    value, type_, size, X, y = _case(rng, funcs, gp_len, var_len, pop, D)
    loss, a, b = _scaled(value, type_, size, X, y)
    # The reference works on batch_forward's predictions, so the library functions' ulps cancel out of the comparison; that the
    # kernel's own predictions are those bits is implied by the tolerance (a tree evaluated differently by an ulp on one row moves
    # b by about 2^-24 / sqrt(D), far outside 1e-6 + kappa D 2^-52 only when it is wrong by much more than an ulp -- and a NaN / inf
    # row that only one of the two sees shows in the NaN masks).
    ref = LS.scaling(_predictions(value, type_, size, X), y)
    excluded = LS.check_against(ref, loss, a, b, D, what=f"{funcs} L{gp_len} v{var_len} pop{pop} D{D}")
    assert excluded <= 0.10
    assert pop < 24 or np.isfinite(ref["loss"]).sum() >= pop // 4


# ---- 2. against the C oracle's predictions (+ - *: bit-exact evaluation) -----------------------------------------------------------------
@pytest.mark.parametrize("gp_len,var_len,D", [(64, 3, 300), (1024, 3, 1500), (64, 40, 70), (64, 13, 1100), (1024, 32, 300)])
def test_matches_reference_on_oracle_predictions(rng, oracle, gp_len, var_len, D):
    value, type_, size, X, y = _case(rng, "exact", gp_len, var_len, 100, D)
    loss, a, b = _scaled(value, type_, size, X, y)
    P = oracle.batch_evaluate(value, type_, size, X, 1)[:, :, 0]
    assert np.array_equal(_bits(P), _bits(_predictions(value, type_, size, X)))
    ref = LS.scaling(P, y)
    assert LS.check_against(ref, loss, a, b, D, what=f"oracle L{gp_len} v{var_len} D{D}") <= 0.10


# ---- 3. the exact rules ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,var_len", [(1, 3), (300, 3), (TILE + 7, 3), (300, 40), (300, 13), (TILE + 7, 32), (1, 32)])
def test_exact_rules_and_determinism(rng, D, var_len):
    value, type_, size, X, y = _case(rng, "all", 64, var_len, 40, D)
    bad = _malform(value, type_, size)
    _plant(value, type_, size, 0, [(0.75, C, 1)])                                      # a CONST tree
    _plant(value, type_, size, 1, [(R.F_SUB, B, 3), (0, V, 1), (0, V, 1)])             # x0 - x0
    # 1 / (x0 - c) with c = the x0 of ONE row: a division by zero on that row
    _plant(value, type_, size, 3, [(R.F_DIV, B, 5), (1.0, C, 1), (R.F_SUB, B, 3), (0, V, 1), (X[D // 2, 0], C, 1)])
    loss, a, b = _scaled(value, type_, size, X, y)
    y64 = y.astype(np.float64).reshape(-1)
    ybar, syy_D = y64.mean(), np.var(y64)
    # float64 sums in another order agree to ~D 2^-53: the float32 roundings coincide unless the value sits on a rounding boundary
    for x in (ybar, syy_D):
        assert np.float32(x * (1 - 1e-12)) == np.float32(x * (1 + 1e-12)), "the fixture's label statistics sit on a float32 rounding boundary"
    for t in (0, 1):
        assert b[t] == 0 and _bits(a[t]) == _bits(np.float32(ybar)) and _bits(loss[t]) == _bits(np.float32(syy_D)), (t, loss[t], a[t], b[t])
    for t in bad + (3,):
        assert np.isnan(loss[t]) and np.isnan(a[t]) and np.isnan(b[t]), t
    assert np.isfinite(loss).sum() >= 10
    if D == 1:   # one row: every finite tree is constant
        ok = np.isfinite(loss)
        assert np.all(b[ok] == 0) and np.all(_bits(a[ok]) == _bits(np.float32(ybar))) and np.all(loss[ok] == 0)
    # two calls give equal bits, and dedup=True the bits of the plain call
    again = _scaled(value, type_, size, X, y)
    for g, w in zip(again, (loss, a, b)):
        assert np.array_equal(_bits(g), _bits(w))
    value2, type2, size2 = (np.concatenate([x, x[:17]]) for x in (value, type_, size))
    forest = Forest(var_len, 1, *_dev(value2, type2, size2))
    Xd, yd = _dev(X, y)
    plain = [x.cpu().numpy() for x in forest.SR_scaled_fitness(Xd, yd)]
    dedup = [x.cpu().numpy() for x in forest.SR_scaled_fitness(Xd, yd, dedup=True)]
    for g, w in zip(dedup, plain):
        assert np.array_equal(_bits(g), _bits(w))
    assert np.array_equal(_bits(plain[0][:40]), _bits(loss)) and np.array_equal(_bits(plain[1][:40]), _bits(b))
    assert np.array_equal(_bits(plain[0][40:]), _bits(loss[:17]))


def test_graph_capture_replays_the_call(rng):
    value, type_, size, X, y = _case(rng, "arith", 64, 3, 200, 300)
    v, t, s, Xd, yd = _dev(value, type_, size, X, y)
    args = (200, 300, 64, 3, 1, v, t, s, Xd, yd)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        eager = torch.ops.evogp_hip.tree_SR_linear_scaling(*args)   # (the stream's counter ring is made outside the capture)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            out = torch.ops.evogp_hip.tree_SR_linear_scaling(*args)
        for _ in range(2):
            out[0].fill_(7.0)
            g.replay()
            side.synchronize()
            assert np.array_equal(_bits(out[0].cpu().numpy()), _bits(eager[0].cpu().numpy()))
            assert np.array_equal(_bits(out[1].cpu().numpy()), _bits(eager[1].cpu().numpy()))


# ---- 4. the rewrite kernel --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gp_len,grow", [(64, False), (64, True), (1024, False), (1024, True), (1020, True)])
def test_wrap_kernel_bit_for_bit(rng, oracle, gp_len, grow):
    pop = 60
    value, type_, size = random_forest(rng, pop, gp_len, ALL_FUNCS, 3, 1, max_depth=5)
    bad = _malform(value, type_, size)
    _plant(value, type_, size, 5, _chain(rng, (gp_len - 1) // 2, 3))            # a full row: fits only a grown one
    _plant(value, type_, size, 6, _chain(rng, (gp_len - 5) // 2, 3))            # len + 4 == gp_len (even gp_len: len = gp_len - 5 or - 4)
    value[8, 40:] = 3.5                                                         # tail words of the input are not copied into a wrapped row
    coef = rng.normal(0, 2, (pop, 2)).astype(np.float32)
    coef[13] = [np.nan, 1.0]
    coef[14] = [1.0, np.inf]
    coef[15] = [0.0, -0.0]
    out_len = min(gp_len + 4, 1024) if grow else gp_len
    want = LS.wrap_rows(value, type_, size, coef, out_len)
    v, t, s, cd = _dev(value, type_, size, coef)
    got = [x.cpu().numpy() for x in torch.ops.evogp_hip.tree_wrap_linear(out_len, v, t, s, cd)]
    assert got[0].shape == (pop, out_len) and got[3].dtype == np.uint8
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert np.array_equal(got[3], want[3])
    assert not got[3][list(bad) + [13, 14]].any() and got[3][6] == 1
    assert got[3][5] == (1 if grow and gp_len <= 1020 else 0)
    for r in np.flatnonzero(got[3]):
        assert oracle.validate_tree(got[1][r], got[2][r]) == 0, r
    # Forest.apply_scaling is this op, with the mask rule
    forest = Forest(3, 1, v, t, s, func_mask=(1 << 29) - 1)
    f2, applied = forest.apply_scaling(cd[:, 1].clone(), cd[:, 0].clone(), grow=grow)
    assert f2.max_tree_len == out_len and torch.equal(applied.cpu(), torch.from_numpy(want[3]).bool()) and f2.func_mask == (1 << 29) - 1
    assert np.array_equal(_bits(f2.batch_node_value.cpu().numpy()), _bits(want[0]))


# ---- 5. / 6. the wrapped tree is the scaled model; scaling a scaled tree changes nothing ------------------------------------------------
@pytest.fixture(scope="module")
def fitted():
    rng = np.random.default_rng(20261018)
    D = 48
    value, type_, size, X, y = _case(rng, "arith", 64, 3, 300, D)
    forest = Forest(3, 1, *_dev(value, type_, size))
    Xd, yd = _dev(X, y)
    loss, slope, intercept = forest.SR_scaled_fitness(Xd, yd)
    P = forest.batch_forward(Xd)[:, :, 0].cpu().numpy()
    return dict(forest=forest, X=Xd, y=yd, y_np=y, D=D, loss=loss, slope=slope, intercept=intercept, P=P, ref=LS.scaling(P, y))


def test_plain_fitness_of_the_wrapped_forest_is_the_scaled_loss(fitted):
    f = fitted
    wrapped, applied = f["forest"].apply_scaling(f["slope"], f["intercept"], grow=True)
    ok = applied.cpu().numpy()
    loss, a, b = (x.cpu().numpy().astype(np.float64) for x in (f["loss"], f["intercept"], f["slope"]))
    assert np.array_equal(ok, np.isfinite(loss)) and ok.sum() >= 100
    mse = wrapped.SR_fitness(f["X"], f["y"]).cpu().numpy().astype(np.float64)
    bound = LS.refit_bound(f["P"], a, b, loss)
    off = np.abs(mse - loss)
    print(f"wrapped forest: {ok.sum()} trees, worst |SR_fitness - scaled loss| / bound {np.max(off[ok] / bound[ok]):.3g}, "
          f"median {np.median(off[ok] / bound[ok]):.3g}")
    worst = np.flatnonzero(ok & ~(off <= bound))
    assert worst.size == 0, (worst[:5], mse[worst[:5]], loss[worst[:5]], bound[worst[:5]])


def test_scaled_loss_is_invariant_under_an_affine_map_of_the_tree(fitted):
    f = fitted
    rng = np.random.default_rng(7)
    ref, D, pop = f["ref"], f["D"], f["P"].shape[0]
    P64 = f["P"].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        mean, msq = P64.mean(1), (P64 * P64).mean(1)
    b0 = (rng.uniform(0.5, 2.0, pop) * rng.choice([-1.0, 1.0], pop)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        a0 = np.nan_to_num(0.1 * np.sqrt(msq) * rng.choice([-1.0, 1.0], pop), nan=1.0, posinf=1.0).astype(np.float32)
    forest2, applied = f["forest"].apply_scaling(torch.from_numpy(b0).cuda(), torch.from_numpy(a0).cuda(), grow=True)
    assert bool(applied.all())
    loss2, _, _ = forest2.SR_scaled_fitness(f["X"], f["y"])
    loss2 = loss2.cpu().numpy().astype(np.float64)
    ref2 = LS.scaling(forest2.batch_forward(f["X"])[:, :, 0].cpu().numpy(), f["y_np"])
    # kappa' / kappa = 1 + (2 a0 b0 mean + a0^2) / (b0^2 msq): with |a0| = 0.1 sqrt(msq) and |b0| >= 0.5 within [0.56, 1.44]
    with np.errstate(invalid="ignore", divide="ignore"):
        predicted = 1 + (2 * a0 * b0 * mean + a0.astype(np.float64) ** 2) / (b0.astype(np.float64) ** 2 * msq)
        pick = np.isfinite(ref["loss"]) & (ref["kappa"] > 0) & (ref["kappa"] < 1e8) & (predicted > 0.55) & (predicted < 1.45)
        ratio = ref2["kappa"] / ref["kappa"]
    assert pick.sum() >= 100
    assert np.all((ratio[pick] >= 0.5) & (ratio[pick] <= 2.0)), (ratio[pick].min(), ratio[pick].max())
    loss1 = f["loss"].cpu().numpy().astype(np.float64)
    r1, at = LS.tolerance(ref["kappa"], D, ref["syy_D"])
    r2, _ = LS.tolerance(ref2["kappa"], D, ref2["syy_D"])
    tol = r1 * np.abs(ref["loss"]) + r2 * np.abs(ref2["loss"]) + 2 * at
    off = np.abs(loss2 - loss1)
    print(f"invariance: {pick.sum()} trees, worst |loss2 - loss1| / tol {np.max(off[pick] / tol[pick]):.3g}, median {np.median(off[pick] / tol[pick]):.3g}")
    worst = np.flatnonzero(pick & ~(off <= tol))
    assert worst.size == 0, (worst[:5], loss1[worst[:5]], loss2[worst[:5]], tol[worst[:5]], ref["kappa"][worst[:5]])


# ---- 7. problem and pipeline ----------------------------------------------------------------------------------------------------------
def test_problem_scores_and_pipeline(fitted):
    from evogp_amd.algorithm import DefaultCrossover, DefaultMutation, DefaultSelection, GeneticProgramming
    from evogp_amd.pipeline import StandardPipeline
    from evogp_amd.problem import SymbolicRegression
    from evogp_amd.tree import GenerateDescriptor

    f = fitted
    prob = SymbolicRegression(datapoints=f["X"], labels=f["y"], linear_scaling=True)
    want = torch.where(torch.isnan(f["loss"]), torch.full_like(f["loss"], float("-inf")), -f["loss"])
    assert np.array_equal(_bits(prob.scores(f["forest"]).cpu().numpy()), _bits(want.cpu().numpy()))
    assert np.array_equal(_bits(prob.evaluate(f["forest"]).cpu().numpy()), _bits((-f["loss"]).cpu().numpy()))
    tprob = SymbolicRegression(datapoints=f["X"], labels=f["y"], linear_scaling=True, execute_mode="torch")
    tl, tb, ta = (x.cpu().numpy() for x in tprob.scaled_fitness(f["forest"]))
    LS.check_against(f["ref"], tl, ta, tb, f["D"], what="torch mode")

    d = GenerateDescriptor(max_tree_len=64, input_len=3, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=5,
                           const_samples=[-1, 0, 1])
    algo = GeneticProgramming(Forest.random_generate(512, d, keys=torch.tensor([3, 4], dtype=torch.uint32, device="cuda")), DefaultCrossover(),
                              DefaultMutation(0.2, d), DefaultSelection(0.3, 2))
    pipe = StandardPipeline(algo, prob, generation_limit=3, is_show_details=False)
    best = pipe.run()
    assert best.node_value.shape == (68,) and np.isfinite(float(pipe.best_fitness))
    one = Forest(3, 1, best.node_value[None].contiguous(), best.node_type[None].contiguous(), best.subtree_size[None].contiguous())
    mse = float(one.SR_fitness(f["X"], f["y"])[0])
    n = int(best.subtree_size[0]) - 4   # the tree inside the wrapper: words 2 .. n + 1
    inner = Forest(3, 1, *(torch.zeros(1, 64, dtype=x.dtype, device="cuda") for x in one._tensors()))
    for dst, src in zip(inner._tensors(), one._tensors()):
        dst[0, :n] = src[0, 2:n + 2]
    pred = inner.batch_forward(f["X"])[:, :, 0].cpu().numpy()
    a, b = float(best.node_value[n + 3]), float(best.node_value[n + 2])
    loss = -float(pipe.best_fitness)
    bound = LS.refit_bound(pred, np.array([a]), np.array([b]), np.array([loss]))[0]
    print(f"pipeline best: fitness {-loss:.6g}, plain MSE of best_tree {mse:.6g}, bound {bound:.3g}")
    assert abs(mse - loss) <= bound
