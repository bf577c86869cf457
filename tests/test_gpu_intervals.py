"""GPU: the interval kernel (csrc/sr_interval.hip) against the numpy restatement (tests/interval_ref.py) -- bit for bit where no library
function is involved, by containment and in ulps where one is -- and against the device's own evaluations: every value batch_forward
and SR_fitness compute inside the box obeys the claim, with no tolerance."""
import os
import sys

import numpy as np
import pytest
import torch

import evogp_amd  # noqa: F401  (registers the ops)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import interval_cases as IC  # noqa: E402
import interval_ref as IR  # noqa: E402
import sr_grad_ref as R  # noqa: E402
from grad_trees import ALL_FUNCS, random_forest  # noqa: E402

from evogp_amd.problem import SymbolicRegression  # noqa: E402
from evogp_amd.tree import Forest  # noqa: E402

pytestmark = pytest.mark.gpu

DIVISIONS = (R.F_DIV, R.F_LOOSE_DIV, R.F_INV, R.F_LOOSE_INV)


def _dev(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _box(k, var_len):
    """box k of the three, its three columns repeated over var_len variables"""
    lower, upper = IC.BOXES[k]
    idx = np.arange(var_len) % 3
    return lower[idx].copy(), upper[idx].copy()


def _kernel(value, type_, size, lower, upper):
    out = torch.ops.evogp_hip.tree_intervals(*_dev(value, type_, size, lower, upper))
    return [o.cpu().numpy() for o in out]


def _same_bits(got, want, what):
    for name, g, w in zip(("lo", "hi", "flags"), got, want):
        gb, wb = (g.view(np.uint32), w.view(np.uint32)) if g.dtype == np.float32 else (g, w)
        bad = np.argwhere(gb != wb)
        assert len(bad) == 0, f"{what}: {name} differs at (tree, node) {bad[:5].tolist()}: {g[tuple(bad[0])]!r} != {w[tuple(bad[0])]!r}"


def _exact_forest(rng, pop, L, var_len):
    value, type_, size = IC.random_exact_forest(rng, pop, L, var_len, full_rows=min(3, pop) if pop > 1 else 0)
    plant = []
    if L >= 8 and pop >= 24:
        # unknown ids (the interpreters yield 0), and malformed rows: a broken stack discipline, a live prefix that is not one tree,
        # a size word that is not its subtree's size, an empty row, a length beyond the row
        plant += [IC.U(5, IC.V(0)), IC.B(20, IC.V(0), IC.C(np.nan)), IC.B(77, IC.C(1.0), IC.V(0)), IC.U(R.F_NEG, IC.U(40, IC.V(0)))]
        for k, e in enumerate(plant):
            value[4 + k], type_[4 + k], size[4 + k] = IC.rows([e], L)
        bad = IC.rows([IC.B(R.F_ADD, IC.B(R.F_MUL, IC.V(0), IC.C(2.0)), IC.V(0))] * 5, L)
        bad[1][0, 4] = 3
        bad[2][1, 0] = 3
        bad[2][2, 1] = 2
        bad[2][3, 0] = 0
        bad[2][4, 0] = L + 5
        for k in range(5):
            value[10 + k], type_[10 + k], size[10 + k] = bad[0][k], bad[1][k], bad[2][k]
    if L == 1024:
        # chains 401 operands deep, left- and right-leaning: the walk has no operand stack to overflow
        chains = [IC.chain(R.F_SUB, 401, True), IC.chain(R.F_DIV, 401, False), IC.chain(R.F_MUL, 401, True), IC.chain(R.F_MAX, 401, False)]
        for k, nodes in enumerate(chains):
            value[16 + k], type_[16 + k], size[16 + k] = IC.rows([nodes], L)
    return value, type_, size


@pytest.mark.parametrize("box", range(3))
@pytest.mark.parametrize("pop,L,var_len", [(1, 8, 1), (24, 64, 3), (24, 1024, 3), (257, 64, 40), (257, 8, 3)])
def test_exact_tier_bit_for_bit(pop, L, var_len, box, rng):
    """(a) rules 1-3 and 7: lo, hi and flags equal the restatement bit for bit on every node"""
    value, type_, size = _exact_forest(rng, pop, L, var_len)
    lower, upper = _box(box, var_len)
    got = _kernel(value, type_, size, lower, upper)
    want = IR.forest_intervals(value, type_, size, lower, upper)
    _same_bits(got, want, f"pop {pop} L {L} var_len {var_len} box {box}")
    if pop >= 24 and L >= 8:
        assert (got[2][10:15, 0] == 3).all() and np.isnan(got[0][10:15, 0]).all()
        assert (got[2][4:8, 0] == 0).all() and not got[0][4:8, 0].any()


def _has_division(value, type_, size):
    """(pop, L) bool: the subtree rooted at the node holds a division (the node itself included)"""
    pop, L = value.shape
    is_div = (type_ >= 2) & np.isin(value.astype(np.int64), DIVISIONS) & ((type_ == 2) | (type_ == 3))
    out = np.zeros((pop, L), bool)
    for t in range(pop):
        for i in range(int(size[t, 0])):
            out[t, i] = is_div[t, i:i + int(size[t, i])].any()
    return out


@pytest.mark.parametrize("box", range(3))
def test_library_tier_contains_the_exact_intervals(box, rng):
    """(b) all 29 functions: the kernel's interval of every node contains the interval the restatement computes from float64-exact
    endpoint values (no library widening: the device's value at an endpoint lies within E(f) ulps of the exact one and the kernel
    moves it W(f) = 2 E(f) + 1 outward, and every rule is inclusion-monotone in its operands' intervals); where no division is
    involved the flags agree with the restatement's (float64 endpoints, widened)"""
    value, type_, size = random_forest(rng, 96, 64, ALL_FUNCS, 3, 1, max_depth=5, const_range=(-2.0, 2.0))
    lower, upper = IC.BOXES[box]
    lo, hi, fl = _kernel(value, type_, size, lower, upper)
    elo, ehi, efl = IR.forest_intervals(value, type_, size, lower, upper, lib="float64", widen=False)
    live = np.arange(64)[None, :] < size[:, :1]
    assert not (fl & IR.MALFORMED).any()
    bad = np.argwhere(live & ~((lo <= elo) & (hi >= ehi) & ((fl & efl) == efl)))
    assert len(bad) == 0, [(t, i, lo[t, i], elo[t, i], ehi[t, i], hi[t, i], fl[t, i], efl[t, i]) for t, i in bad[:4]]
    wfl = IR.forest_intervals(value, type_, size, lower, upper, lib="float64", widen=True)[2]
    cmp = live & ~_has_division(value, type_, size)
    bad = np.argwhere(cmp & (fl != wfl))
    assert cmp.sum() > 300 and len(bad) == 0, [(t, i, fl[t, i], wfl[t, i]) for t, i in bad[:4]]
    assert not lo[~live].any() and not hi[~live].any() and not fl[~live].any()


def test_library_tier_single_operations():
    """(b) single-operation trees: the kernel's bounds lie within W(f) ulps of the restatement's (float64 endpoints, widened alike): the
    two differ by the device's error at the endpoint, at most E(f) < W(f)"""
    exprs = [IC.single_op(f) for f in IC.ALL]
    value, type_, size = IC.rows(exprs, 8)
    boxes = IC.BOXES + [(np.array([0.5, 0.25, 1.5], np.float32), np.array([2.0, 3.0, 1.5], np.float32)),
                        (np.array([-3.0, -2.0, -1.0], np.float32), np.array([-0.5, 2.5, 4.0], np.float32))]
    for lower, upper in boxes:
        lo, hi, fl = _kernel(value, type_, size, lower, upper)
        wlo, whi, wfl = IR.forest_intervals(value, type_, size, lower, upper, lib="float64", widen=True)
        for r, f in enumerate(IC.ALL):
            w = IR.widening(f) if f in IR.W_ULPS else 0
            dlo = abs(int(IC.ulp_key(lo[r, 0]) - IC.ulp_key(wlo[r, 0])))
            dhi = abs(int(IC.ulp_key(hi[r, 0]) - IC.ulp_key(whi[r, 0])))
            print(f"f {f:2d} box [{lower[0]:g}, {upper[0]:g}]: lo off by {dlo} ulps, hi off by {dhi} ulps (W = {w})")
            assert dlo <= w and dhi <= w and fl[r, 0] == wfl[r, 0], (f, lower, upper, lo[r, 0], wlo[r, 0], hi[r, 0], whi[r, 0])


@pytest.fixture(scope="module")
def fuzz_forest(oracle):
    """64 random trees over all 29 functions with NaN / +-inf constants planted, and every subtree of them as a row of its own"""
    rng = np.random.default_rng(20261018)
    value, type_, size = IC.oracle_forest(oracle, rng, 64, IC.ALL, key=7)
    sv, st, ss, where = IC.all_subtree_rows(value, type_, size)
    return (value, type_, size), (sv, st, ss), where


@pytest.mark.parametrize("box", range(3))
def test_soundness_on_the_device(box, fuzz_forest, rng):
    """(c) every subtree as a row of its own, evaluated by batch_forward on 256 points of the box: every value obeys the claim"""
    (value, type_, size), (sv, st, ss), where = fuzz_forest
    lower, upper = IC.BOXES[box]
    lo, hi, fl = _kernel(value, type_, size, lower, upper)
    assert not (fl & IR.MALFORMED).any()
    X = IC.sample_points(rng, lower, upper)
    rows = Forest(3, 1, *_dev(sv, st, ss))
    vals = rows.batch_forward(torch.from_numpy(X).cuda())[:, :, 0].cpu().numpy()
    bad = [(int(a), int(b)) for k, (a, b) in enumerate(where) if not IR.obeys_claim(vals[k], lo[a, b], hi[a, b], fl[a, b])]
    assert len(where) > 400 and not bad, [(a, b, lo[a, b], hi[a, b], fl[a, b]) for a, b in bad[:5]]


@pytest.mark.parametrize("funcs", ["arith", "all"])
def test_safe_trees_have_a_finite_fitness(funcs, oracle, rng):
    """(d) the claim on SR_fitness's path: a tree that is safe on the dataset's box with |value| <= 1e15 has a finite MSE on the 256
    points (every squared error is below (1e15 + |y|)^2 < 1e31, so neither a term nor the sum can overflow)"""
    value, type_, size = IC.oracle_forest(oracle, rng, 256, IC.ARITH if funcs == "arith" else IC.ALL, key=11, plant=0.05)
    lower, upper = IC.BOXES[0]
    X = IC.sample_points(rng, lower, upper)
    y = (X[:, :1] * X[:, 1:2] - X[:, 2:3]).astype(np.float32)
    forest = Forest(3, 1, *_dev(value, type_, size))
    Xd, yd = _dev(X, y)
    mask = forest.safe_mask(Xd.min(0).values, Xd.max(0).values, max_abs=1e15).cpu().numpy()
    fit = forest.SR_fitness(Xd, yd).cpu().numpy()
    assert 10 < mask.sum() < 256 and np.isfinite(fit[mask]).all(), np.argwhere(mask & ~np.isfinite(fit))[:5]


def test_deterministic_and_graph_replay(rng):
    """(e) two calls and a graph replay give the same bits"""
    value, type_, size = random_forest(rng, 300, 64, ALL_FUNCS, 3, 1, max_depth=5, const_range=(-2.0, 2.0))
    args = _dev(value, type_, size, *IC.BOXES[0])
    first = [o.cpu().numpy() for o in torch.ops.evogp_hip.tree_intervals(*args)]
    second = [o.cpu().numpy() for o in torch.ops.evogp_hip.tree_intervals(*args)]
    _same_bits(second, first, "second call")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        torch.ops.evogp_hip.tree_intervals(*args)      # warm-up outside the capture
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            out = torch.ops.evogp_hip.tree_intervals(*args)
    torch.cuda.current_stream().wait_stream(side)
    for k in range(2):
        for o in out:
            o.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        _same_bits([o.cpu().numpy() for o in out], first, f"replay {k}")


@pytest.mark.parametrize("scaling", [False, True])
def test_problem_masks_unsafe_trees(scaling, oracle, rng):
    """(f) SymbolicRegression(interval_check=True) on the device: unsafe trees score -inf, safe trees exactly what they score without"""
    value, type_, size = IC.oracle_forest(oracle, rng, 200, IC.ARITH, key=13, plant=0.0)
    X = rng.uniform(-1, 1, (64, 3)).astype(np.float32)
    y = (X[:, :1] * X[:, 1:2] - X[:, 2:3]).astype(np.float32)
    Xd, yd = _dev(X, y)
    forest = Forest(3, 1, *_dev(value, type_, size))
    plain = SymbolicRegression(datapoints=Xd, labels=yd, linear_scaling=scaling)
    prob = SymbolicRegression(datapoints=Xd, labels=yd, linear_scaling=scaling, interval_check=True, input_margin=0.1)
    mask = prob.safe_mask(forest)
    ref = IR.safe(*IR.forest_intervals(value, type_, size, prob.input_lower.numpy(), prob.input_upper.numpy()))
    assert np.array_equal(mask.cpu().numpy(), ref) and 0 < ref.sum() < 200
    sc0, sc, ev0, ev = plain.scores(forest), prob.scores(forest), plain.evaluate(forest), prob.evaluate(forest)
    assert torch.equal(sc[mask], sc0[mask]) and (sc[~mask] == float("-inf")).all()
    assert torch.equal(ev[mask].view(torch.int32), ev0[mask].view(torch.int32)) and torch.isnan(ev[~mask]).all()
    assert torch.isfinite(sc0[~mask]).any()      # trees the rows alone would have let through
