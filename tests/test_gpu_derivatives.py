"""GPU: the derivative-bound kernels (csrc/sr_deriv.hip) against the numpy restatement (tests/derivative_ref.py) -- bit for bit where no
library function is involved, by containment where one is -- against the interval kernel they share their rules with, and against the
device's own evaluations: trees the mask accepts are monotone under batch_forward."""
import os
import sys

import numpy as np
import pytest
import torch

import evogp_amd  # noqa: F401  (registers the ops)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import derivative_ref as DR  # noqa: E402
import interval_cases as IC  # noqa: E402
import interval_ref as IR  # noqa: E402
import sr_grad_ref as R  # noqa: E402
from grad_trees import ALL_FUNCS, random_forest  # noqa: E402

from evogp_amd.problem import SymbolicRegression  # noqa: E402
from evogp_amd.tree import Forest  # noqa: E402

pytestmark = pytest.mark.gpu

DIVISIONS = (R.F_DIV, R.F_LOOSE_DIV, R.F_INV, R.F_LOOSE_INV)
NAMES = ("vlo", "vhi", "vflags", "dlo", "dhi", "dflags")


def _dev(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _box(k, var_len):
    """box k of the three, its three columns repeated over var_len variables"""
    lower, upper = IC.BOXES[k]
    idx = np.arange(var_len) % 3
    return lower[idx].copy(), upper[idx].copy()


def _kernel(value, type_, size, lower, upper, wrt):
    out = torch.ops.evogp_hip.tree_derivative_intervals(*_dev(value, type_, size, lower, upper, np.asarray(wrt, np.int32)))
    return [o.cpu().numpy() for o in out]


def _same_bits(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape)
        gb, wb = (g.view(np.uint32), w.view(np.uint32)) if g.dtype == np.float32 else (g, w)
        bad = np.argwhere(gb != wb)
        assert len(bad) == 0, f"{what}: {name} differs at {bad[:5].tolist()}: {g[tuple(bad[0])]!r} != {w[tuple(bad[0])]!r}"


def _exact_forest(rng, pop, L, var_len):
    """the forest of test_gpu_intervals.py's exact tier: random trees over the functions without a library call, full rows, and
    planted: unknown ids, the five malformed kinds, chains 401 operands deep"""
    value, type_, size = IC.random_exact_forest(rng, pop, L, var_len, full_rows=min(3, pop) if pop > 1 else 0)
    if L >= 8 and pop >= 24:
        plant = [IC.U(5, IC.V(0)), IC.B(20, IC.V(0), IC.C(np.nan)), IC.B(77, IC.C(1.0), IC.V(0)), IC.U(R.F_NEG, IC.U(40, IC.V(0)))]
        for k, e in enumerate(plant):
            value[4 + k], type_[4 + k], size[4 + k] = IC.rows([e], L)
        bad = IC.rows([IC.B(R.F_ADD, IC.B(R.F_MUL, IC.V(0), IC.C(2.0)), IC.V(0))] * 5, L)
        bad[1][0, 4] = 3          # a broken stack discipline
        bad[2][1, 0] = 3          # a live prefix that is not one tree
        bad[2][2, 1] = 2          # a size word that is not its subtree's size
        bad[2][3, 0] = 0          # an empty row
        bad[2][4, 0] = L + 5      # a length beyond the row
        for k in range(5):
            value[10 + k], type_[10 + k], size[10 + k] = bad[0][k], bad[1][k], bad[2][k]
    if L == 1024:
        chains = [IC.chain(R.F_SUB, 401, True), IC.chain(R.F_DIV, 401, False), IC.chain(R.F_MUL, 401, True), IC.chain(R.F_MAX, 401, False)]
        for k, nodes in enumerate(chains):
            value[16 + k], type_[16 + k], size[16 + k] = IC.rows([nodes], L)
    return value, type_, size


# (pop, L, var_len of the box, var_len the trees draw from, wrt): one tree; a partial wave; rows of 1024 words with the chains; more
# than four waves with a last partial one, a variable no tree uses (39) and a repeated entry; short rows with a repeated entry
SHAPES = [(1, 8, 1, 1, [0]), (24, 64, 3, 3, [0, 2, 1]), (24, 1024, 3, 3, [1]), (257, 64, 40, 39, [39, 5, 39]), (257, 8, 3, 3, [2, 2, 0])]


@pytest.mark.parametrize("box", range(3))
@pytest.mark.parametrize("pop,L,var_len,tree_vars,wrt", SHAPES)
def test_exact_tier_bit_for_bit(pop, L, var_len, tree_vars, wrt, box, rng):
    """the functions without a library call: all six outputs equal the restatement bit for bit on every node"""
    value, type_, size = _exact_forest(rng, pop, L, tree_vars)
    lower, upper = _box(box, var_len)
    got = _kernel(value, type_, size, lower, upper, wrt)
    want = DR.forest_derivative_intervals(value, type_, size, lower, upper, wrt)
    _same_bits(got, want, f"pop {pop} L {L} var_len {var_len} box {box}")
    dfl = got[5]
    if pop >= 24 and L >= 8:
        assert (dfl[:, 10:15, 0] == IR.MALFORMED).all() and np.isnan(got[3][:, 10:15, 0]).all() and (got[2][10:15, 0] == 3).all()
        assert not dfl[:, 4:8, 0].any() and not got[3][:, 4:8, 0].any()        # unknown ids: exactly [0, 0], flags 0
    if 39 in wrt:      # no tree uses x39: every live node is exactly [0, 0] with flags 0 (malformed rows apart)
        ok = np.ones(pop, bool)
        ok[10:15] = False
        assert not got[3][0, ok].any() and not got[4][0, ok].any() and not dfl[0, ok].any()
        assert (dfl[1] & DR.DEPENDS).any()
    for a in range(len(wrt)):
        for b in range(a):
            if wrt[a] == wrt[b]:      # a repeated entry: equal slices
                assert all(np.array_equal(got[k][a].view(np.uint8), got[k][b].view(np.uint8)) for k in (3, 4, 5))


def _has_division(value, type_, size):
    """(pop, L) bool: the subtree rooted at the node holds a division (the node itself included)"""
    pop, L = value.shape
    is_div = np.isin(value.astype(np.int64), DIVISIONS) & ((type_ == 2) | (type_ == 3))
    out = np.zeros((pop, L), bool)
    for t in range(pop):
        for i in range(int(size[t, 0])):
            out[t, i] = is_div[t, i:i + int(size[t, i])].any()
    return out


@pytest.fixture(scope="module")
def library_forest():
    rng = np.random.default_rng(20261019)
    return random_forest(rng, 96, 64, ALL_FUNCS, 3, 1, max_depth=5, const_range=(-2.0, 2.0))


@pytest.mark.parametrize("box", range(3))
def test_library_tier_contains_the_exact_bounds(box, library_forest):
    """all 29 functions, 96 trees: the kernel's D of every node contains the D the restatement computes from float64-exact library values
    without the library widening (every rule is inclusion-monotone in R and in the children's D, and a wider R can only move a rule
    towards its hull or its fallback); JUMP and DEPENDS agree with the restatement's (float64 endpoints, widened) where no division
    lies below the node"""
    value, type_, size = library_forest
    lower, upper = IC.BOXES[box]
    wrt = [0, 1, 2]
    got = _kernel(value, type_, size, lower, upper, wrt)
    exact = DR.forest_derivative_intervals(value, type_, size, lower, upper, wrt, lib="float64", widen=False)
    live = np.arange(64)[None, :] < size[:, :1]
    assert not (got[2] & IR.MALFORMED).any() and not (got[5] & IR.MALFORMED).any()
    bad = np.argwhere(live & ~((got[0] <= exact[0]) & (got[1] >= exact[1])))
    assert len(bad) == 0, [(t, i, got[0][t, i], exact[0][t, i], exact[1][t, i], got[1][t, i]) for t, i in bad[:4]]
    bad = np.argwhere(live[None] & ~((got[3] <= exact[3]) & (got[4] >= exact[4])))
    assert len(bad) == 0, [(k, t, i, got[3][k, t, i], exact[3][k, t, i], exact[4][k, t, i], got[4][k, t, i]) for k, t, i in bad[:4]]
    wide = DR.forest_derivative_intervals(value, type_, size, lower, upper, wrt, lib="float64", widen=True)
    cmp = (live & ~_has_division(value, type_, size))[None]
    bad = np.argwhere(cmp & (got[5] != wide[5]))
    assert cmp.sum() > 300 and len(bad) == 0, [(k, t, i, got[5][k, t, i], wide[5][k, t, i]) for k, t, i in bad[:4]]
    for o in got[:3]:
        assert not o[~live].any()
    for o in got[3:]:
        assert not o[:, ~live].any()


@pytest.mark.parametrize("box", range(3))
def test_enclosures_contain_the_interval_kernel(box, library_forest, rng):
    """R contains what tree_intervals gives, with equal flags, on the device: all 29 functions and the exact tier with its planted rows"""
    for value, type_, size in (library_forest, _exact_forest(rng, 257, 64, 3)):
        lower, upper = IC.BOXES[box]
        lo, hi, fl = [o.cpu().numpy() for o in torch.ops.evogp_hip.tree_intervals(*_dev(value, type_, size, lower, upper))]
        vlo, vhi, vfl = _kernel(value, type_, size, lower, upper, [0])[:3]
        bad_row = (fl[:, :1] & IR.MALFORMED) != 0
        inside = (vlo <= lo) & (vhi >= hi)
        inside |= bad_row & np.isnan(vlo) & np.isnan(lo)
        bad = np.argwhere(~inside | (vfl != fl))
        assert len(bad) == 0, [(t, i, lo[t, i], hi[t, i], fl[t, i], vlo[t, i], vhi[t, i], vfl[t, i]) for t, i in bad[:4]]


MONOTONE_FUNCS = [R.F_ADD, R.F_SUB, R.F_MUL, R.F_MAX, R.F_MIN, R.F_ABS]


@pytest.mark.parametrize("box", [0, 1])
def test_accepted_trees_are_monotone_on_the_device(box, oracle, rng):
    """trees monotone_mask accepts as nondecreasing in x_v: batch_forward on 32 sorted values of x_v, the other columns fixed, is
    nondecreasing in a float64 comparison of the fp32 outputs.  RESTRICTED to trees over + - * max min abs: their fp32 evaluation is a
    composition of monotone, correctly rounded operations (and on these dyadic constants and inputs mostly an exact one), so no
    tolerance is needed; a library function's rounding error is not monotone"""
    value, type_, size = IC.oracle_forest(oracle, rng, 256, MONOTONE_FUNCS, key=60 + box, plant=0.0)
    lower, upper = IC.BOXES[box]
    forest = Forest(3, 1, *_dev(value, type_, size))
    accepted = 0
    for v in range(3):
        if lower[v] == upper[v]:
            continue
        mask = forest.monotone_mask(lower, upper, {v: 1}).cpu().numpy()
        dfl = forest.SR_derivative_intervals(lower, upper, wrt=[v])[2][0, :, 0].cpu().numpy()
        moving = mask & ((dfl & DR.DEPENDS) != 0)
        accepted += int(moving.sum())
        X = []
        for _ in range(4):      # four settings of the other columns, 32 sorted values of x_v in each
            base = [np.float32(lower[k] + (upper[k] - lower[k]) * np.float32(rng.integers(0, 17) / 16.0)) for k in range(3)]
            for j in range(32):
                p = list(base)
                p[v] = np.float32(lower[v] + (upper[v] - lower[v]) * np.float32(j / 31.0))
                X.append(p)
        X = np.minimum(np.maximum(np.array(X, np.float32), lower[None, :]), upper[None, :])
        out = forest.batch_forward(torch.from_numpy(X).cuda())[:, :, 0].cpu().numpy().astype(np.float64).reshape(256, 4, 32)
        assert np.isfinite(out[mask]).all()
        drops = np.argwhere(mask[:, None, None] & (np.diff(out, axis=2) < 0))
        assert len(drops) == 0, [(int(t), int(g), int(j), out[t, g, j], out[t, g, j + 1]) for t, g, j in drops[:4]]
    assert accepted > 20, accepted


def test_deterministic_and_graph_replay(library_forest):
    """two calls and a graph replay (4 hardware queues, nothing set) give the same bits"""
    value, type_, size = library_forest
    args = _dev(value, type_, size, *IC.BOXES[0], np.array([0, 2], np.int32))
    first = [o.cpu().numpy() for o in torch.ops.evogp_hip.tree_derivative_intervals(*args)]
    second = [o.cpu().numpy() for o in torch.ops.evogp_hip.tree_derivative_intervals(*args)]
    _same_bits(second, first, "second call")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        torch.ops.evogp_hip.tree_derivative_intervals(*args)      # warm-up outside the capture
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            out = torch.ops.evogp_hip.tree_derivative_intervals(*args)
    torch.cuda.current_stream().wait_stream(side)
    for k in range(2):
        for o in out:
            o.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        _same_bits([o.cpu().numpy() for o in out], first, f"replay {k}")


@pytest.mark.parametrize("scaling", [False, True])
def test_problem_masks_trees_that_are_not_monotone(scaling, oracle, rng):
    """SymbolicRegression(monotonic=) on the device: trees that fail the mask score -inf, the others exactly what they score without
    (under linear scaling: unless their fitted slope is negative)"""
    value, type_, size = IC.oracle_forest(oracle, rng, 200, IC.ARITH, key=13, plant=0.0)
    X = rng.uniform(-1, 1, (64, 3)).astype(np.float32)
    y = (X[:, :1] * 2.0 + X[:, 1:2] - X[:, 2:3]).astype(np.float32)
    Xd, yd = _dev(X, y)
    forest = Forest(3, 1, *_dev(value, type_, size))
    plain = SymbolicRegression(datapoints=Xd, labels=yd, linear_scaling=scaling)
    prob = SymbolicRegression(datapoints=Xd, labels=yd, linear_scaling=scaling, monotonic={0: 1, 2: -1}, input_margin=0.1)
    mask = prob.monotone_mask(forest)
    o = DR.forest_derivative_intervals(value, type_, size, prob.input_lower.numpy(), prob.input_upper.numpy(), [0, 2])
    ref = DR.monotone(*o, [(0.0, np.inf), (-np.inf, 0.0)])
    assert np.array_equal(mask.cpu().numpy(), ref) and 0 < ref.sum() < 200
    assert not (mask & ~forest.safe_mask(prob.input_lower, prob.input_upper)).any()
    sc0, sc, ev0, ev = plain.scores(forest), prob.scores(forest), plain.evaluate(forest), prob.evaluate(forest)
    keep = mask
    if scaling:
        slope = plain.scaled_fitness(forest)[1]
        keep = mask & ~(slope < 0)
        assert (sc[mask & (slope < 0)] == float("-inf")).all()
    assert torch.equal(sc[keep], sc0[keep]) and (sc[~mask] == float("-inf")).all()
    assert torch.equal(ev[keep].view(torch.int32), ev0[keep].view(torch.int32)) and torch.isnan(ev[~mask]).all()
    assert torch.isfinite(sc0[~mask]).any() and torch.isfinite(sc[keep]).any()
