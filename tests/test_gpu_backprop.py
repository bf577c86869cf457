"""GPU: semantic backpropagation (csrc/sr_backprop.hip; ops tree_SR_desired and tree_SR_backprop_match).

  * the materialising op against the float32 restatement (tests/backprop_ref.py): status and state exactly, desired BIT FOR BIT on trees
    over + - * / neg inv sqrt abs max min IF, where the forward values and every rule are one correctly rounded float32 operation on both
    sides.  Where the last step is the EXP or LOG rule, desired against the float64 log / exp of the device's own target within the ulp
    bounds the project pins logf and expf to: tests/ulp_bounds.py line 14, LOG 1.9 and EXP 1.0 (the EXP rule calls logf, the LOG rule expf);
  * every path: LDS tapes (gp_len 64) and global tapes (gp_len 128, live lengths 1, 63, 64, 65, 79, 127), D = 1, 64, 65, 100, 257 (one to
    four waves per tree), the one-wave plan of a population that fills the chip, pos at the root, the last leaf, the deepest node and a
    random node, K = 1, 63, 64, 65, 200, 300, 1024 (the three sizes of the LDS row of sums);
  * the fused op against the materialised arrays of the SAME device: counts exactly; dist and const_dist recomputed in float64 numpy from
    the device's desired.  dist is a sum of at most D non-negative float64 terms on both sides: (D + 2) 2^-52 relative.
    const_dist: the device takes M2 = sum_q [S2_q - S1_q^2 / n_q] + the pairwise merge terms from sums SHIFTED by a pilot a_q, a REQUIRED
    value of the tree, so every term is at most R^2 with R = max - min of the REQUIRED desired values; S2_q and S1_q^2 / n_q are sums of
    n_q such terms, each sum rounded at most n_q + 3 times, and the merge adds at most four terms of size n R^2 / 4 with a handful of
    roundings each: |M2 - two-pass value| <= 4 (D + 8) 2^-52 n R^2, n the number of REQUIRED rows (M2 itself is at least R^2 / 2).
    const within one float32 ulp of the float64 mean; best: the recomputed distance of the chosen entry within the dist tolerance of the
    minimum, the smaller of two identical winners, never an entry that is not finite on a REQUIRED row, -1 without a REQUIRED row;
  * two runs give identical bits, the binding contract, the three forest invariants, SemanticBackpropMutation end to end on the device."""
import functools
import os
import sys
import zlib

import numpy as np
import pytest
import torch

import evogp_amd  # noqa: F401  (registers the ops)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import backprop_ref as BR  # noqa: E402
import backprop_tables as BT  # noqa: E402
import forest_invariance as FI  # noqa: E402
import sr_grad_ref as R  # noqa: E402
import test_backprop_host as H  # noqa: E402
import ulp_bounds  # noqa: E402
from grad_trees import random_forest  # noqa: E402
from helpers import fbits  # noqa: E402
from interval_cases import B, C, IF, U, V, flatten, rows  # noqa: E402

from evogp_amd.algorithm import DefaultCrossover, DefaultMutation, DefaultSelection, GeneticProgramming, SemanticBackpropMutation  # noqa: E402
from evogp_amd.pipeline import StandardPipeline  # noqa: E402
from evogp_amd.problem import SymbolicRegression  # noqa: E402
from evogp_amd.tree import Forest, GenerateDescriptor  # noqa: E402

pytestmark = pytest.mark.gpu
hip = torch.ops.evogp_hip
VAR_LEN = 3
BINARY = [R.F_ADD, R.F_SUB, R.F_MUL, R.F_DIV, R.F_MAX, R.F_MIN]


def _dev(*arrs):
    return [torch.from_numpy(np.array(a, copy=True, order="C")).cuda() for a in arrs]


def desired_op(forest, X, y, pos):
    return tuple(o.cpu().numpy() for o in hip.tree_SR_desired(*_dev(*forest), *_dev(X, y, np.asarray(pos, np.int32))))


def match_op(forest, X, y, pos, lib):
    return tuple(o.cpu().numpy() for o in hip.tree_SR_backprop_match(*_dev(*forest), *_dev(X, y, np.asarray(pos, np.int32), lib)))


def _nested(rng, depth, left, top=None):
    """a chain of `depth` random binary functions with random leaves, leaning left or right; `top`: a unary function on it (one node more)"""
    leaf = lambda: [np.float32(rng.integers(VAR_LEN)), R.T_VAR, 1] if rng.random() < 0.6 else [np.float32(rng.uniform(0.5, 1.5)), R.T_CONST, 1]  # noqa: E731
    n = 2 * depth + 1
    fs = [[np.float32(rng.choice(BINARY)), R.T_BFUNC, n - 2 * k] for k in range(depth)]
    nodes = fs + [leaf() for _ in range(depth + 1)] if left else [w for f in fs for w in (f, leaf())] + [leaf()]
    return ([[np.float32(top), R.T_UFUNC, n + 1]] if top is not None else []) + nodes


def _deepest(type_row, n):
    kids = BR.children(type_row, n)
    depth = [0] * n
    for i in range(n):
        for c in kids[i]:
            depth[c] = depth[i] + 1
    return int(np.argmax(depth))


@functools.lru_cache(maxsize=None)
def path_case(gp_len, D):
    """24 trees over the exact functions (W up to 4), a dataset, four position vectors and the float32 restatement of each: computed once,
    shared, never written to"""
    rng = np.random.default_rng([20261021, gp_len, D])
    value, type_, size = random_forest(rng, 24, gp_len, BR.EXACT32, VAR_LEN, 1, max_depth=5)
    lengths = (1, 63, 64, 65, 79, 127) if gp_len > 64 else (1, 31, 63)
    for t, n in enumerate(lengths):
        nodes = [[np.float32(1), R.T_VAR, 1]] if n == 1 else _nested(rng, (n - 1) // 2, left=t % 2 == 0, top=None if n % 2 else R.F_NEG)
        assert len(nodes) == n
        FI._set(value, type_, size, t, nodes)
    FI._set(value, type_, size, len(lengths), flatten(B(R.F_MUL, B(R.F_SUB, V(0), V(0)), V(1))))   # 0 * x1: FREE on the rows whose label is 0
    X = rng.uniform(0.5, 1.5, (D, VAR_LEN)).astype(np.float32)
    X[rng.random(X.shape) < 0.3] *= -1.0
    X[rng.random(X.shape) < 0.05] = 0.0
    y = (1.5 * X[:, :1] ** 2 - X[:, -1:]).astype(np.float32)
    y[rng.random(y.shape) < 0.1] = 0.0
    n = size[:, 0].astype(np.int64)
    positions = {"root": np.zeros(24, np.int32), "last leaf": (n - 1).astype(np.int32),
                 "deepest": np.array([_deepest(type_[t], n[t]) for t in range(24)], np.int32),
                 "random": (rng.integers(0, 1 << 20, 24) % n).astype(np.int32)}
    forest = (value, type_, size)
    with np.errstate(all="ignore"):
        ref = {k: BR.forest_desired(*forest, X, y, p, np.float32) for k, p in positions.items()}
    for a in forest + (X, y) + tuple(positions.values()) + tuple(x for r in ref.values() for x in r):
        a.setflags(write=False)
    return forest, X, y, positions, ref


def assert_materialised(got, want, what):
    desired, state, status = got
    assert desired.dtype == np.float32 and state.dtype == np.uint8 and status.dtype == np.int32
    assert np.array_equal(status, want[2]), f"{what}: status differs at trees {np.flatnonzero(status != want[2])[:4].tolist()}"
    assert np.array_equal(state, want[1]), f"{what}: state differs at {np.argwhere(state != want[1])[:4].tolist()}"
    same = fbits(desired) == fbits(want[0])
    assert same.all(), f"{what}: desired differs at {np.argwhere(~same)[:4].tolist()}: {desired[~same][:4]} against {want[0][~same][:4]}"


def check_fused(forest, X, y, pos, K, got, what):
    """the fused op at K library rows against the materialised arrays `got` of the same device"""
    desired, state, status = got
    pop, D = desired.shape
    rng = np.random.default_rng([K, zlib.crc32(what.encode())])
    lib = rng.uniform(-2, 2, (K, D)).astype(np.float32)
    has = np.flatnonzero((status == 0) & (state == 0).any(1))
    t0 = int(has[0]) if len(has) else None
    if K >= 8 and t0 is not None:
        lib[3] = lib[7] = np.where(state[t0] == 0, desired[t0], 0.25)    # two identical rows that win on tree t0
        lib[5] = np.inf                                                   # never finite
        lib[6, np.flatnonzero(state[t0] == 0)[0]] = np.nan                # not finite on a REQUIRED row of t0
    best, dist, const, const_dist, counts, status2 = match_op(forest, X, y, pos, lib)
    assert best.dtype == np.int32 and dist.dtype == np.float64 and const.dtype == np.float32 and const_dist.dtype == np.float64 and counts.dtype == np.int32
    assert dist.shape == (pop, K) and counts.shape == (pop, 3)
    rbest, rdist, rconst, rconst_dist, rcounts = BR.match(desired, state, status, lib)
    assert np.array_equal(status2, status) and np.array_equal(counts, rcounts), f"{what}: status or counts differ"
    assert np.array_equal(np.isinf(dist), np.isinf(rdist)) and not np.isnan(dist).any(), f"{what}: the +inf entries differ"
    fin = np.isfinite(rdist)
    tol = (D + 2) * 2.0 ** -52
    bad = fin & ~(np.abs(np.where(fin, dist, 0) - np.where(fin, rdist, 0)) <= tol * np.where(fin, rdist, 0))
    assert not bad.any(), f"{what}: dist beyond (D + 2) 2^-52 at {np.argwhere(bad)[:4].tolist()}: {dist[bad][:4]} against {rdist[bad][:4]}"
    assert np.array_equal(best == -1, rbest == -1), f"{what}: best == -1 at other trees than expected: {np.flatnonzero((best == -1) != (rbest == -1))[:4].tolist()}"
    for t in np.flatnonzero(best >= 0):
        assert 0 <= best[t] < K and rdist[t, best[t]] <= rdist[t].min() * (1 + tol), f"{what}: tree {t} chose {best[t]} at {rdist[t, best[t]]}, the minimum is {rdist[t].min()}"
    if K >= 8 and t0 is not None:
        assert best[t0] == 3 and dist[t0, 3] == 0 and dist[t0, 7] == 0 and np.isinf(dist[t0, 5]) and np.isinf(dist[t0, 6]), f"{what}: the planted rows on tree {t0}"
        assert (best != 5).all()
    req = counts[:, 0] > 0
    assert np.array_equal(np.isnan(const), ~req) and np.array_equal(np.isnan(const_dist), ~req), f"{what}: const is NaN exactly without a REQUIRED row"
    for t in np.flatnonzero(req):
        d = desired[t, state[t] == 0].astype(np.float64)
        ulp = float(np.spacing(np.abs(np.float32(rconst[t]))))
        assert abs(float(const[t]) - rconst[t]) <= ulp, f"{what}: const of tree {t}: {const[t]!r} against {rconst[t]!r}"
        bound = 4 * (D + 8) * 2.0 ** -52 * len(d) * float(d.max() - d.min()) ** 2
        assert abs(const_dist[t] - rconst_dist[t]) <= bound, f"{what}: const_dist of tree {t}: {const_dist[t]!r} against {rconst_dist[t]!r}, bound {bound:.3g}"
    return (best, dist, const, const_dist, counts, status2), lib


def _bits(a):
    return a.view(np.uint64) if a.dtype == np.float64 else fbits(a) if a.dtype == np.float32 else a


def same_bits(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


# ---- every path ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 64, 65, 100, 257])
@pytest.mark.parametrize("gp_len", [64, 128])
def test_paths(gp_len, D):
    forest, X, y, positions, ref = path_case(gp_len, D)
    states = np.zeros(3, np.int64)
    for k, (name, pos) in enumerate(positions.items()):
        what = f"L={gp_len} D={D} pos={name}"
        got = desired_op(forest, X, y, pos)
        assert_materialised(got, ref[name], what)
        if name == "root":
            assert (got[1] == 0).all() and np.array_equal(fbits(got[0]), fbits(np.broadcast_to(y[:, 0], got[0].shape)))
        states += np.bincount(got[1].ravel(), minlength=3)
        assert same_bits(desired_op(forest, X, y, pos), got), f"{what}: two calls differ"
        for K in ((1, 63, 64, 65, 200, 300, 1024) if D == 100 and name == "random" else (65,) if k % 2 else (8,)):
            fused, lib = check_fused(forest, X, y, pos, K, got, f"{what} K={K}")
            assert same_bits(match_op(forest, X, y, pos, lib), fused), f"{what} K={K}: two fused calls differ"
    if D >= 64:
        assert states.all(), f"L={gp_len} D={D}: a state does not occur: {states}"


def test_a_population_that_fills_the_chip_takes_one_wave_per_tree():
    """pop >= 16 x compute units of one-to-three-node trees: the plan gives every tree ONE wave, which walks the two tiles of D = 100 itself"""
    pop, L, D = 16 * torch.cuda.get_device_properties(0).multi_processor_count, 8, 100
    rng = np.random.default_rng(4200)
    leaf = lambda: V(int(rng.integers(VAR_LEN))) if rng.random() < 0.7 else C(float(rng.uniform(0.5, 1.5)))  # noqa: E731
    shapes = [lambda: leaf(), lambda: U(int(rng.choice([R.F_NEG, R.F_ABS, R.F_INV, R.F_SQRT])), leaf()), lambda: B(int(rng.choice(BINARY)), leaf(), leaf())]
    forest = rows([shapes[int(rng.integers(3))]() for _ in range(pop)], L)
    X = rng.uniform(0.5, 1.5, (D, VAR_LEN)).astype(np.float32)
    X[rng.random(X.shape) < 0.3] *= -1.0
    y = (X[:, :1] * X[:, 1:2]).astype(np.float32)
    pos = (rng.integers(0, 6, pop) % forest[2][:, 0]).astype(np.int32)
    got = desired_op(forest, X, y, pos)
    with np.errstate(all="ignore"):
        assert_materialised(got, BR.forest_desired(*forest, X, y, pos, np.float32), "W = 1")
    check_fused(forest, X, y, pos, 70, got, "W = 1 K=70")
    # a slice of the forest runs under another plan (W = 2): the materialised arrays do not depend on it
    part = desired_op(tuple(a[:24] for a in forest), X, y, pos[:24])
    assert same_bits(part, tuple(a[:24] for a in got))


# ---- the EXP and LOG rules ----------------------------------------------------------------------------------------------------------------
def test_exp_and_log_rules_within_the_library_bounds():
    """exp(x0) + x1 and x2 * log(x0 + x1): the last step is the EXP rule (logf of the target) and the LOG rule (expf of it).  The target is
    the desired value AT the EXP / LOG node, which the device gives bit for bit; the truth is the float64 function of it"""
    D = 200
    rng = np.random.default_rng(14)
    X = rng.uniform(0.5, 1.5, (D, VAR_LEN)).astype(np.float32)
    y = rng.uniform(-3.0, 40.0, (D, 1)).astype(np.float32)    # targets up to 80: expf stays far below float32's maximum
    forest = rows([B(R.F_ADD, U(R.F_EXP, V(0)), V(1)), B(R.F_MUL, V(2), U(R.F_LOG, B(R.F_ADD, V(0), V(1))))], 16)
    at = np.array([1, 2], np.int32)   # the EXP node, the LOG node
    target = desired_op(forest, X, y, at)
    got = desired_op(forest, X, y, at + 1)
    with np.errstate(all="ignore"):
        assert_materialised(target, BR.forest_desired(*forest, X, y, at, np.float32), "the targets of the last step")
        want = BR.forest_desired(*forest, X, y, at + 1, np.float32)
        assert np.array_equal(got[2], want[2]) and not got[2].any() and np.array_equal(got[1], want[1]) and (target[1] == 0).all()
        t64 = target[0].astype(np.float64)
        assert np.array_equal(got[1][0] == 0, t64[0] > 0) and (got[1][0][t64[0] <= 0] == 2).all() and (got[1][1] == 0).all()
        for t, (rule, fn, truth) in enumerate((("EXP", "LOG", np.log(t64[0])), ("LOG", "EXP", np.exp(t64[1])))):
            ulps = ulp_bounds.UNARY[fn][0]   # tests/ulp_bounds.py:14 -- the EXP rule calls logf (1.9), the LOG rule expf (1.0)
            ok = got[1][t] == 0
            assert ok.sum() > D // 2
            err = np.abs(got[0][t][ok].astype(np.float64) - truth[ok]) / np.spacing(np.abs(truth[ok]).astype(np.float32)).astype(np.float64)
            print(f"the {rule} rule: worst error {err.max():.3f} ulp over {int(ok.sum())} rows, bound {ulps}")
            assert err.max() <= ulps, f"the {rule} rule: {err.max():.3f} ulp"


# ---- edge rows among ordinary trees -------------------------------------------------------------------------------------------------------
def test_edge_rows_among_ordinary_trees():
    L, D = 16, 70
    rng = np.random.default_rng(70)
    ordinary = [B(R.F_ADD, B(R.F_MUL, V(0), V(1)), V(0)), B(R.F_SUB, V(2), B(R.F_DIV, V(0), V(1)))]
    edge = [U(R.F_SIN, V(0)),                                       # 2: blocked
            IF(V(0), V(1), V(2)),                                   # 3: entered through the condition: blocked
            B(R.F_MUL, B(R.F_SUB, V(1), V(1)), V(0)),               # 4: 0 * x0 against labels that are never 0: every row IMPOSSIBLE
            B(R.F_MUL, B(R.F_SUB, V(1), V(1)), V(0)),               # 5: the same tree, pos out of range
            B(R.F_ADD, C(np.nan), V(0)),                            # 6: a NaN sibling
            IF(V(0), V(1), V(2))]                                   # 7: the branch taken where x0 > 0, the other branch decides elsewhere
    pos = [4, 3, 1, 1, 4, 5, 2, 2] + [4, 3]
    value, type_, size = rows(ordinary + edge, L)
    mal = np.zeros((2, L), np.float32), np.zeros((2, L), np.int16), np.zeros((2, L), np.int16)
    mal[0][0, :2], mal[1][0, :2], mal[2][0, :2] = [R.F_ADD, 0], [R.T_BFUNC, R.T_VAR], [2, 1]      # x0 + <nothing>
    mal[0][1, 0], mal[1][1, 0], mal[2][1, 0] = 0.5, R.T_CONST, 0                                  # n = 0
    tail = rows(ordinary, L)
    forest = tuple(np.concatenate([a, m, t]) for a, m, t in zip((value, type_, size), mal, tail))
    pos = np.array(pos[:8] + [0, 0] + pos[8:], np.int32)
    X = rng.uniform(0.5, 1.5, (D, VAR_LEN)).astype(np.float32)
    X[::3, 0] *= -1.0
    y = (X[:, :1] * X[:, 1:2] + X[:, 2:3]).astype(np.float32)
    X[6, 2] = y[6, 0] = 0.75       # tree 7, a row where the IF returns x2 (x0 <= 0) and x2 is the label: FREE
    got = desired_op(forest, X, y, pos)
    with np.errstate(all="ignore"):
        assert_materialised(got, BR.forest_desired(*forest, X, y, pos, np.float32), "edge rows")
    desired, state, status = got
    assert status.tolist() == [0, 0, 3, 3, 0, 2, 0, 0, 1, 1, 0, 0]
    assert (state[[2, 3, 4, 5, 6, 8, 9]] == 2).all() and np.isnan(desired[[2, 3, 4, 5, 6, 8, 9]]).all()
    assert np.array_equal(state[7] == 0, X[:, 0] > 0) and state[7, 6] == 1 and (np.delete(state[7], 6)[np.delete(X[:, 0], 6) <= 0] == 2).all()
    for a, b in ((0, 10),):   # the neighbours are untouched
        assert np.array_equal(fbits(desired[a:a + 2]), fbits(desired[b:b + 2])) and np.array_equal(state[a:a + 2], state[b:b + 2])
    (best, dist, const, const_dist, counts, _), _ = check_fused(forest, X, y, pos, 65, got, "edge rows K=65")
    assert (best[[2, 3, 4, 5, 6, 8, 9]] == -1).all() and not dist[[2, 3, 4, 5, 6, 8, 9]].any() and (counts[[2, 3, 4, 5, 6, 8, 9]] == [0, 0, D]).all()
    # a library that is finite nowhere: every distance +inf, best -1, the constant still given
    best, dist, const, const_dist, counts, _ = match_op(forest, X, y, pos, np.full((3, D), np.inf, np.float32))
    assert (best == -1).all() and np.isinf(dist[[0, 1, 7, 10, 11]]).all() and np.isfinite(const[[0, 1, 7]]).all()


# ---- the binding contract, the C ABI and the forest invariants -------------------------------------------------------------------------
@pytest.mark.parametrize("op", [BT.DESIRED, BT.MATCH])
def test_binding_contract(op):
    BT.BC.test_valid_call_and_one_fault_at_a_time(op)


@pytest.mark.parametrize("op,case", [(op, c) for op in (BT.DESIRED, BT.MATCH) for c in FI.cases_for(op)])
def test_op_keeps_the_invariants(op, case):
    FI.check(op, FI.TABLE[op], FI.build_case(case), "cuda")
    torch.cuda.synchronize()


def test_argument_errors_through_the_c_abi_launch_nothing():
    import ctypes as C_
    from evogp_amd import _lib
    lib_ = _lib.lib
    forest = _dev(*rows([V(0)] * 4, 8))
    X, y, pos, libt = _dev(np.ones((8, 2), np.float32), np.full((8, 1), 3.0, np.float32), np.zeros(4, np.int32), np.ones((8, 2), np.float32))
    desired, state = torch.full((4, 8), 7.0, device="cuda"), torch.full((4, 8), 7, dtype=torch.uint8, device="cuda")
    status = torch.full((4,), 7, dtype=torch.int32, device="cuda")
    dist, best = torch.full((4, 2), 7.0, dtype=torch.float64, device="cuda"), torch.full((4,), 7, dtype=torch.int32, device="cuda")
    const, const_dist = torch.full((4,), 7.0, device="cuda"), torch.full((4,), 7.0, dtype=torch.float64, device="cuda")
    counts = torch.full((4, 3), 7, dtype=torch.int32, device="cuda")
    p = lambda t: None if t is None else C_.c_void_p(t.data_ptr())  # noqa: E731

    def des(pop=4, D=8, gp_len=8, var_len=2, out_len=1, value=forest[0], out=desired):
        return lib_.evogp_hip_sr_desired(pop, D, gp_len, var_len, out_len, p(value), p(forest[1]), p(forest[2]), p(X), p(y), p(pos), p(out), p(state),
                                         p(status), None)

    def mat(pop=4, D=8, gp_len=8, var_len=2, out_len=1, value=forest[0], out=dist, K=2):
        return lib_.evogp_hip_sr_backprop_match(pop, D, gp_len, var_len, out_len, p(value), p(forest[1]), p(forest[2]), p(X), p(y), p(pos), K, p(libt),
                                                p(out), p(best), p(const), p(const_dist), p(counts), p(status), None)

    for f in (des, mat):
        for bad in (dict(pop=0), dict(D=0), dict(gp_len=0), dict(gp_len=1025), dict(var_len=0), dict(out_len=0)):
            assert f(**bad) == -1, (f.__name__, bad)
        assert f(value=None) == -2 and f(out=None) == -2 and f(out_len=2) == -3
    assert mat(K=0) == -1 and mat(K=1025) == -1
    torch.cuda.synchronize()
    assert all((t == 7).all() for t in (desired, state, status, dist, best, const, const_dist, counts))   # nothing was launched
    assert des() == 0 and mat() == 0
    torch.cuda.synchronize()
    assert (desired == 3).all() and (state == 0).all() and (status == 0).all() and (dist == 32).all() and (best == 0).all()
    assert (const == 3).all() and (const_dist == 0).all() and (counts == torch.tensor([8, 0, 0], device="cuda")).all()


# ---- Forest and SemanticBackpropMutation end to end ------------------------------------------------------------------------------------
def _cuda_forest(exprs, width=H.L):
    return Forest(3, 1, *_dev(*rows(exprs, width)))


@pytest.mark.parametrize("name", sorted(H.PLANTED))
def test_a_planted_defect_is_repaired_in_one_call(name):
    truth, wrong, pos = H.PLANTED[name]
    X = H._data().cuda()
    y = _cuda_forest([truth]).batch_forward(X)[:, :, 0].t().contiguous()
    op = SemanticBackpropMutation(1.0, X, y, library=_cuda_forest([V(1), B(R.F_ADD, V(0), V(1)), V(2), C(0.5)]))
    f = _cuda_forest([wrong, wrong])
    op.apply(f, torch.tensor([1], device="cuda"), torch.tensor([pos], dtype=torch.int32, device="cuda"))
    for a, b in zip(f._tensors(), _cuda_forest([wrong, truth])._tensors()):
        assert torch.equal(a, b), name
    assert torch.equal(f.batch_forward(X)[1, :, 0], y[:, 0])   # loss exactly 0


def test_the_constant_donor_and_the_forest_methods():
    X = H._data().cuda()
    y = (X[:, :1] + 2.5).contiguous()
    lib = _cuda_forest([V(0), V(1), V(2)])
    f = _cuda_forest([B(R.F_ADD, V(0), V(1)), U(R.F_SIN, V(0))])
    pos = torch.tensor([2, 1], dtype=torch.int32, device="cuda")
    desired, state, status = f.SR_desired_semantics(X, y, pos)
    assert status.tolist() == [0, 3] and (desired[0] == 2.5).all() and (state[0] == 0).all() and (state[1] == 2).all()
    best, dist, const, const_dist, counts, _ = f.SR_backprop_match(X, y, pos, lib)
    assert best[1] == -1 and float(const[0]) == 2.5 and float(const_dist[0]) == 0.0 and counts.tolist() == [[24, 0, 0], [0, 0, 24]]
    assert torch.equal(dist, f.SR_backprop_match(X, y, pos, lib.batch_forward(X)[:, :, 0].contiguous())[1])
    SemanticBackpropMutation(1.0, X, y, library=lib).apply(f, torch.tensor([0, 1], device="cuda"), pos)
    for a, b in zip(f._tensors(), _cuda_forest([B(R.F_ADD, V(0), C(2.5)), U(R.F_SIN, V(0))])._tensors()):
        assert torch.equal(a, b)   # the constant 2.5; the blocked tree bit for bit


def test_three_generations_of_genetic_programming():
    rng = np.random.default_rng(5)
    X = torch.from_numpy(rng.uniform(-2, 2, (256, 2)).astype(np.float32)).cuda()
    y = (X[:, :1] ** 2 + X[:, :1] * X[:, 1:2]).contiguous()
    d = GenerateDescriptor(max_tree_len=32, input_len=2, output_len=1, using_funcs=["+", "-", "*", "/", "sin"], max_layer_cnt=4, const_samples=[-1, 0, 1, 2])
    torch.manual_seed(9)
    op = SemanticBackpropMutation(0.3, X, y, descriptor=d, library_size=100, fallback=DefaultMutation(0.3, d))
    assert 2 < op.library.pop_size <= 102 and op.semantics.shape == (op.library.pop_size, 256)
    algo = GeneticProgramming(Forest.random_generate(200, d, keys=torch.tensor([1, 2], dtype=torch.uint32, device="cuda")), DefaultCrossover(), op,
                              DefaultSelection(0.3, 2))
    first = float(SymbolicRegression(datapoints=X, labels=y).scores(algo.forest).max())
    pipe = StandardPipeline(algo, SymbolicRegression(datapoints=X, labels=y), generation_limit=3, is_show_details=False)
    best = pipe.run()
    assert best is pipe.best_tree and np.isfinite(float(pipe.best_fitness)) and float(pipe.best_fitness) >= first
    t, s = algo.forest.batch_node_type.cpu().numpy(), algo.forest.batch_subtree_size.cpu().numpy()
    from subtree_ref import check_prefix_tree
    assert all(check_prefix_tree(t[i], s[i]) for i in range(200))
    op.update_library(algo.forest)
    assert 1 <= op.library.pop_size <= 200
    algo.step(SymbolicRegression(datapoints=X, labels=y).scores(algo.forest))
