"""GPU: the midpoint builds of semantic backpropagation (csrc/sr_backprop.hip with MID; ops tree_SR_desired_mid and tree_SR_agx_match;
approximately geometric semantic crossover).

  * the materialising op against the float32 restatement (tests/agx_ref.py): status and state exactly, desired BIT FOR BIT on trees over
    + - * / neg inv sqrt abs max min IF -- the forward values of both parents, the midpoint 0.5 * a + 0.5 * b and every rule are correctly
    rounded float32 operations on both sides;
  * every path: 24 recipients and 24 mates built as tests/test_gpu_backprop.py builds its trees, LDS tapes (gp_len 64) and global tapes
    (gp_len 128, live lengths 1, 63, 64, 65, 79, 127 among recipients AND mates), D = 1, 64, 65, 257, pos at the root, the last leaf, the
    deepest node and a random node, a mate vector that is a permutation but for one repeated mate, with one pair of a tree with itself;
  * the fused op against float64 numpy on the device's own desired values, with the bounds of check_fused in tests/test_gpu_backprop.py
    (they derive from the summation, not from where the target came from), K = 1, 64, 65, 300, 1024;
  * a path that shares nothing with the new walk: the labelled op tree_SR_desired on one tree alone, its labels the midpoint that torch
    forms from batch_forward of the two forests;
  * the one-wave plan, stale words behind a mate's live length, two calls, the three forest invariants, the binding contract, the C
    argument checks, and the operator end to end on the device."""
import functools
import os
import sys
from contextlib import contextmanager

import numpy as np
import pytest
import torch

import evogp_amd  # noqa: F401  (registers the ops)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import agx_ref as AR  # noqa: E402
import agx_tables as AT  # noqa: E402
import backprop_ref as BR  # noqa: E402
import forest_invariance as FI  # noqa: E402
import sr_grad_ref as R  # noqa: E402
import test_agx_host as H  # noqa: E402
import test_gpu_backprop as G  # noqa: E402
from grad_trees import random_forest  # noqa: E402
from helpers import fbits  # noqa: E402
from interval_cases import B, C, U, V, rows  # noqa: E402

from evogp_amd.algorithm import ApproxGeometricCrossover, DefaultCrossover, DefaultMutation, DefaultSelection, GeneticProgramming  # noqa: E402
from evogp_amd.pipeline import StandardPipeline  # noqa: E402
from evogp_amd.problem import SymbolicRegression  # noqa: E402
from evogp_amd.tree import Forest, GenerateDescriptor  # noqa: E402

pytestmark = pytest.mark.gpu
hip = torch.ops.evogp_hip
VAR_LEN = G.VAR_LEN
_dev = G._dev


def desired_mid_op(forest, mates, X, pos, mate):
    return tuple(o.cpu().numpy() for o in hip.tree_SR_desired_mid(*_dev(*forest), *_dev(*mates), *_dev(X, np.asarray(pos, np.int32), np.asarray(mate, np.int32))))


def agx_match_op(forest, mates, X, pos, mate, lib):
    return tuple(o.cpu().numpy() for o in hip.tree_SR_agx_match(*_dev(*forest), *_dev(*mates), *_dev(X, np.asarray(pos, np.int32), np.asarray(mate, np.int32), lib)))


@contextmanager
def fused_through(mates, mate):
    """G.check_fused with its fused call going to tree_SR_agx_match: the same bounds, the labels unused"""
    saved = G.match_op
    G.match_op = lambda forest, X, y, pos, lib: agx_match_op(forest, mates, X, pos, mate, lib)
    try:
        yield
    finally:
        G.match_op = saved


def _mates_like_path_case(gp_len, rng):
    """24 trees built as G.path_case builds its recipients, from another stream"""
    value, type_, size = random_forest(rng, 24, gp_len, BR.EXACT32, VAR_LEN, 1, max_depth=5)
    lengths = (127, 1, 79, 63, 65, 64) if gp_len > 64 else (63, 1, 31)
    for t, n in enumerate(lengths):
        nodes = [[np.float32(2), R.T_VAR, 1]] if n == 1 else G._nested(rng, (n - 1) // 2, left=t % 2 == 1, top=None if n % 2 else R.F_ABS)
        assert len(nodes) == n
        FI._set(value, type_, size, t, nodes)
    return value, type_, size, len(lengths)


@functools.lru_cache(maxsize=None)
def mid_case(gp_len, D):
    """the recipients, data and positions of G.path_case, 24 mates, the mate vector and the float32 restatement of each position vector:
    computed once, shared, never written to"""
    forest, X, _, positions, _ = G.path_case(gp_len, D)
    rng = np.random.default_rng([20261021, 25, gp_len, D])
    mv, mt, ms, k = _mates_like_path_case(gp_len, rng)
    for a, b in zip((mv, mt, ms), forest):
        a[k] = b[k]                    # the recipient 0 * x1 is its own mate: a midpoint of 0, FREE at its x1 leaf
    mate = rng.permutation(24).astype(np.int32)
    mate[np.flatnonzero(mate == k)[0]] = mate[k]
    mate[k] = k                        # one pair of a tree with itself ...
    mate[(k + 5) % 24] = mate[(k + 6) % 24]   # ... and one mate taken twice
    assert (mate == k).sum() == 1 and len(set(mate.tolist())) == 23
    mates = (mv, mt, ms)
    with np.errstate(all="ignore"):
        ref = {name: AR.forest_desired_mid(*forest, *mates, X, p, mate, np.float32) for name, p in positions.items()}
    for a in mates + (mate,) + tuple(x for r in ref.values() for x in r):
        a.setflags(write=False)
    return forest, mates, X, positions, mate, ref


# ---- every path ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 64, 65, 257])
@pytest.mark.parametrize("gp_len", [64, 128])
def test_paths(gp_len, D):
    forest, mates, X, positions, mate, ref = mid_case(gp_len, D)
    want_lengths = {1, 63, 64, 65, 79, 127} if gp_len > 64 else {1, 31, 63}
    assert want_lengths <= set(forest[2][:, 0].tolist()) and want_lengths <= set(mates[2][:, 0].tolist())
    states = np.zeros(3, np.int64)
    for k, (name, pos) in enumerate(positions.items()):
        what = f"L={gp_len} D={D} pos={name}"
        got = desired_mid_op(forest, mates, X, pos, mate)
        G.assert_materialised(got, ref[name], what)
        if name == "root":   # the midpoints themselves, and exactly the finite ones REQUIRED
            assert not got[2].any() and np.array_equal(got[1] == 0, np.isfinite(got[0])) and (got[1][got[1] != 0] == 2).all()
        states += np.bincount(got[1].ravel(), minlength=3)
        assert G.same_bits(desired_mid_op(forest, mates, X, pos, mate), got), f"{what}: two calls differ"
        with fused_through(mates, mate):
            for K in ((1, 64, 65, 300, 1024) if D == 65 and name == "random" else (65,) if k % 2 else (8,)):
                fused, lib = G.check_fused(forest, X, None, pos, K, got, f"{what} K={K}")
                assert G.same_bits(agx_match_op(forest, mates, X, pos, mate, lib), fused), f"{what} K={K}: two fused calls differ"
    if D >= 64:
        assert states.all(), f"L={gp_len} D={D}: a state does not occur: {states}"


@pytest.mark.parametrize("gp_len,D", [(64, 65), (128, 257)])
def test_the_labelled_op_on_one_tree_with_torchs_midpoint_gives_the_same_bits(gp_len, D):
    """a path that shares nothing with the new walk: a and b from batch_forward of the two forests, the midpoint from torch float32, the
    inversion from tree_SR_desired on that tree alone"""
    forest, mates, X, positions, mate, _ = mid_case(gp_len, D)
    pos = positions["random"]
    got = desired_mid_op(forest, mates, X, pos, mate)
    Xd = torch.from_numpy(np.array(X)).cuda()
    a = Forest(VAR_LEN, 1, *_dev(*forest)).batch_forward(Xd)[:, :, 0]
    b = Forest(VAR_LEN, 1, *_dev(*mates)).batch_forward(Xd)[:, :, 0]
    mid = (0.5 * a + 0.5 * b[torch.from_numpy(np.array(mate)).cuda().long()]).cpu().numpy()
    compared = 0
    for t in range(16):
        one = tuple(np.ascontiguousarray(x[t:t + 1]) for x in forest)
        d, st, status = G.desired_op(one, X, np.ascontiguousarray(mid[t][:, None]), pos[t:t + 1])
        assert status[0] == got[2][t], f"tree {t}: status {status[0]} against {got[2][t]}"
        fin = np.isfinite(mid[t])
        assert np.array_equal(st[0][fin], got[1][t][fin]) and np.array_equal(fbits(d[0][fin]), fbits(got[0][t][fin])), f"tree {t}"
        assert (got[1][t][~fin] == 2).all() and np.isnan(got[0][t][~fin]).all()
        compared += int(fin.sum())
    assert compared > 8 * D


def test_a_population_that_fills_the_chip_takes_one_wave_per_tree():
    """pop >= 16 x compute units of one-to-three-node trees: the plan gives every tree ONE wave, which walks the two tiles of D = 100 itself"""
    pop, L, D = 16 * torch.cuda.get_device_properties(0).multi_processor_count, 8, 100
    rng = np.random.default_rng(4201)
    leaf = lambda: V(int(rng.integers(VAR_LEN))) if rng.random() < 0.7 else C(float(rng.uniform(0.5, 1.5)))  # noqa: E731
    shapes = [lambda: leaf(), lambda: U(int(rng.choice([R.F_NEG, R.F_ABS, R.F_INV, R.F_SQRT])), leaf()), lambda: B(int(rng.choice(G.BINARY)), leaf(), leaf())]
    forest = rows([shapes[int(rng.integers(3))]() for _ in range(pop)], L)
    mates = rows([shapes[int(rng.integers(3))]() for _ in range(100)], L)
    X = rng.uniform(0.5, 1.5, (D, VAR_LEN)).astype(np.float32)
    X[rng.random(X.shape) < 0.3] *= -1.0
    pos = (rng.integers(0, 6, pop) % forest[2][:, 0]).astype(np.int32)
    mate = rng.integers(0, 100, pop).astype(np.int32)
    got = desired_mid_op(forest, mates, X, pos, mate)
    with np.errstate(all="ignore"):
        G.assert_materialised(got, AR.forest_desired_mid(*forest, *mates, X, pos, mate, np.float32), "W = 1")
    with fused_through(mates, mate):
        G.check_fused(forest, X, None, pos, 70, got, "W = 1 K=70")
    # a slice of the forest runs under another plan (W = 2): the materialised arrays do not depend on it
    part = desired_mid_op(tuple(a[:24] for a in forest), mates, X, pos[:24], mate[:24])
    assert G.same_bits(part, tuple(a[:24] for a in got))


def test_stale_words_behind_a_mates_live_length_change_no_bit():
    forest, mates, X, positions, mate, _ = mid_case(64, 65)
    stale = FI.stale_tails(np.random.default_rng(77), *(np.array(a) for a in mates), 1)[:3]
    n = mates[2][:, 0].astype(np.int64)
    assert any(not np.array_equal(fbits(a), fbits(b)) for a, b in zip(stale, mates)) and np.array_equal(stale[2][:, 0], mates[2][:, 0])
    assert all(np.array_equal(fbits(a[t, :n[t]]) if a.dtype == np.float32 else a[t, :n[t]], fbits(b[t, :n[t]]) if b.dtype == np.float32 else b[t, :n[t]])
               for a, b in zip(stale, mates) for t in range(24))
    pos = positions["random"]
    lib = np.random.default_rng(78).uniform(-2, 2, (70, 65)).astype(np.float32)
    assert G.same_bits(desired_mid_op(forest, stale, X, pos, mate), desired_mid_op(forest, mates, X, pos, mate))
    assert G.same_bits(agx_match_op(forest, stale, X, pos, mate, lib), agx_match_op(forest, mates, X, pos, mate, lib))


def test_status_codes_and_their_order_among_ordinary_trees():
    L, D = 16, 70
    rng = np.random.default_rng(71)
    SUM = B(R.F_ADD, B(R.F_MUL, V(0), V(1)), V(0))
    recipients = [SUM, U(R.F_SIN, V(0)), U(R.F_SIN, V(0)), SUM, SUM, SUM, SUM, C(np.inf), SUM, SUM]
    mates = list(rows([V(0), B(R.F_DIV, V(1), V(2)), C(np.inf), B(R.F_ADD, V(0), V(2))], L))
    mates[2][3, 0] = 2   # x0 + <nothing>
    forest = list(rows(recipients, L))
    forest[2][8, 0] = 2  # a malformed recipient
    pos = np.array([4, 1, 1, 4, 4, 5, 0, 0, 0, 4], np.int32)
    mate = np.array([0, 0, 4, -1, 3, 7, 2, 0, 9, 1], np.int32)
    X = rng.uniform(0.5, 1.5, (D, VAR_LEN)).astype(np.float32)
    X[::3, 0] *= -1.0
    X[5::11, 2] = 0.0     # mate 1 is NaN on these rows only
    got = desired_mid_op(forest, mates, X, pos, mate)
    with np.errstate(all="ignore"):
        G.assert_materialised(got, AR.forest_desired_mid(*forest, *mates, X, pos, mate, np.float32), "status codes")
    desired, state, status = got
    assert status.tolist() == [0, 3, 4, 4, 4, 2, 0, 0, 1, 0]
    gone = [1, 2, 3, 4, 5, 6, 7, 8]   # a status, an infinite mate, an infinite recipient
    assert (state[gone] == 2).all() and np.isnan(desired[gone]).all() and (state[0] == 0).all()
    assert np.array_equal(state[9] == 2, X[:, 2] == 0) and (state[9][X[:, 2] != 0] == 0).all() and 0 < (state[9] == 2).sum() < D
    with fused_through(mates, mate):
        (best, dist, _, _, counts, _), _ = G.check_fused(forest, X, None, pos, 65, got, "status codes K=65")
    assert (best[gone] == -1).all() and not dist[gone].any() and (counts[gone] == [0, 0, D]).all()


# ---- the binding contract, the C ABI and the forest invariants -------------------------------------------------------------------------
@pytest.mark.parametrize("op", [AT.DESIRED_MID, AT.AGX_MATCH])
def test_binding_contract(op):
    AT.BC.test_valid_call_and_one_fault_at_a_time(op)


@pytest.mark.parametrize("op,case", [(op, c) for op in (AT.DESIRED_MID, AT.AGX_MATCH) for c in FI.cases_for(op)])
def test_op_keeps_the_invariants(op, case):
    FI.check(op, FI.TABLE[op], FI.build_case(case), "cuda")
    torch.cuda.synchronize()


def test_argument_errors_through_the_c_abi_launch_nothing():
    import ctypes as C_
    from evogp_amd import _lib
    lib_ = _lib.lib
    forest = _dev(*rows([V(0)] * 4, 8))
    mates = _dev(*rows([C(5.0)] * 3, 8))
    X, pos, mate, libt = _dev(np.ones((8, 2), np.float32), np.zeros(4, np.int32), np.array([0, 1, 2, 0], np.int32), np.ones((8, 2), np.float32))
    desired, state = torch.full((4, 8), 7.0, device="cuda"), torch.full((4, 8), 7, dtype=torch.uint8, device="cuda")
    status = torch.full((4,), 7, dtype=torch.int32, device="cuda")
    dist, best = torch.full((4, 2), 7.0, dtype=torch.float64, device="cuda"), torch.full((4,), 7, dtype=torch.int32, device="cuda")
    const, const_dist = torch.full((4,), 7.0, device="cuda"), torch.full((4,), 7.0, dtype=torch.float64, device="cuda")
    counts = torch.full((4, 3), 7, dtype=torch.int32, device="cuda")
    p = lambda t: None if t is None else C_.c_void_p(t.data_ptr())  # noqa: E731

    def des(pop=4, D=8, gp_len=8, var_len=2, out_len=1, value=forest[0], out=desired, n_mates=3, mvalue=mates[0], mate_=mate):
        return lib_.evogp_hip_sr_desired_mid(pop, D, gp_len, var_len, out_len, p(value), p(forest[1]), p(forest[2]), p(X), n_mates, p(mvalue),
                                             p(mates[1]), p(mates[2]), p(mate_), p(pos), p(out), p(state), p(status), None)

    def mat(pop=4, D=8, gp_len=8, var_len=2, out_len=1, value=forest[0], out=dist, n_mates=3, mvalue=mates[0], mate_=mate, K=2):
        return lib_.evogp_hip_sr_agx_match(pop, D, gp_len, var_len, out_len, p(value), p(forest[1]), p(forest[2]), p(X), n_mates, p(mvalue),
                                           p(mates[1]), p(mates[2]), p(mate_), p(pos), K, p(libt), p(out), p(best), p(const), p(const_dist),
                                           p(counts), p(status), None)

    for f in (des, mat):
        for bad in (dict(pop=0), dict(D=0), dict(gp_len=0), dict(gp_len=1025), dict(var_len=0), dict(out_len=0), dict(n_mates=0)):
            assert f(**bad) == -1, (f.__name__, bad)
        assert f(value=None) == -2 and f(out=None) == -2 and f(mvalue=None) == -2 and f(mate_=None) == -2 and f(out_len=2) == -3
        assert f(n_mates=0, value=None) == -1 and f(out_len=2, mvalue=None) == -2   # the order: bad argument, null pointer, out_len
    assert mat(K=0) == -1 and mat(K=1025) == -1
    torch.cuda.synchronize()
    assert all((t == 7).all() for t in (desired, state, status, dist, best, const, const_dist, counts))   # nothing was launched
    assert des() == 0 and mat() == 0
    torch.cuda.synchronize()
    # x0 = 1 and the mate 5: the midpoint 3 on every row; the library of ones is 2 away on 8 rows
    assert (desired == 3).all() and (state == 0).all() and (status == 0).all() and (dist == 32).all() and (best == 0).all()
    assert (const == 3).all() and (const_dist == 0).all() and (counts == torch.tensor([8, 0, 0], device="cuda")).all()


# ---- Forest and ApproxGeometricCrossover end to end ------------------------------------------------------------------------------------
def _cuda_forest(exprs, width=H.L):
    return Forest(3, 1, *_dev(*rows(exprs, width)))


def _i32(*v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("name", sorted(H.PLANTED))
def test_a_planted_geometric_case(name):
    recipient, mate, pos, donor, child = H.PLANTED[name]
    X = H._data().abs().cuda()
    op = ApproxGeometricCrossover(X, library=_cuda_forest([V(0), donor, V(2), C(0.5)]))
    parents = _cuda_forest([recipient, mate])
    a, b = parents.batch_forward(X)[:, :, 0]
    best, dist, *_ = parents[:1].SR_midpoint_match(X, _i32(pos), parents, op.semantics, mate_index=_i32(1))
    assert int(best[0]) == 1 and float(dist[0, 1]) == 0.0, name
    new, found = op.apply(parents, _i32(0), _i32(1), _i32(pos))
    assert found.tolist() == [True], name
    for x, y in zip(new._tensors(), _cuda_forest([child])._tensors()):
        assert torch.equal(x, y), name
    assert np.array_equal(fbits(new.batch_forward(X)[0, :, 0].cpu().numpy()), fbits((0.5 * a + 0.5 * b).cpu().numpy())), name   # bit for bit


def test_the_forest_methods_and_the_constant_donor():
    X = H._data().cuda()
    lib = _cuda_forest([V(0), V(1), V(2)])
    parents = _cuda_forest([B(R.F_ADD, V(0), C(1.0)), B(R.F_ADD, V(0), C(4.0)), U(R.F_SIN, V(0))])
    pos = _i32(2, 0, 1)
    desired, state, status = parents.SR_midpoint_semantics(X, pos, parents, mate_index=_i32(1, 0, 5))
    assert status.tolist() == [0, 0, 4] and (desired[0] == 2.5).all() and torch.equal(desired[1], X[:, 0] + 2.5) and (state[:2] == 0).all() and (state[2] == 2).all()
    assert parents.SR_midpoint_semantics(X, pos, parents)[2].tolist() == [0, 0, 3]   # every tree with itself
    best, dist, const, const_dist, counts, _ = parents.SR_midpoint_match(X, pos, parents, lib, mate_index=_i32(1, 0, 5))
    assert best[2] == -1 and float(const[0]) == 2.5 and float(const_dist[0]) == 0.0 and counts.tolist() == [[24, 0, 0], [24, 0, 0], [0, 0, 24]]
    assert torch.equal(dist, parents.SR_midpoint_match(X, pos, parents, lib.batch_forward(X)[:, :, 0].contiguous(), mate_index=_i32(1, 0, 5))[1])
    new, found = ApproxGeometricCrossover(X, library=lib).apply(parents, _i32(0, 2), _i32(1, 0), _i32(2, 1))
    assert found.tolist() == [True, False]
    for x, y in zip(new._tensors(), _cuda_forest([B(R.F_ADD, V(0), C(2.5)), U(R.F_SIN, V(0))])._tensors()):
        assert torch.equal(x, y)   # the constant 2.5; the blocked tree copied bit for bit


def test_three_generations_of_genetic_programming():
    rng = np.random.default_rng(5)
    X = torch.from_numpy(rng.uniform(-2, 2, (256, 2)).astype(np.float32)).cuda()
    y = (X[:, :1] ** 2 + X[:, :1] * X[:, 1:2]).contiguous()
    d = GenerateDescriptor(max_tree_len=32, input_len=2, output_len=1, using_funcs=["+", "-", "*", "/", "sin"], max_layer_cnt=4, const_samples=[-1, 0, 1, 2])
    torch.manual_seed(9)
    op = ApproxGeometricCrossover(X, descriptor=d, library_size=100, fallback=DefaultCrossover())
    assert 2 < op.library.pop_size <= 102 and op.semantics.shape == (op.library.pop_size, 256)
    algo = GeneticProgramming(Forest.random_generate(200, d, keys=torch.tensor([1, 2], dtype=torch.uint32, device="cuda")), op, DefaultMutation(0.2, d),
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
