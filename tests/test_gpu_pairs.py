"""GPU: pairwise semantic moments (csrc/sr_pair.hip) against the numpy restatement (tests/pair_ref.py) fed with ``batch_forward`` of the same
forest -- NaN words in exactly the restatement's positions, finite words within the derived bound (D + 8) 2^-53 sum |term|, no fitted
tolerance and no allowed-bad fraction -- on every shape of tests/pair_cases.py SHAPES; then, without any tolerance, what the pinned
reduction order promises: the words of a pair do not depend on the event, the slot, M, the neighbours, the population or the kernel that
took it; the symmetry of Sab and Sdd; Sbb against own; copies and repeated candidates; the rule of the unusable tree; determinism on one
stream and on two; the forest invariants and the binding contract; the chooser on the device against the restatement's; and five
generations of GeneticProgramming with a semantically chosen mate."""
import os
import sys

import numpy as np
import pytest
import torch

import evogp_amd  # noqa: F401  (registers the ops)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forest_invariance as FI  # noqa: E402
import pair_cases as PC  # noqa: E402
import pair_ref as PR  # noqa: E402
import pair_tables as PT  # noqa: E402
import semantic_ref as S  # noqa: E402
import subtree_ref  # noqa: E402

from evogp_amd.algorithm import (ApproxGeometricCrossover, DefaultCrossover, DefaultMutation, DefaultSelection, GeneticProgramming,  # noqa: E402
                                 SemanticMate)
from evogp_amd.pipeline import StandardPipeline  # noqa: E402
from evogp_amd.problem import SymbolicRegression  # noqa: E402
from evogp_amd.tree import Forest, GenerateDescriptor  # noqa: E402

pytestmark = pytest.mark.gpu
hip = torch.ops.evogp_hip


def _dev(*arrs):
    return [torch.from_numpy(np.array(a, order="C")).cuda() for a in arrs]   # (a copy: the shared arrays are read-only)


def moments(fa, X, y, first, cand, fb=None):
    """(own, moments) of the op as numpy arrays; fa, fb: (value, type, size) numpy forests"""
    a = _dev(*fa)
    b = a if fb is None else _dev(*fb)
    own, mom = hip.tree_SR_pair_moments(*a, *b, _dev(X)[0], None if y is None else _dev(y)[0], *_dev(np.asarray(first, np.int32),
                                                                                                         np.asarray(cand, np.int32)))
    return own.cpu().numpy(), mom.cpu().numpy()


_truth = {}


def truth(funcs, gp_len, pop, D, var_len=3):
    """(forest, X, y, P, usable): the register interpreter's predictions of a shared forest, once per forest and dataset"""
    key = (funcs, gp_len, pop, D, var_len)
    if key not in _truth:
        f = PC.pair_forest(funcs, gp_len, pop, var_len)
        X, y = PC.pair_data(D, var_len)
        P = Forest(var_len, 1, *_dev(*f)).batch_forward(_dev(X)[0])[:, :, 0].contiguous().cpu().numpy()
        _truth[key] = (f, X, y, P, PR.usable(P, S.formed_mask(f[1], f[2])))
    return _truth[key]


def _u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_u64(a), _u64(b))


# ---- 1. against the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", PC.SHAPES, ids=PC.shape_id)
def test_moments_match_the_restatement(shape):
    funcs, gp_len, pop, E, M, D, var_len, labels = shape
    f, X, y, P, u = truth(funcs, gp_len, pop, D, var_len)
    y = y if labels else None
    first, cand = PC.case_events(shape)
    want_own, want, own_mag, mag = PR.pair_moments(P, u, P, u, y, first, cand)
    PC.check_condition(shape, want)
    own, mom = moments(f, X, y, first, cand)
    assert own.shape == (E,) and mom.shape == (E, M, 3) and own.dtype == mom.dtype == np.float64
    assert np.array_equal(np.isnan(own), np.isnan(want_own)), np.flatnonzero(np.isnan(own) != np.isnan(want_own))[:8]
    assert np.array_equal(np.isnan(mom), np.isnan(want)), np.argwhere(np.isnan(mom) != np.isnan(want))[:8]
    ok, oko = ~np.isnan(want), ~np.isnan(want_own)
    assert np.isfinite(mom[ok]).all() and np.isfinite(own[oko]).all()
    err, lim = np.abs(mom - want)[ok], PR.bound(D, mag)[ok]
    erro, limo = np.abs(own - want_own)[oko], PR.bound(D, own_mag)[oko]
    worst = max([float((err / np.maximum(lim, 1e-300)).max()) if err.size else 0.0, float((erro / np.maximum(limo, 1e-300)).max()) if erro.size else 0.0])
    print(f"{PC.shape_id(shape)}: {int(ok.sum()) // 3} finite pairs of {E * M}, worst error / bound {worst:.3g}")
    assert (err <= lim).all(), np.argwhere(np.abs(mom - want) > PR.bound(D, mag))[:8]
    assert (erro <= limo).all()


# ---- 2. bit for bit: the words of a pair depend on the pair and the dataset alone ---------------------------------------------------------
@pytest.mark.parametrize("D", [257, 1100])
def test_a_pair_keeps_its_bits_in_another_event_slot_m_neighbourhood_and_population(D):
    f, X, y, P, u = truth("all", 64, 200, D)
    rng = np.random.default_rng(D)
    firsts = rng.choice(np.flatnonzero(u), 12, replace=False)
    cands = rng.choice(np.arange(200), (12, 4))          # usable or not: a NaN word keeps its place as well
    own, mom = moments(f, X, y, firsts, cands)
    assert np.isfinite(own).all() and np.isfinite(mom).all(axis=2).sum() >= 12
    # every pair alone, in a shuffled order
    order = rng.permutation(48)
    own1, mom1 = moments(f, X, y, np.repeat(firsts, 4)[order], cands.reshape(-1)[order][:, None])
    assert _same_bits(mom1[:, 0], mom.reshape(48, 3)[order]) and _same_bits(own1, np.repeat(own, 4)[order])
    # under M = 16, in other slots, next to other candidates
    slots = np.array([3, 7, 8, 15])
    wide = rng.integers(0, 200, (12, 16))
    wide[:, slots] = cands
    own16, mom16 = moments(f, X, y, firsts, wide)
    assert _same_bits(mom16[:, slots], mom) and _same_bits(own16, own)
    # the candidates moved to a mates forest of another gp_len and another size, in another order
    used = np.unique(cands)
    perm = rng.permutation(len(used))
    mates = tuple(np.zeros((len(used), 1024), a.dtype) for a in f)
    for m, a in zip(mates, f):
        m[:, :64] = a[used[perm]]
    where = np.empty(200, np.int64)
    where[used[perm]] = np.arange(len(used))
    ownm, momm = moments(f, X, y, firsts, where[cands], fb=mates)
    assert _same_bits(momm, mom) and _same_bits(ownm, own)
    # ... and the first trees too: both sides from the wide forest
    allm = tuple(np.zeros((200, 1024), a.dtype) for a in f)
    for m, a in zip(allm, f):
        m[:, :64] = a
    ownw, momw = moments(allm, X, y, firsts, cands)
    assert _same_bits(momw, mom) and _same_bits(ownw, own)


def test_sab_and_sdd_are_symmetric_and_sbb_is_the_candidates_own():
    f, X, y, P, u = truth("all", 1024, 200, 1100)
    rng = np.random.default_rng(2)
    a, b = rng.integers(0, 200, 150), rng.integers(0, 200, 150)
    own_a, ab = moments(f, X, y, a, b[:, None])
    own_b, ba = moments(f, X, y, b, a[:, None])
    assert np.isfinite(ab).all(axis=(1, 2)).sum() >= 30
    assert _same_bits(ab[:, 0, 1:], ba[:, 0, 1:])
    both = np.isfinite(ab[:, 0, 0])
    assert _same_bits(ab[both, 0, 0], own_b[both]) and _same_bits(ba[both, 0, 0], own_a[both])


def test_the_same_words_come_out_of_both_kernels():
    """rows deeper than the register stack (a 79-node comb, T + 0 * S) send their whole event to the scratch-stack kernel"""
    f, X, y, P, u = truth("all", 1024, 200, 1100)
    comb, deep, t, copy = PC.COMB_ROW, PC.DEEP_ROW, PC.T_ROW, PC.COPY_ROW
    other = int(np.flatnonzero(u)[np.flatnonzero(u) >= 24][0])   # a usable random tree
    assert u[[comb, deep, t, copy, 0]].all() and f[2][comb, 0] == 79
    first = np.array([comb, t, 0, 0, deep, t])
    cand = np.array([[t, 0, deep], [0, copy, t], [t, copy, other], [t, comb, other], [comb, t, 0], [comb, 0, copy]])
    own, mom = moments(f, X, y, first, cand)
    # event 2 runs in the register kernel, event 3 (the same first tree, the comb among its candidates) in the scratch-stack kernel
    assert _same_bits(mom[2, 0], mom[3, 0]) and _same_bits(mom[2, 2], mom[3, 2]) and _same_bits(own[2], own[3])
    # Sbb of a candidate is the own word of the same tree, whichever kernel produced either
    assert _same_bits(mom[0, 0, 0], own[1]) and _same_bits(mom[2, 0, 0], own[1]) and _same_bits(mom[0, 1, 0], own[2])
    assert _same_bits(mom[1, 0, 0], own[2]) and _same_bits(mom[4, 0, 0], own[0]) and _same_bits(mom[0, 2, 0], own[4]) and _same_bits(mom[5, 0, 0], own[0])
    # (t, 0): event 1 in the register kernel, (0, t): events 2 and 3; (comb, t) against (t, comb)
    assert _same_bits(mom[1, 0, 1:], mom[2, 0, 1:]) and _same_bits(mom[0, 0, 1:], mom[5, 0, 1:])
    # a structural copy: Sdd is zero and the other words are the first tree's own
    assert mom[1, 1, 2] == 0.0 and mom[1, 2, 2] == 0.0 and _same_bits(mom[1, 1, :2], [own[1], own[1]]) and _same_bits(mom[1, 1], mom[1, 2])
    # T + 0 * S predicts what T predicts
    assert mom[4, 1, 2] == 0.0 and _same_bits(own[4], own[1])
    want = PR.pair_moments(P, u, P, u, y, first, cand)
    assert np.isfinite(mom).all() and (np.abs(mom - want[1]) <= PR.bound(1100, want[3])).all()


def test_a_repeated_candidate_gives_repeated_columns():
    f, X, y, P, u = truth("all", 64, 200, 257)
    rng = np.random.default_rng(4)
    first = rng.integers(0, 200, 70)
    c = rng.integers(0, 200, (70, 2))
    cand = np.stack([c[:, 0], c[:, 1], c[:, 0], c[:, 0], c[:, 1]], 1)
    _, mom = moments(f, X, None, first, cand)
    assert np.isfinite(mom).any() and _same_bits(mom[:, 0], mom[:, 2]) and _same_bits(mom[:, 0], mom[:, 3]) and _same_bits(mom[:, 1], mom[:, 4])


# ---- 3. the unusable tree -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gp_len,D", [(64, 65), (1024, 1100)])
def test_an_unusable_tree_poisons_exactly_its_words(gp_len, D):
    f, X, y, P, u = truth("all", gp_len, 200, D)
    inf_last, bad, nan_row, t = PC.INF_LAST_ROW, PC.MALFORMED[0], PC.NAN_ROW, PC.T_ROW
    assert np.isfinite(P[inf_last, :-1]).all() and np.isinf(P[inf_last, -1]) and u[[0, t, PC.COPY_ROW]].all()
    first = np.array([0, inf_last, bad, 0, 200, t, -1, nan_row, 0])
    cand = np.array([[t, inf_last, 0], [0, t, 0], [0, t, 0], [bad, -1, t], [0, 0, 0], [200, PC.MALFORMED[1], PC.COPY_ROW], [t, t, t], [t, 0, 0],
                     [2 ** 31 - 1, -2 ** 31, nan_row]])
    own, mom = moments(f, X, y, first, cand)
    assert np.isnan(own).tolist() == [False, True, True, False, True, False, True, True, False]
    assert np.isnan(mom).all(axis=2).tolist() == [[False, True, False], [True] * 3, [True] * 3, [True, True, False], [True] * 3, [True, True, False],
                                                  [True] * 3, [True] * 3, [True] * 3]
    assert (np.isnan(mom).all(axis=2) == np.isnan(mom).any(axis=2)).all()
    clean_own, clean = moments(f, X, y, np.array([0, 0, t]), np.array([[t, 0], [t, t], [PC.COPY_ROW, t]]))
    assert _same_bits(mom[0, 0], clean[0, 0]) and _same_bits(mom[0, 2], clean[0, 1]) and _same_bits(mom[3, 2], clean[0, 0])
    assert _same_bits(mom[5, 2], clean[2, 0]) and _same_bits(own[[0, 3, 5, 8]], clean_own[[0, 0, 2, 0]])


# ---- 4. determinism -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gp_len", [64, 1024])
def test_two_calls_and_two_streams_give_the_same_bits(gp_len):
    f, X, y, P, u = truth("all", gp_len, 200, 1100)
    first, cand = PC.events(np.random.default_rng(9), 300, 8, 200)
    args = _dev(*f) * 2 + _dev(X, y, first, cand)

    def call():
        return hip.tree_SR_pair_moments(*args)

    one, two = call(), call()
    outs = []
    for _ in range(2):
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            outs.append(call())
        stream.synchronize()
    torch.cuda.synchronize()
    assert torch.isfinite(one[1]).any()
    for other in (two, outs[0], outs[1]):
        assert all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in zip(one, other))


# ---- 5. the tables --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FI.cases_for(PT.PAIRS))
def test_op_keeps_the_invariants(case):
    FI.check(PT.PAIRS, FI.TABLE[PT.PAIRS], FI.build_case(case), "cuda")
    torch.cuda.synchronize()


def test_binding_contract():
    PT.BC.test_valid_call_and_one_fault_at_a_time(PT.PAIRS)
    row = PT.ROWS[PT.PAIRS]()
    own, mom = hip.tree_SR_pair_moments(*[a for _, a in row["args"]])
    # CONST 1.0 against CONST 1.0 under labels of 0.5 on 8 rows
    assert own.cpu().tolist() == [2.0] * 5 and mom.cpu().tolist() == [[[2.0, 2.0, 0.0]] * 2] * 5


# ---- 6. the Forest methods and the chooser -----------------------------------------------------------------------------------------------------
def test_forest_methods_on_the_device():
    f, X, y, P, u = truth("all", 64, 200, 257)
    forest = Forest(3, 1, *_dev(*f))
    Xd, yd = _dev(X, y)
    first, cand = PC.events(np.random.default_rng(1), 65, 3, 200)
    own, mom = forest.SR_pair_moments(Xd, yd, *_dev(first, cand))
    wo, wm = moments(f, X, y, first, cand)
    assert _same_bits(own.cpu().numpy(), wo) and _same_bits(mom.cpu().numpy(), wm)
    own1, mom1 = forest.SR_pair_moments(Xd, yd[:, None], torch.from_numpy(first.astype(np.int64)).cuda(), _dev(cand[:, 1])[0])
    assert mom1.shape == (65, 3) and _same_bits(mom1.cpu().numpy(), wm[:, 1]) and _same_bits(own1.cpu().numpy(), wo)
    dist = forest.semantic_distance(Xd, *_dev(first, cand[:, 0]))
    _, plain = moments(f, X, None, first, cand[:, :1])
    assert dist.dtype == torch.float64 and _same_bits(dist.cpu().numpy(), np.sqrt(plain[:, 0, 2]))
    empty = forest.SR_pair_moments(Xd, yd, torch.zeros(0, dtype=torch.int32, device="cuda"), torch.zeros((0, 4), dtype=torch.int32, device="cuda"))
    assert empty[0].shape == (0,) and empty[1].shape == (0, 4, 3) and empty[1].dtype == torch.float64


@pytest.mark.parametrize("criterion", PR.CRITERIA)
def test_the_chooser_on_the_device_equals_the_restatements(criterion):
    f, X, y, P, u = truth("all", 64, 200, 257)
    forest = Forest(3, 1, *_dev(*f))
    left, cand = PC.events(np.random.default_rng(6), 300, 8, 200)
    mate = SemanticMate(*_dev(X, y), candidates=8, criterion=criterion)
    right, score = mate.choose(forest, *_dev(left, cand))
    own, mom = moments(f, X, y, left, cand)
    want_right, want_score, _ = PR.choose(PR.scores(criterion, own, mom), cand)
    assert right.dtype == torch.int32 and score.dtype == torch.float64
    assert np.array_equal(right.cpu().numpy(), want_right)
    got = score.cpu().numpy()
    assert np.array_equal(np.isinf(got), np.isinf(want_score)) and np.isfinite(got).sum() >= 100
    fin = np.isfinite(got)
    assert np.allclose(got[fin], want_score[fin], rtol=1e-13, atol=0)
    drawn, _ = mate(forest, _dev(left)[0])
    assert drawn.shape == (300,) and int(drawn.min()) >= 0 and int(drawn.max()) < 200


# ---- 7. end to end ---------------------------------------------------------------------------------------------------------------------------
def test_five_generations_with_a_semantically_chosen_mate():
    rng = np.random.default_rng(8)
    X = torch.from_numpy(rng.uniform(-2, 2, (128, 3)).astype(np.float32)).cuda()
    y = (X[:, :1] * X[:, 1:2] + X[:, 2:3] / (1.5 + X[:, :1] ** 2)).contiguous()
    d = GenerateDescriptor(max_tree_len=64, input_len=3, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=5, const_samples=[-1, 0, 1, 2])
    crossover = ApproxGeometricCrossover(X, descriptor=d.update(max_layer_cnt=3), mate=SemanticMate(X, y, candidates=8, criterion="midpoint"),
                                         fallback=DefaultCrossover())
    algo = GeneticProgramming(Forest.random_generate(512, d, keys=torch.tensor([1, 2], dtype=torch.uint32, device="cuda")), crossover,
                              DefaultMutation(0.2, d.update(max_layer_cnt=3)), DefaultSelection(0.3, 4))
    pipe = StandardPipeline(algo, SymbolicRegression(datapoints=X, labels=y), generation_limit=5, is_show_details=False)
    best = pipe.run()
    assert best is pipe.best_tree and algo.forest.pop_size == 512 and np.isfinite(float(pipe.best_fitness))
    t, s = algo.forest.batch_node_type.cpu().numpy(), algo.forest.batch_subtree_size.cpu().numpy()
    assert all(subtree_ref.check_prefix_tree(t[i], s[i]) for i in range(512))
