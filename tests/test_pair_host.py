"""CPU: the pairwise semantic moments above the kernel -- Forest.SR_pair_moments / semantic_distance, SemanticMate with its four
criteria, SemanticMateCrossover and ApproxGeometricCrossover(mate=) -- with the numpy restatement registered as a test-only CPU kernel
(tests/cpu_pair_ops.py), the forest invariants (dead words, row order, the population a tree stands in) of the op on it, and the argument
checks of the C entry points, which return before any launch.  Importing this module also puts the op into the invariance and binding
tables (tests/pair_tables.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cpu_agx_ops  # noqa: E402
import cpu_backprop_ops  # noqa: E402
import cpu_dedup_ops  # noqa: E402
import cpu_ops  # noqa: E402
import cpu_pair_ops  # noqa: E402
import cpu_semantic_ops  # noqa: E402
import forest_invariance as FI  # noqa: E402
import pair_ref as PR  # noqa: E402
import pair_tables as PT  # noqa: E402
import sr_grad_ref as R  # noqa: E402
import subtree_ref  # noqa: E402
from interval_cases import B, C, V, rows  # noqa: E402

for m in (cpu_ops, cpu_dedup_ops, cpu_semantic_ops, cpu_backprop_ops, cpu_agx_ops, cpu_pair_ops):
    m.register()

import evogp.algorithm  # noqa: E402
from evogp_amd import _lib  # noqa: E402
from evogp_amd.algorithm import (ApproxGeometricCrossover, DefaultCrossover, DefaultMutation, DefaultSelection, GeneticProgramming,  # noqa: E402
                                 SemanticMate, SemanticMateCrossover)
from evogp_amd.tree import Forest, GenerateDescriptor, set_default_device  # noqa: E402
from evogp_amd.tree import utils as _tree_utils  # noqa: E402

L, D = 16, 24
TREE = B(R.F_ADD, B(R.F_MUL, V(0), V(1)), V(2))   # T = x0 x1 + x2
# 0: T + 1   1: T - 1 (the complement)   2: a constant   3: NaN on every row   4: T   5: x0   6: T + 1 again
PLANTED = [B(R.F_ADD, TREE, C(1.0)), B(R.F_SUB, TREE, C(1.0)), C(2.0), B(R.F_DIV, V(0), C(0.0)), TREE, V(0), B(R.F_ADD, TREE, C(1.0))]


@pytest.fixture(autouse=True)
def _cpu_default_device():
    saved = _tree_utils._DEVICE
    set_default_device("cpu")
    yield
    _tree_utils._DEVICE = saved


def _bits(t):
    a = t.contiguous().numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


def _forest(exprs=PLANTED, inputs=3, width=L):
    return Forest(inputs, 1, *(torch.from_numpy(a) for a in rows(exprs, width)))


def _data():
    """small integers without zeros: T, T + 1 and T - 1 are exact in float32; the labels are T"""
    rng = np.random.default_rng(11)
    X = rng.choice(np.setdiff1d(np.arange(-8, 9), [0]), (D, 3)).astype(np.float32)
    return torch.from_numpy(X), torch.from_numpy(X[:, 0] * X[:, 1] + X[:, 2])


def _i32(*v):
    return torch.tensor(v, dtype=torch.int32)


def _same(a: Forest, b: Forest):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a._tensors(), b._tensors()))


def _descriptor(**kw):
    args = dict(max_tree_len=L, input_len=3, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=3, const_samples=[-1, 0, 1])
    args.update(kw)
    return GenerateDescriptor(**args)


# ---- the invariants of the op on the CPU stand-in, the tables ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FI.cases_for(PT.PAIRS))
def test_cpu_stand_in_keeps_the_invariants(case):
    FI.check(PT.PAIRS, FI.TABLE[PT.PAIRS], FI.build_case(case, min(40, FI.CASES[case]["pop"]), 50), "cpu")


def test_the_op_is_in_both_tables_and_the_classes_are_exported():
    assert FI.cases_for(PT.PAIRS) == ["arith_L64", "all_L64_v13", "all_L1024_v40"] and PT.PAIRS in PT.BC.TABLE
    for name, cls in (("SemanticMate", SemanticMate), ("SemanticMateCrossover", SemanticMateCrossover)):
        assert getattr(evogp.algorithm, name) is cls and name in evogp.algorithm.__all__
    assert issubclass(SemanticMateCrossover, DefaultCrossover) and type(SemanticMateCrossover(lambda p, l: (l, l))) is not DefaultCrossover


# ---- the Forest methods --------------------------------------------------------------------------------------------------------------------
def test_forest_methods_the_flat_form_and_mates():
    X, y = _data()
    f = _forest()
    own, mom = f.SR_pair_moments(X, y, _i32(0, 0, 4, 3, 9), _i32([1, 0, 3], [2, 5, 7], [4, 1, -1], [0, 0, 0], [0, 0, 0]))
    assert own.dtype == mom.dtype == torch.float64 and own.shape == (5,) and mom.shape == (5, 3, 3)
    assert own[:3].tolist() == [D, D, 0.0] and own[3:].isnan().all()
    assert mom[0, 0].tolist() == [D, -D, 4 * D] and mom[0, 1].tolist() == [D, D, 0.0] and mom[0, 2].isnan().all()
    assert mom[2, 0].tolist() == [0.0, 0.0, 0.0] and mom[2, 1].tolist() == [D, 0.0, D] and mom[2, 2].isnan().all() and mom[1, 2].isnan().all()
    assert mom[3:].isnan().all(), "an unusable or out-of-range first tree poisons the whole event"
    # (E,) candidates are read as (E, 1) and come back as (E, 3); int64 indices and (D, 1) labels are taken
    own1, mom1 = f.SR_pair_moments(X, y[:, None], torch.tensor([0, 0, 4]), torch.tensor([1, 2, 4]))
    assert mom1.shape == (3, 3) and np.array_equal(_bits(mom1), _bits(mom[:3, 0])) and np.array_equal(_bits(own1), _bits(own[:3]))
    # labels None: the moments of the predictions themselves
    own0, mom0 = f.SR_pair_moments(X, None, _i32(5), _i32([5, 2]))
    sxx = float((X[:, 0].double() ** 2).sum())
    assert own0.tolist() == [sxx] and mom0[0, 0].tolist() == [sxx, sxx, 0.0] and mom0[0, 1, 0] == 4.0 * D
    # mates: candidates index another forest, of another width
    mates = _forest([C(2.0), B(R.F_SUB, TREE, C(1.0))], width=32)
    ownm, momm = f.SR_pair_moments(X, y, _i32(0, 0), _i32([1, 0], [0, 2]), mates=mates)
    assert np.array_equal(_bits(momm[0, 0]), _bits(mom[0, 0])) and np.array_equal(_bits(momm[0, 1]), _bits(mom[1, 0])) and momm[1, 1].isnan().all()
    # the distance
    dist = f.semantic_distance(X, _i32(0, 0, 4, 0), _i32(1, 0, 0, 3))
    assert dist.dtype == torch.float64 and dist[:3].tolist() == [np.sqrt(4 * D), 0.0, np.sqrt(D)] and dist[3].isnan()
    assert f.semantic_distance(X, _i32(0), _i32(1), mates=mates).tolist() == [np.sqrt(4 * D)]
    # no events: empty outputs, nothing launched
    n0 = dict(cpu_pair_ops.calls)
    e_own, e_mom = f.SR_pair_moments(X, y, torch.zeros(0, dtype=torch.int32), torch.zeros((0, 4), dtype=torch.int32))
    assert e_own.shape == (0,) and e_mom.shape == (0, 4, 3)


def test_every_refusal_comes_before_the_first_launch():
    X, y = _data()
    f = _forest()
    first, cand = _i32(0, 1), _i32([1, 2], [0, 3])
    multi = Forest(3, 2, *f._tensors())
    n0 = dict(cpu_pair_ops.calls)
    for call, match in (
            (lambda: multi.SR_pair_moments(X, y, first, cand), "single-output"),
            (lambda: multi.semantic_distance(X, first, first), "single-output"),
            (lambda: f.SR_pair_moments(X, y, first, cand, mates=multi), "single-output"),
            (lambda: f.SR_pair_moments(X, y, first, cand, mates=_forest([V(0)], inputs=2)), "3 inputs"),
            (lambda: f.SR_pair_moments(X, y, first, cand, mates="forest"), "mates"),
            (lambda: f.SR_pair_moments(X, y, first, torch.zeros((2, 17), dtype=torch.int32)), "1 to 16 candidates"),
            (lambda: f.SR_pair_moments(X, y, first, torch.zeros((2, 0), dtype=torch.int32)), "1 to 16 candidates"),
            (lambda: f.SR_pair_moments(X, y, first, _i32([1, 2])), "candidates shape"),
            (lambda: f.SR_pair_moments(X, y, first, torch.zeros((2, 2, 2), dtype=torch.int32)), "candidates shape"),
            (lambda: f.SR_pair_moments(X, y, cand, cand), "first shape"),
            (lambda: f.SR_pair_moments(X, y, first.float(), cand), "integers"),
            (lambda: f.SR_pair_moments(X, y, first, cand.double()), "integers"),
            (lambda: f.SR_pair_moments(X, y[:-1], first, cand), "labels shape"),
            (lambda: f.SR_pair_moments(X, torch.stack([y, y], 1), first, cand), "labels shape"),
            (lambda: f.SR_pair_moments(X[:, :2], y, first, cand), "inputs shape"),
            (lambda: f.semantic_distance(X, first, cand), "second shape"),
            (lambda: f.semantic_distance(X, first, _i32(0, 1, 2)), "candidates shape")):
        with pytest.raises(ValueError, match=match):
            call()
    assert cpu_pair_ops.calls == n0


# ---- the chooser -----------------------------------------------------------------------------------------------------------------------------
def _chooser(criterion, **kw):
    X, y = _data()
    return SemanticMate(X, y, criterion=criterion, **kw)


@pytest.mark.parametrize("criterion", PR.CRITERIA)
def test_the_chooser_on_a_planted_population(criterion):
    f = _forest()
    left = _i32(0, 6)
    cand = _i32([0, 2, 3, 1, 5], [2, 3, 6, 5, 1])   # itself, a constant, an all-NaN tree, the complement, another tree
    right, score = _chooser(criterion).choose(f, left, cand)
    assert right.dtype == torch.int32 and score.dtype == torch.float64
    if criterion == "competent":
        assert right.tolist()[0] != 0 and right.tolist()[1] != 6 and torch.isfinite(score).all(), "never the tree itself (Sdd = 0 scores +inf)"
    else:
        assert right.tolist() == [1, 1], "T - 1 is the complement of T + 1 under the labels T"
        assert score.tolist() == {"midpoint": [0.0, 0.0], "blend": [0.0, 0.0], "angle": [-1.0, -1.0]}[criterion]
    X, y = _data()
    own, mom = f.SR_pair_moments(X, y, left, cand)
    want_right, want_score, _ = PR.choose(PR.scores(criterion, own.numpy(), mom.numpy()), cand.numpy())
    assert right.tolist() == want_right.tolist() and np.allclose(score.numpy(), want_score, rtol=1e-15, atol=0)
    s = _chooser(criterion).scores(own, mom)
    assert np.array_equal(np.isinf(s.numpy()), np.isinf(PR.scores(criterion, own.numpy(), mom.numpy()))) and bool(torch.isinf(s[:, [2, 1]][[0, 1], [0, 1]]).all())


def test_ties_all_inf_a_callable_and_the_drawn_candidates():
    f = _forest()
    mate = _chooser("midpoint")
    right, score = mate.choose(f, _i32(0, 0, 3, 0), _i32([6, 0, 6], [3, 3, 3], [0, 1, 2], [3, 1, 1]))
    assert right.tolist() == [6, 3, 0, 1] and score.tolist() == [float(D), float("inf"), float("inf"), 0.0]
    # a callable: the farthest candidate
    far = _chooser(lambda own, mom: -mom[..., 2])
    right, score = far.choose(f, _i32(0), _i32([0, 4, 1, 3]))
    assert right.tolist() == [1] and score.tolist() == [-4.0 * D] and score.dtype == torch.float64
    # drawn candidates: uniform indices from torch's generator, then choose()
    torch.manual_seed(3)
    drawn = mate(f, _i32(0, 0, 4, 5))
    torch.manual_seed(3)
    cand = torch.randint(0, 7, (4, 8), dtype=torch.int32)
    again = mate.choose(f, _i32(0, 0, 4, 5), cand)
    assert torch.equal(drawn[0], again[0]) and torch.equal(drawn[1], again[1])
    for bad in (dict(candidates=0), dict(candidates=17), dict(candidates=2.0), dict(criterion="nearest")):
        with pytest.raises(ValueError, match="candidates|criterion"):
            SemanticMate(*_data(), **bad)
    with pytest.raises(ValueError, match="labels"):
        SemanticMate(_data()[0], torch.zeros(D + 1))
    assert SemanticMate(_data()[0]).labels is None


# ---- the crossovers --------------------------------------------------------------------------------------------------------------------------
class _Recording:
    def __init__(self, mate):
        self.mate, self.seen = mate, []

    def __call__(self, parents, left):
        right, score = self.mate(parents, left)
        self.seen.append((left.clone(), right.clone()))
        return right, score


def test_semantic_mate_crossover_breeds_from_the_chosen_right_parent():
    X, y = _data()
    d = _descriptor()
    forest = Forest.random_generate(40, d, keys=torch.tensor([1, 2]))
    survivors = torch.arange(0, 40, 2, dtype=torch.int32)
    rec = _Recording(SemanticMate(X, y, candidates=4, criterion="angle"))
    op = SemanticMateCrossover(rec)
    with np.errstate(all="ignore"):
        torch.manual_seed(5)
        child = op(forest, survivors, 30, torch.zeros(40))
        parents = forest[survivors]
        torch.manual_seed(5)
        left, right, left_pos, right_pos = op.pairs(parents, 30)
    assert torch.equal(rec.seen[0][1], right) and torch.equal(rec.seen[0][0], left) and torch.equal(rec.seen[1][1], right)
    sizes = parents.batch_subtree_size[:, 0]
    assert ((0 <= right_pos) & (right_pos < sizes[right.long()])).all() and ((0 <= left_pos) & (left_pos < sizes[left.long()])).all()
    assert _same(child, parents.crossover(left, right, left_pos, right_pos)) and child.pop_size == 30
    t, s = child.batch_node_type.numpy(), child.batch_subtree_size.numpy()
    assert all(subtree_ref.check_prefix_tree(t[i], s[i]) for i in range(30))
    # the left parents and left positions are DefaultCrossover.draw's
    torch.manual_seed(5)
    l0, _, lp0, _ = DefaultCrossover().draw(sizes, 20, 30, sizes.device)
    assert torch.equal(l0, left) and torch.equal(lp0, left_pos)
    with pytest.raises(ValueError, match="mate"):
        SemanticMateCrossover("midpoint")


def test_agx_without_a_mate_is_bit_identical_and_with_one_replaces_only_right():
    X, y = _data()
    d = _descriptor()
    forest = Forest.random_generate(40, d, keys=torch.tensor([3, 4]))
    survivors = torch.arange(0, 40, 2, dtype=torch.int32)
    fitness = torch.zeros(40)

    def run(**kw):
        torch.manual_seed(7)
        op = ApproxGeometricCrossover(X, descriptor=d.update(max_layer_cnt=2), library_size=40, fallback=DefaultCrossover(), **kw)
        torch.manual_seed(8)
        with np.errstate(all="ignore"):
            return op(forest, survivors, 30, fitness)

    n0 = dict(cpu_pair_ops.calls)
    plain, none = run(), run(mate=None)
    assert _same(plain, none) and cpu_pair_ops.calls == n0, "mate=None: the same draws, the same offspring, no call of the new op"
    rec = _Recording(SemanticMate(X, y, candidates=4))
    mated = run(mate=rec)
    assert cpu_pair_ops.calls["pair_moments"] == n0["pair_moments"] + 1 and mated.pop_size == 30
    torch.manual_seed(8)
    parents = forest[survivors]
    left, _, left_pos, _ = DefaultCrossover().draw(parents.batch_subtree_size[:, 0], 20, 30, "cpu")
    assert torch.equal(rec.seen[0][0], left), "the left parents are the ones the operator draws without a mate"
    t, s = mated.batch_node_type.numpy(), mated.batch_subtree_size.numpy()
    assert all(subtree_ref.check_prefix_tree(t[i], s[i]) for i in range(30))
    with pytest.raises(ValueError, match="mate"):
        ApproxGeometricCrossover(X, descriptor=d, mate="midpoint")


def test_the_default_pipeline_never_calls_the_new_op():
    from evogp_amd.pipeline import StandardPipeline
    from evogp_amd.problem import SymbolicRegression

    X, y = _data()
    d = _descriptor()
    n0 = dict(cpu_pair_ops.calls)
    with np.errstate(all="ignore"):
        for crossover in (DefaultCrossover(), ApproxGeometricCrossover(X, descriptor=d.update(max_layer_cnt=2), library_size=40, fallback=DefaultCrossover())):
            algo = GeneticProgramming(Forest.random_generate(40, d, keys=torch.tensor([1, 2])), crossover, DefaultMutation(0.2, d), DefaultSelection(0.3, 2))
            StandardPipeline(algo, SymbolicRegression(datapoints=X, labels=y[:, None]), is_show_details=False, generation_limit=2).run()
        assert cpu_pair_ops.calls == n0
        algo = GeneticProgramming(Forest.random_generate(40, d, keys=torch.tensor([1, 2])), SemanticMateCrossover(SemanticMate(X, y, candidates=3)),
                                  DefaultMutation(0.2, d), DefaultSelection(0.3, 2))
        StandardPipeline(algo, SymbolicRegression(datapoints=X, labels=y[:, None]), is_show_details=False, generation_limit=2).run()
    assert cpu_pair_ops.calls["pair_moments"] == n0["pair_moments"] + 2 and algo.forest.pop_size == 40


# ---- the C entry points -------------------------------------------------------------------------------------------------------------------
def test_c_entry_points_check_their_arguments():
    Lb = _lib.lib
    p = ctypes.c_void_p(16)   # never dereferenced: every call below returns from its argument checks
    M, W = Lb.evogp_hip_sr_pair_moments, Lb.evogp_hip_sr_pair_moments_workspace_bytes
    BAD, NULL = -1, -2

    def call(E=4, n=3, D_=8, vl=3, pa=5, la=32, pb=6, lb=64, ptrs=None, labels=p):
        a = [p] * 12 if ptrs is None else ptrs   # value_a type_a size_a value_b type_b size_b variables first candidates own moments workspace
        return M(E, n, D_, vl, pa, la, a[0], a[1], a[2], pb, lb, a[3], a[4], a[5], a[6], labels, a[7], a[8], a[9], a[10], a[11], None)

    for bad in (dict(n=0), dict(n=17), dict(D_=0), dict(vl=0), dict(pa=0), dict(pb=0), dict(la=0), dict(lb=0), dict(la=1025), dict(lb=1025),
                dict(E=2 ** 31), dict(D_=2 ** 31), dict(pa=2 ** 31), dict(pb=2 ** 31)):
        assert call(**bad) == BAD, bad
    for k in range(12):
        ptrs = [p] * 12
        ptrs[k] = None
        assert call(ptrs=ptrs) == NULL, k
    assert call(n=17, ptrs=[None] * 12) == BAD, "argument errors come before null pointers"
    # no events: nothing to launch and nothing to point at; the forests and the dataset are still checked
    assert call(E=0, ptrs=[p] * 7 + [None] * 5, labels=None) == 0 and call(E=0, ptrs=[None] + [p] * 11) == NULL and call(E=0, n=0) == BAD
    nbytes = ctypes.c_ulonglong(0)
    assert W(1000, 8, ctypes.byref(nbytes)) == 0 and 1000 <= nbytes.value <= 1024 + 256
    assert W(0, 8, ctypes.byref(nbytes)) == 0 and nbytes.value == 0
    assert W(4, 0, ctypes.byref(nbytes)) == BAD and W(4, 17, ctypes.byref(nbytes)) == BAD and W(2 ** 31, 1, ctypes.byref(nbytes)) == BAD
    assert W(4, 1, None) == NULL
    assert Lb.evogp_hip_abi_version() == _lib.ABI_VERSION
