"""CPU: approximately geometric semantic crossover above the kernel -- the argument checks of Forest.SR_midpoint_semantics /
SR_midpoint_match, the library shared between ApproxGeometricCrossover and SemanticBackpropMutation, and the operator itself (planted
geometric cases, the constant donor, the fallback, a pair of one tree with itself, generations of GeneticProgramming), with the numpy
restatement registered as a test-only CPU kernel (tests/cpu_agx_ops.py), and the forest invariants (dead words, row order, slices) of
the two ops on it.  Importing this module also puts the two ops into the invariance and binding tables (tests/agx_tables.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import agx_tables as AT  # noqa: E402
import cpu_agx_ops  # noqa: E402
import cpu_backprop_ops  # noqa: E402
import cpu_dedup_ops  # noqa: E402
import cpu_ops  # noqa: E402
import cpu_semantic_ops  # noqa: E402
import forest_invariance as FI  # noqa: E402
import sr_grad_ref as R  # noqa: E402
from interval_cases import B, C, U, V, rows  # noqa: E402

cpu_ops.register()
cpu_dedup_ops.register()
cpu_semantic_ops.register()
cpu_backprop_ops.register()
cpu_agx_ops.register()

import evogp.algorithm  # noqa: E402
from evogp_amd.algorithm import (ApproxGeometricCrossover, BaseCrossover, DefaultCrossover, DefaultMutation, DefaultSelection,  # noqa: E402
                                 GeneticProgramming, SemanticBackpropMutation, SemanticLibrary)
from evogp_amd.tree import Forest, GenerateDescriptor, set_default_device  # noqa: E402
from evogp_amd.tree import utils as _tree_utils  # noqa: E402

L = 16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "agx_parent_backprop_mutation.npz")


@pytest.fixture(autouse=True)
def _cpu_default_device():
    saved = _tree_utils._DEVICE
    set_default_device("cpu")
    yield
    _tree_utils._DEVICE = saved


def _bits(t):
    a = t.numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _forest(exprs, inputs=3, width=L):
    return Forest(inputs, 1, *(torch.from_numpy(a) for a in rows(exprs, width)))


def _data(n=24):
    """small integers without zeros: sums, halves of sums, products and the quotients used below are exact in float32"""
    rng = np.random.default_rng(11)
    return torch.from_numpy(rng.choice(np.setdiff1d(np.arange(-8, 9), [0]), (n, 3)).astype(np.float32))


def _descriptor(**kw):
    args = dict(max_tree_len=L, input_len=3, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=3, const_samples=[-1, 0, 1])
    args.update(kw)
    return GenerateDescriptor(**args)


def _same(a: Forest, b: Forest):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a._tensors(), b._tensors()))


def _copy(f: Forest):
    return Forest(f.input_len, f.output_len, *(a.clone() for a in f._tensors()))


def _i32(*v):
    return torch.tensor(v, dtype=torch.int32)


# ---- the invariants of the two ops on the CPU stand-ins ------------------------------------------------------------------------------
@pytest.mark.parametrize("op,case", [(op, c) for op in (AT.DESIRED_MID, AT.AGX_MATCH) for c in FI.cases_for(op)])
def test_cpu_stand_in_keeps_the_invariants(op, case):
    FI.check(op, FI.TABLE[op], FI.build_case(case, min(40, FI.CASES[case]["pop"]), 50), "cpu")


def test_the_ops_are_in_both_tables_and_the_class_is_exported():
    assert FI.cases_for(AT.DESIRED_MID) == FI.cases_for(AT.AGX_MATCH) == ["arith_L64", "all_L64_v13", "all_L1024_v40"]
    assert AT.DESIRED_MID in AT.BC.TABLE and AT.AGX_MATCH in AT.BC.TABLE
    assert evogp.algorithm.ApproxGeometricCrossover is ApproxGeometricCrossover and issubclass(ApproxGeometricCrossover, BaseCrossover)
    assert "ApproxGeometricCrossover" in evogp.algorithm.__all__


# ---- the two Forest methods -------------------------------------------------------------------------------------------------------------
def test_forest_methods_and_their_argument_checks():
    X = _data()
    f = _forest([B(R.F_ADD, V(0), V(1)), U(R.F_SIN, V(0)), V(1)])
    mates = _forest([B(R.F_ADD, V(0), V(2)), V(2), V(0)])
    pos = _i32(2, 1, 0)
    desired, state, status = f.SR_midpoint_semantics(X, pos, mates)
    assert desired.shape == (3, 24) and desired.dtype == torch.float32 and state.dtype == torch.uint8 and status.tolist() == [0, 3, 0]
    assert torch.equal(desired[0], 0.5 * X[:, 1] + 0.5 * X[:, 2]) and torch.equal(desired[2], 0.5 * X[:, 1] + 0.5 * X[:, 0])
    assert desired[1].isnan().all() and (state[1] == 2).all()
    # mate_index: another pairing, int64 as well; its range is the kernel's to report
    again = f.SR_midpoint_semantics(X, pos.to(torch.int64), mates, mate_index=torch.tensor([0, 1, 2]))
    assert all(torch.equal(a, b) or (a.isnan() == b.isnan()).all() for a, b in zip(again, (desired, state, status)))
    d2, _, s2 = f.SR_midpoint_semantics(X, pos, mates[:2], mate_index=_i32(1, 0, 2))
    assert s2.tolist() == [0, 3, 4] and torch.equal(d2[0], (0.5 * (X[:, 0] + X[:, 1]) + 0.5 * X[:, 2]) - X[:, 0])
    lib = torch.stack([X[:, 0], 0.5 * X[:, 1] + 0.5 * X[:, 2], X[:, 2]])
    best, dist, const, const_dist, counts, status2 = f.SR_midpoint_match(X, pos, mates, lib)
    assert best.tolist()[:2] == [1, -1] and dist.shape == (3, 3) and dist.dtype == torch.float64 and float(dist[0, 1]) == 0.0
    assert counts.tolist() == [[24, 0, 0], [0, 0, 24], [24, 0, 0]] and torch.equal(status, status2) and const_dist.dtype == torch.float64
    libf = _forest([V(0), V(1), V(2)])   # a library forest: its semantics are batch_forward's
    assert f.SR_midpoint_match(X, pos, mates, libf)[1].shape == (3, 3)
    n0 = dict(cpu_agx_ops.calls)
    multi = Forest(3, 2, *f._tensors())
    for call in (lambda: multi.SR_midpoint_semantics(X, pos, mates), lambda: multi.SR_midpoint_match(X, pos, mates, lib),
                 lambda: f.SR_midpoint_semantics(X, pos, Forest(3, 2, *mates._tensors())),
                 lambda: f.SR_midpoint_match(X, pos, Forest(3, 2, *mates._tensors()), lib)):
        with pytest.raises(ValueError, match="single-output"):
            call()
    for bad, msg in ((_forest([V(0)] * 3, inputs=2), "input_len"), (_forest([V(0)] * 3, width=32), "max_tree_len"), (mates[:2], "mate_index"),
                     ("mates", "single-output Forest")):
        with pytest.raises(ValueError, match=msg):
            f.SR_midpoint_semantics(X, pos, bad)
        with pytest.raises(ValueError, match=msg):
            f.SR_midpoint_match(X, pos, bad, lib)
    for bad in (pos[:2], pos[None], pos.to(torch.float32)):
        with pytest.raises(ValueError, match="positions"):
            f.SR_midpoint_semantics(X, bad, mates)
        with pytest.raises(ValueError, match="mate_index"):
            f.SR_midpoint_match(X, pos, mates, lib, mate_index=bad)
    with pytest.raises(ValueError, match="mate_index"):
        f.SR_midpoint_semantics(X, pos, mates, mate_index=torch.tensor([True, False, True]))
    with pytest.raises(AssertionError, match="inputs shape"):
        f.SR_midpoint_semantics(X[:, :2], pos, mates)
    for bad in (X.t()[:, :5].contiguous(), X[:, 0], torch.zeros((0, 24)), torch.zeros((1025, 24))):
        with pytest.raises(ValueError, match="library"):
            f.SR_midpoint_match(X, pos, mates, bad)
    with pytest.raises(ValueError, match="library forest"):
        f.SR_midpoint_match(X, pos, mates, _forest([V(0)], inputs=2))
    assert cpu_agx_ops.calls == n0   # every check comes before the first launch


# ---- the constructor and the shared library -----------------------------------------------------------------------------------------
def test_the_constructor_and_its_errors():
    X = _data()
    torch.manual_seed(3)
    with np.errstate(all="ignore"):
        op = ApproxGeometricCrossover(X, descriptor=_descriptor(), library_size=100)
    assert 3 < op.library.pop_size < 103 and op.semantics.shape == (op.library.pop_size, 24) and op.fallback is None and op.allow_constant
    assert ApproxGeometricCrossover(X, descriptor=_descriptor(), library_size=0).library.pop_size == 3
    for kw, msg in ((dict(), "library or a descriptor"), (dict(descriptor=_descriptor(input_len=2)), "descriptor should"),
                    (dict(library=_forest([V(0)], inputs=2)), "library should"), (dict(descriptor=_descriptor(), fallback=object()), "fallback"),
                    (dict(descriptor=_descriptor(), fallback=DefaultMutation(0.1, _descriptor())), "fallback"),
                    (dict(descriptor=_descriptor(), library_size=-1), "library_size")):
        with pytest.raises(ValueError, match=msg):
            ApproxGeometricCrossover(X, **kw)
    for bad in (X[:, 0], torch.zeros((0, 3)), [[1.0, 2.0, 3.0]]):
        with pytest.raises(ValueError, match="datapoints"):
            ApproxGeometricCrossover(bad, descriptor=_descriptor())
    with pytest.raises(ValueError, match="shared library"):
        ApproxGeometricCrossover(X[:5], library=op.semantic_library)
    wide = ApproxGeometricCrossover(X, library=_forest([V(0)], width=32))
    n0 = dict(cpu_agx_ops.calls)
    with pytest.raises(ValueError, match="max_tree_len"):
        wide(_forest([V(1), V(2)]), torch.tensor([0, 1]), 4, torch.zeros(2))
    with pytest.raises(ValueError, match="one output"):
        op(Forest(3, 2, *_forest([V(1), V(2)])._tensors()), torch.tensor([0, 1]), 4, torch.zeros(2))
    assert cpu_agx_ops.calls == n0


def test_one_library_object_reaches_both_operators():
    X = _data()
    y = X[:, :1].contiguous()
    shared = SemanticLibrary(X, library=_forest([V(0), V(1), V(2)]))
    cross = ApproxGeometricCrossover(X, library=shared)
    mut = SemanticBackpropMutation(1.0, X, y, library=shared)
    assert cross.semantic_library is shared is mut.semantic_library and cross.library.pop_size == 3 == mut.library.pop_size
    mut.update_library(_forest([B(R.F_ADD, V(0), V(1)), B(R.F_ADD, V(1), V(0)), V(2), B(R.F_MUL, V(2), C(1.0))]))
    for op in (cross, mut):
        assert op.library.pop_size == 2 and op.library.batch_subtree_size[:, 0].tolist() == [3, 1] and op.semantics.shape == (2, 24)
    cross.update_library(_forest([V(1)]))
    assert mut.library.pop_size == 1 and int(mut.library.batch_node_value[0, 0]) == 1 and shared.semantics.shape == (1, 24)
    # the mutation now draws its donors from the one member: x0 + x2 at its x2 leaf becomes x0 + x1
    f = _forest([B(R.F_ADD, V(0), V(2))])
    SemanticBackpropMutation(1.0, X, y, library=shared, allow_constant=False).apply(f, torch.tensor([0]), _i32(2))
    assert _same(f, _forest([B(R.F_ADD, V(0), V(1))]))
    # a Forest as the library still gives every operator a library of its own
    own = ApproxGeometricCrossover(X, library=_forest([V(0), V(1)]))
    assert own.semantic_library is not shared and own.library.pop_size == 2


def test_backprop_mutation_on_the_shared_helper_gives_the_parent_commits_forests():
    """the run recorded on the parent commit (tests/golden/agx_parent_backprop_mutation.npz): the built library, its semantics and the
    forest after two calls, bit for bit"""
    rng = np.random.default_rng(11)
    X = torch.from_numpy(rng.choice(np.setdiff1d(np.arange(-8, 9), [0]), (24, 3)).astype(np.float32) / 4)
    y = (X[:, :1] * X[:, 1:2] + X[:, 2:3]).contiguous()
    d = _descriptor()
    torch.manual_seed(20261021)
    with np.errstate(all="ignore"):
        op = SemanticBackpropMutation(0.6, X, y, descriptor=d, library_size=30, fallback=DefaultMutation(0.5, d))
        f = Forest.random_generate(40, d, keys=torch.tensor([5, 6]))
        out = op(f, skip_rows=3)
        out = op(out)
    want = np.load(GOLDEN)
    lib = op.library
    got = dict(lib_value=_bits(lib.batch_node_value), lib_type=lib.batch_node_type.numpy(), lib_size=lib.batch_subtree_size.numpy(),
               semantics=_bits(op.semantics), value=_bits(out.batch_node_value), type=out.batch_node_type.numpy(), size=out.batch_subtree_size.numpy())
    assert sorted(got) == sorted(want.files)
    for k in got:
        assert np.array_equal(got[k], want[k]), k


# ---- planted geometric cases ----------------------------------------------------------------------------------------------------------
HALF = B(R.F_MUL, B(R.F_ADD, V(1), V(2)), C(0.5))        # (x1 + x2) * 0.5
INVHALF = U(R.F_INV, HALF)
PLANTED = {   # name -> (recipient, mate, the position of the recipient's x1 leaf, the donor the library holds, the child)
    "ADD": (B(R.F_ADD, V(0), V(1)), B(R.F_ADD, V(0), V(2)), 2, HALF, B(R.F_ADD, V(0), HALF)),
    "SUB": (B(R.F_SUB, V(0), V(1)), B(R.F_SUB, V(0), V(2)), 2, HALF, B(R.F_SUB, V(0), HALF)),
    "MUL": (B(R.F_MUL, C(4.0), V(1)), B(R.F_MUL, C(4.0), V(2)), 2, HALF, B(R.F_MUL, C(4.0), HALF)),
    "DIV": (B(R.F_DIV, V(1), C(4.0)), B(R.F_DIV, V(2), C(4.0)), 1, HALF, B(R.F_DIV, HALF, C(4.0))),
    "NEG": (U(R.F_NEG, V(1)), U(R.F_NEG, V(2)), 1, HALF, U(R.F_NEG, HALF)),
}


@pytest.mark.parametrize("name", sorted(PLANTED))
def test_a_planted_geometric_case(name):
    recipient, mate, pos, donor, child = PLANTED[name]
    X = _data().abs()   # positive integers: no sum is zero, so no result is a zero whose sign two orders of evaluation could disagree on
    lib = _forest([V(0), donor, V(2), C(0.5)])
    op = ApproxGeometricCrossover(X, library=lib)
    parents = _forest([recipient, mate])
    a, b = parents.batch_forward(X)[:, :, 0]
    mid = 0.5 * a + 0.5 * b
    best, dist, *_ = parents[:1].SR_midpoint_match(X, _i32(pos), parents, op.semantics, mate_index=_i32(1))
    assert int(best[0]) == 1 and float(dist[0, 1]) == 0.0, name
    new, found = op.apply(parents, _i32(0), _i32(1), _i32(pos))
    assert found.tolist() == [True] and _same(new, _forest([child])), name
    assert np.array_equal(_bits(new.batch_forward(X)[0, :, 0]), _bits(mid)), name   # the midpoint, bit for bit


def test_the_constant_donor():
    X = _data()
    lib = _forest([V(0), V(1), V(2)])
    parents = _forest([B(R.F_ADD, V(0), C(1.0)), B(R.F_ADD, V(0), C(4.0))])   # the midpoint is x0 + 2.5
    new, found = ApproxGeometricCrossover(X, library=lib).apply(parents, _i32(0), _i32(1), _i32(2))
    assert found.tolist() == [True] and _same(new, _forest([B(R.F_ADD, V(0), C(2.5))]))
    new, _ = ApproxGeometricCrossover(X, library=lib, allow_constant=False).apply(parents, _i32(0), _i32(1), _i32(2))
    assert int(new.batch_node_type[0, 2]) == R.T_VAR and int(new.batch_subtree_size[0, 0]) == 3   # the nearest variable instead


class _Fixed(ApproxGeometricCrossover):
    """the draws of a call, fixed: offspring n is parents[left[n]] at left_pos[n] with the mate parents[right[n]]"""
    fixed = ([0, 1, 0], [1, 0, 1], [1, 2, 0])

    def draw(self, tree_sizes, n_parents, target_cnt, device):
        assert target_cnt == len(self.fixed[0]) and n_parents == 2
        return (*(_i32(*v) for v in self.fixed), _i32(0, 0, 0))


def test_an_unmatched_offspring_with_and_without_a_fallback():
    X = _data()
    lib = _forest([V(0), V(2)])
    blocked, open_ = U(R.F_SIN, V(0)), B(R.F_ADD, V(0), V(1))
    forest = _forest([V(2), blocked, open_])
    survivors = torch.tensor([1, 2])
    out = _Fixed(X, library=lib)(forest, survivors, 3, torch.zeros(3))
    assert out.pop_size == 3 and _same(out[0:1], _forest([blocked]))          # a copy of its recipient, bit for bit
    assert not _same(out[1:2], _forest([open_])) and int(out.batch_subtree_size[1, 0]) == 3

    class Marker(BaseCrossover):   # writes trees no library holds
        calls = 0

        def __call__(self, forest_, survivor_indices, target_cnt, fitness):
            Marker.calls += 1
            assert forest_ is forest and survivor_indices is survivors and target_cnt == 3
            return _forest([B(R.F_MUL, C(7.0), V(2))] * target_cnt)

    got = _Fixed(X, library=lib, fallback=Marker())(forest, survivors, 3, torch.zeros(3))
    assert Marker.calls == 1 and _same(got[0:1], _forest([B(R.F_MUL, C(7.0), V(2))])) and _same(got[1:], out[1:])


def test_a_pair_of_one_tree_with_itself():
    """the midpoint is the tree's own predictions: the subtree is replaced by the library member nearest to what it already computes"""
    X = _data()
    lib = _forest([V(0), B(R.F_ADD, V(1), V(2)), V(2)])
    tree = B(R.F_MUL, V(0), B(R.F_ADD, V(2), V(1)))
    parents = _forest([tree, V(1)])
    new, found = ApproxGeometricCrossover(X, library=lib, allow_constant=False).apply(parents, _i32(0), _i32(0), _i32(2))
    assert found.tolist() == [True] and _same(new, _forest([B(R.F_MUL, V(0), B(R.F_ADD, V(1), V(2)))]))
    assert torch.equal(new.batch_forward(X)[0, :, 0], parents.batch_forward(X)[0, :, 0])


def test_three_generations_of_genetic_programming():
    X = _data()
    y = (X[:, :1] * X[:, 1:2] + X[:, 2:3]).contiguous()
    d = _descriptor()
    torch.manual_seed(2)
    with np.errstate(all="ignore"):
        op = ApproxGeometricCrossover(X, descriptor=d, library_size=30, fallback=DefaultCrossover())
        algo = GeneticProgramming(Forest.random_generate(40, d, keys=torch.tensor([5, 6])), op, DefaultMutation(0.2, d), DefaultSelection(0.3, 4))
        n0 = cpu_agx_ops.calls["match"]
        forest = algo.forest
        for _ in range(3):
            forest = algo.step(-forest.SR_fitness(X, y))
    assert forest.pop_size == 40 and cpu_agx_ops.calls["match"] == n0 + 3
    t, s = forest.batch_node_type.numpy(), forest.batch_subtree_size.numpy()
    from subtree_ref import check_prefix_tree
    assert all(check_prefix_tree(t[i], s[i]) for i in range(40))
