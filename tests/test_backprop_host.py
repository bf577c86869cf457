"""CPU: semantic backpropagation above the kernel -- the argument checks of Forest.SR_desired_semantics / SR_backprop_match, the library
of SemanticBackpropMutation and the operator itself (planted defects, the constant donor, the fallback, skip_rows, a generation of
GeneticProgramming), with the numpy restatement registered as a test-only CPU kernel (tests/cpu_backprop_ops.py), and the forest
invariants (dead words, row order, slices) of the two ops on it.  Importing this module also puts the two ops into the invariance and
binding tables (tests/backprop_tables.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import backprop_ref as BR  # noqa: E402
import backprop_tables as BT  # noqa: E402
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

from evogp_amd.algorithm import (DefaultCrossover, DefaultMutation, DefaultSelection, GeneticProgramming,  # noqa: E402
                                 SemanticBackpropMutation)
from evogp_amd.tree import Forest, GenerateDescriptor, set_default_device  # noqa: E402
from evogp_amd.tree import utils as _tree_utils  # noqa: E402

L = 16


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
    """quarters in [-2, 2] without zeros: sums, differences and the products of two of them are exact in float32"""
    rng = np.random.default_rng(11)
    X = rng.choice(np.setdiff1d(np.arange(-8, 9), [0]), (n, 3)).astype(np.float32) / 4
    return torch.from_numpy(X)


def _descriptor(**kw):
    args = dict(max_tree_len=L, input_len=3, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=3, const_samples=[-1, 0, 1])
    args.update(kw)
    return GenerateDescriptor(**args)


def _same(a: Forest, b: Forest):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a._tensors(), b._tensors()))


def _copy(f: Forest):
    return Forest(f.input_len, f.output_len, *(a.clone() for a in f._tensors()))


# ---- the invariants of the two ops on the CPU stand-ins ------------------------------------------------------------------------------
@pytest.mark.parametrize("op,case", [(op, c) for op in (BT.DESIRED, BT.MATCH) for c in FI.cases_for(op)])
def test_cpu_stand_in_keeps_the_invariants(op, case):
    FI.check(op, FI.TABLE[op], FI.build_case(case, min(40, FI.CASES[case]["pop"]), 50), "cpu")


def test_the_ops_are_in_both_tables():
    assert FI.cases_for(BT.DESIRED) == FI.cases_for(BT.MATCH) == ["arith_L64", "all_L64_v13", "all_L1024_v40"]
    assert BT.DESIRED in BT.BC.TABLE and BT.MATCH in BT.BC.TABLE


# ---- the two Forest methods -------------------------------------------------------------------------------------------------------------
def test_forest_methods_and_their_argument_checks():
    X = _data()
    f = _forest([B(R.F_ADD, B(R.F_MUL, V(0), V(1)), V(0)), U(R.F_SIN, V(0)), V(1)])
    y = (X[:, :1] * X[:, 1:2] + X[:, 2:3]).contiguous()
    pos = torch.tensor([4, 1, 0], dtype=torch.int32)
    desired, state, status = f.SR_desired_semantics(X, y, pos)
    assert desired.shape == (3, 24) and desired.dtype == torch.float32 and state.dtype == torch.uint8 and status.tolist() == [0, 3, 0]
    assert torch.equal(desired[0], X[:, 2]) and torch.equal(desired[2], y[:, 0]) and desired[1].isnan().all() and (state[1] == 2).all()
    best, dist, const, const_dist, counts, status2 = f.SR_backprop_match(X, y, pos, X.t().contiguous())
    assert best.tolist() == [2, -1, best[2]] and dist.shape == (3, 3) and dist.dtype == torch.float64 and float(dist[0, 2]) == 0.0
    assert counts.tolist() == [[24, 0, 0], [0, 0, 24], [24, 0, 0]] and torch.equal(status, status2) and const_dist.dtype == torch.float64
    # a library forest: its semantics are batch_forward's
    lib = _forest([V(0), V(1), V(2)])
    again = f.SR_backprop_match(X, y, pos.to(torch.int64), lib)
    assert all(torch.equal(a, b) or (a.isnan() == b.isnan()).all() for a, b in zip(again, (best, dist, const, const_dist, counts, status2)))
    n0 = dict(cpu_backprop_ops.calls)
    multi = Forest(3, 2, *f._tensors())
    for call in (lambda: multi.SR_desired_semantics(X, torch.cat([y, y], 1), pos), lambda: multi.SR_backprop_match(X, torch.cat([y, y], 1), pos, lib)):
        with pytest.raises(ValueError, match="single-output"):
            call()
    for bad in (pos[:2], pos[None], pos.to(torch.float32)):
        with pytest.raises(ValueError, match="positions"):
            f.SR_desired_semantics(X, y, bad)
        with pytest.raises(ValueError, match="positions"):
            f.SR_backprop_match(X, y, bad, lib)
    with pytest.raises(AssertionError, match="inputs shape"):
        f.SR_desired_semantics(X[:, :2], y, pos)
    with pytest.raises(AssertionError, match="outputs shape"):
        f.SR_desired_semantics(X, y[:5], pos)
    for bad in (X.t()[:, :5].contiguous(), X[:, 0], torch.zeros((0, 24)), torch.zeros((1025, 24))):
        with pytest.raises(ValueError, match="library"):
            f.SR_backprop_match(X, y, pos, bad)
    with pytest.raises(ValueError, match="library forest"):
        f.SR_backprop_match(X, y, pos, _forest([V(0)], inputs=2))
    assert cpu_backprop_ops.calls == n0   # every check comes before the first launch


# ---- the library ------------------------------------------------------------------------------------------------------------------------
def test_a_built_library_holds_every_variable_and_no_model_twice():
    X = _data()
    y = X[:, :1].contiguous()
    torch.manual_seed(3)
    with np.errstate(all="ignore"):
        op = SemanticBackpropMutation(0.5, X, y, descriptor=_descriptor(), library_size=200)
        lib = op.library
        _, rep = lib.semantic_classes(X)
    assert rep.all() and lib.pop_size <= 1024 and op.semantics.shape == (lib.pop_size, 24) and 3 < lib.pop_size < 203
    one = lib.batch_subtree_size[:, 0] == 1
    leaves = set(zip(lib.batch_node_type[one, 0].tolist(), lib.batch_node_value[one, 0].tolist()))
    assert {(R.T_VAR, 0.0), (R.T_VAR, 1.0), (R.T_VAR, 2.0)} <= leaves
    with np.errstate(all="ignore"):
        assert torch.equal(op.semantics.isnan(), lib.batch_forward(X)[:, :, 0].isnan())
        big = SemanticBackpropMutation(0.5, X, y, descriptor=_descriptor(using_funcs=["+", "-", "*", "/", "sin", "exp"], max_layer_cnt=4,
                                                                         const_samples=list(np.linspace(-2, 2, 41))), library_size=1500)
    assert big.library.pop_size == 1024   # truncated
    only = SemanticBackpropMutation(0.5, X, y, descriptor=_descriptor(), library_size=0)
    assert only.library.pop_size == 3
    for kw, msg in ((dict(), "library or a descriptor"), (dict(descriptor=_descriptor(input_len=2)), "descriptor should"),
                    (dict(library=_forest([V(0)], inputs=2)), "library should"), (dict(descriptor=_descriptor(), fallback=object()), "fallback"),
                    (dict(descriptor=_descriptor(), library_size=-1), "library_size")):
        with pytest.raises(ValueError, match=msg):
            SemanticBackpropMutation(0.5, X, y, **kw)
    with pytest.raises(ValueError, match="datapoints"):
        SemanticBackpropMutation(0.5, X, y[:5], descriptor=_descriptor())
    # update_library: the semantically distinct members of a forest, the smallest of each class
    op.update_library(_forest([B(R.F_ADD, V(0), V(1)), B(R.F_ADD, V(1), V(0)), V(2), B(R.F_MUL, V(2), C(1.0))]))
    assert op.library.pop_size == 2 and op.library.batch_subtree_size[:, 0].tolist() == [3, 1] and op.semantics.shape == (2, 24)
    wide = SemanticBackpropMutation(1.0, X, y, library=_forest([V(0)], width=32))
    with pytest.raises(ValueError, match="max_tree_len"):
        wide(_forest([V(1)]))


# ---- planted defects --------------------------------------------------------------------------------------------------------------------
M01 = B(R.F_MUL, V(0), V(1))
S01 = B(R.F_ADD, V(0), V(1))
PLANTED = {   # name -> (the truth, the tree with x0 where the truth has x2, the position of that leaf)
    "ADD": (B(R.F_ADD, M01, V(2)), B(R.F_ADD, M01, V(0)), 4),
    "SUB": (B(R.F_SUB, V(2), M01), B(R.F_SUB, V(0), M01), 1),
    "MUL": (B(R.F_MUL, S01, V(2)), B(R.F_MUL, S01, V(0)), 4),
    "DIV": (B(R.F_DIV, V(2), V(1)), B(R.F_DIV, V(0), V(1)), 1),
    "NEG": (U(R.F_NEG, B(R.F_SUB, V(1), V(2))), U(R.F_NEG, B(R.F_SUB, V(1), V(0))), 3),
}


@pytest.mark.parametrize("name", sorted(PLANTED))
def test_a_planted_defect_is_repaired_in_one_call(name):
    truth, wrong, pos = PLANTED[name]
    X = _data()
    y = _forest([truth]).batch_forward(X)[:, :, 0].t().contiguous()   # (D, 1): the bits the repaired tree must produce
    lib = _forest([V(1), B(R.F_ADD, V(0), V(1)), V(2), C(0.5)])
    op = SemanticBackpropMutation(1.0, X, y, library=lib)
    f = _forest([wrong, wrong])
    assert float(((f.batch_forward(X)[0, :, 0] - y[:, 0]) ** 2).sum()) > 0
    out = op.apply(f, torch.tensor([1]), torch.tensor([pos], dtype=torch.int32))
    assert out is f and _same(f[0:1], _forest([wrong])) and _same(f[1:2], _forest([truth])), name
    assert torch.equal(f.batch_forward(X)[1, :, 0], y[:, 0])   # loss exactly 0


def test_the_constant_donor():
    X = _data()
    y = (X[:, :1] + 2.5).contiguous()
    lib = _forest([V(0), V(1), V(2)])
    tree = B(R.F_ADD, V(0), V(1))
    f = _forest([tree])
    SemanticBackpropMutation(1.0, X, y, library=lib).apply(f, torch.tensor([0]), torch.tensor([2], dtype=torch.int32))
    assert _same(f, _forest([B(R.F_ADD, V(0), C(2.5))]))
    g = _forest([tree])
    SemanticBackpropMutation(1.0, X, y, library=lib, allow_constant=False).apply(g, torch.tensor([0]), torch.tensor([2], dtype=torch.int32))
    assert int(g.batch_node_type[0, 2]) == R.T_VAR and int(g.batch_subtree_size[0, 0]) == 3   # the nearest variable instead


def test_a_blocked_tree_goes_to_the_fallback_or_stays():
    X = _data()
    y = X[:, 2:3].contiguous()
    lib = _forest([V(0), V(1), V(2)])
    blocked, open_ = U(R.F_SIN, V(0)), B(R.F_ADD, V(0), V(1))
    rows_, pos = torch.tensor([0, 1]), torch.tensor([1, 1], dtype=torch.int32)
    f = _forest([blocked, open_])
    SemanticBackpropMutation(1.0, X, y, library=lib).apply(f, rows_, pos)
    assert _same(f[0:1], _forest([blocked])) and not _same(f[1:2], _forest([open_]))   # bit for bit; the other tree was repaired

    class Marker(DefaultMutation):   # writes a tree no library holds
        def __call__(self, forest, skip_rows=0):
            assert self.mutation_rate == 1.0
            n = forest.pop_size
            return _forest([B(R.F_MUL, C(7.0), V(2))] * n)

    fb = Marker(0.25, _descriptor())
    g = _forest([blocked, open_])
    SemanticBackpropMutation(1.0, X, y, library=lib, fallback=fb).apply(g, rows_, pos)
    assert _same(g[0:1], _forest([B(R.F_MUL, C(7.0), V(2))])) and _same(g[1:2], f[1:2]) and fb.mutation_rate == 0.25
    # a real fallback: the blocked tree is mutated by it, whatever it draws
    torch.manual_seed(1)
    h = _forest([blocked] * 8)
    SemanticBackpropMutation(1.0, X, y, library=lib, fallback=DefaultMutation(0.1, _descriptor()))(h)
    assert not _same(h, _forest([blocked] * 8))


def test_skip_rows_rate_zero_and_a_generation():
    X = _data()
    y = (X[:, :1] * X[:, 1:2] + X[:, 2:3]).contiguous()
    d = _descriptor()
    torch.manual_seed(2)
    with np.errstate(all="ignore"):
        op = SemanticBackpropMutation(1.0, X, y, descriptor=d, library_size=30, fallback=DefaultMutation(0.5, d))
        start = Forest.random_generate(40, d, keys=torch.tensor([5, 6]))
        f = _copy(start)
        n0 = cpu_backprop_ops.calls["match"]
        out = op(f, skip_rows=7)
        assert cpu_backprop_ops.calls["match"] == n0 + 1
        assert _same(out[:7], start[:7]) and not _same(out[7:], start[7:])
        op.mutation_rate = 0.0
        g = _copy(start)
        assert op(g) is g and _same(g, start) and cpu_backprop_ops.calls["match"] == n0 + 1
        # inside GeneticProgramming.step
        op.mutation_rate = 0.3
        algo = GeneticProgramming(_copy(start), DefaultCrossover(), op, DefaultSelection(0.3, 4))
        nxt = algo.step(-start.SR_fitness(X, y))
    assert nxt.pop_size == 40 and cpu_backprop_ops.calls["match"] == n0 + 2
    t, s = nxt.batch_node_type.numpy(), nxt.batch_subtree_size.numpy()
    from subtree_ref import check_prefix_tree
    assert all(check_prefix_tree(t[i], s[i]) for i in range(40))
    assert BR.OK == 0
