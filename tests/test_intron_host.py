"""CPU: exact semantic intron removal above the kernels -- Forest.SR_subtree_introns / remove_introns / simplify(introns=True),
SymbolicRegression(intron_removal_every=), StandardPipeline's hook and the ``sig=`` keyword of the subtree library -- with the numpy
restatement registered as test-only CPU kernels (tests/cpu_intron_ops.py), the forest invariants (dead words, row order, slices) of both
ops on it, and the argument checks of the two C entry points, which return before any launch.  Importing this module also puts the two
ops into the invariance and binding tables (tests/intron_tables.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cpu_dedup_ops  # noqa: E402
import cpu_grad_ops  # noqa: E402
import cpu_intron_ops  # noqa: E402
import cpu_ops  # noqa: E402
import cpu_scale_ops  # noqa: E402
import cpu_semantic_ops  # noqa: E402
import cpu_structure_ops  # noqa: E402
import cpu_sublib_ops  # noqa: E402
import cpu_subtree_ops  # noqa: E402
import cpu_wloss_ops  # noqa: E402
import forest_invariance as FI  # noqa: E402
import intron_ref as IR  # noqa: E402
import intron_tables as IT  # noqa: E402
import sr_grad_ref as R  # noqa: E402
import subtree_ref  # noqa: E402
from intron_ref import c, iff, op, un, x  # noqa: E402

for m in (cpu_ops, cpu_grad_ops, cpu_dedup_ops, cpu_scale_ops, cpu_semantic_ops, cpu_structure_ops, cpu_subtree_ops, cpu_wloss_ops,
          cpu_sublib_ops, cpu_intron_ops):
    m.register()

from evogp_amd import _lib  # noqa: E402
from evogp_amd.algorithm import SemanticLibrary  # noqa: E402
from evogp_amd.problem import SymbolicRegression  # noqa: E402
from evogp_amd.tree import Forest, GenerateDescriptor, set_default_device  # noqa: E402
from evogp_amd.tree import utils as _tree_utils  # noqa: E402

L = 32
D = 40


@pytest.fixture(autouse=True)
def _cpu_default_device():
    saved = _tree_utils._DEVICE
    set_default_device("cpu")
    yield
    _tree_utils._DEVICE = saved


def _bits(t):
    a = t.contiguous().numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a: Forest, b: Forest):
    return a.pop_size == b.pop_size and all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(a._tensors(), b._tensors()))


def _E(a, b):
    return bool(IR.equal(a.numpy(), b.numpy()).all())


def _data(seed=3, var_len=3):
    rng = np.random.default_rng(seed)
    X = rng.normal(0.0, 1.0, (D, var_len)).astype(np.float32)
    X[:, 0] = rng.uniform(0.5, 1.5, D)                 # x0 > 0 and x1 > x0 on every row (the hierarchy plant), x2 of both signs
    X[:, 1] = X[:, 0] + rng.uniform(0.25, 1.0, D).astype(np.float32)
    y = (2.0 * X[:, :1] * X[:, 1:2] - 0.5).astype(np.float32)
    return torch.from_numpy(X), torch.from_numpy(y)


def _forest(seed=5, pop=40, kind="all"):
    rng = np.random.default_rng(seed)
    funcs, wraps = (IR.ARITH, IR.ARITH_WRAPS) if kind == "arith" else (IR.ALL_FUNCS, tuple(IR.WRAPS))
    trees = []
    while len(trees) < pop:
        nodes = IR.random_nodes(rng, funcs, 3, 3, 0.15 if len(trees) % 2 else 0.0, wraps)
        if len(nodes) <= L:
            trees.append(nodes)
    trees[0] = op(R.F_MIN, iff(x(0), x(1), x(2)), x(0))
    trees[1] = op(R.F_ADD, un(R.F_NEG, un(R.F_NEG, x(1))), c(0.0))
    f = IR.forest(trees, L)
    f[2][2, 0] = 0   # malformed
    for a in f:      # structural duplicates, for dedup=True
        a[7], a[9] = a[1], a[1]
    return Forest(3, 1, *(torch.from_numpy(a) for a in f), func_mask=(1 << 29) - 1)


# ---- the invariants of both ops on the CPU stand-ins, the tables --------------------------------------------------------------------------
@pytest.mark.parametrize("op_name", [IT.INTRONS, IT.REWRITE])
@pytest.mark.parametrize("case", FI.cases_for(IT.INTRONS))
def test_cpu_stand_ins_keep_the_invariants(case, op_name):
    FI.check(op_name, FI.TABLE[op_name], FI.build_case(case, min(40, FI.CASES[case]["pop"]), 50), "cpu")


def test_the_ops_are_in_both_tables():
    for name in (IT.INTRONS, IT.REWRITE):
        assert FI.cases_for(name) == ["arith_L64", "all_L64_v13", "all_L1024_v40"] and name in IT.BC.TABLE
    row = FI.TABLE[IT.REWRITE]
    assert row["cls"] == "rewriter" and row["tails"] == FI.ZERO3 and row["copied"] is FI._malformed_rows and "evogp_hip_remove_introns" in row["cite"]
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "evogp_hip.h")).read()
    assert "[new_len, gp_len) is zero in all three arrays" in header and "A malformed row is copied as it is" in header, "the cited lines"


# ---- the Forest methods ---------------------------------------------------------------------------------------------------------------------
def test_rep_and_removal_on_a_forest():
    X, _ = _data()
    f = _forest()
    keep = [a.clone() for a in f._tensors()]
    with np.errstate(all="ignore"):
        rep = f.SR_subtree_introns(X)
        g, removed = f.remove_introns(X)
        P0, P1 = f.batch_forward(X)[:, :, 0], g.batch_forward(X)[:, :, 0]
    assert rep.shape == (40, L) and rep.dtype == torch.int16 and removed.shape == (40,) and removed.dtype == torch.int32
    assert all(torch.equal(a, b) for a, b in zip(keep, f._tensors())), "the input forest is untouched"
    assert g is not f and g.func_mask == f.func_mask != 0 and g.input_len == 3 and g.output_len == 1
    assert rep[0, 0] == 2 and rep[0, 1] == 3 and int(removed[0]) == 5 and int(g.batch_subtree_size[0, 0]) == 1, "the hierarchy plant: x0"
    assert int(removed[1]) == 4 and list(g.batch_node_type[1, :2]) == [R.T_VAR, 0] and float(g.batch_node_value[1, 0]) == 1.0
    assert int(removed[2]) == 0 and all(torch.equal(a[2], b[2]) for a, b in zip(g._tensors(), f._tensors())), "a malformed row is copied"
    ok = np.arange(40) != 2
    assert _E(P0[ok], P1[ok]), "the predictions keep their bits on every row"
    t1, s1 = g.batch_node_type.numpy(), g.batch_subtree_size.numpy()
    assert all(subtree_ref.check_prefix_tree(t1[t], s1[t]) for t in range(40) if t != 2)
    assert torch.equal(g.batch_subtree_size[:, 0][ok].int(), (f.batch_subtree_size[:, 0].int() - removed)[ok])
    assert 10 <= int((removed > 0).sum()) <= 30, "a test forest with and without introns"
    with np.errstate(all="ignore"):
        g2, removed2 = g.remove_introns(X)
    assert _same(g, g2) and not removed2.any(), "a fixed point (this forest drops no refused candidate)"


def test_sig_is_reused_and_garbage_sig_is_safe():
    X, _ = _data()
    f = _forest()
    with np.errstate(all="ignore"):
        sig = f.SR_subtree_signatures(X)
        n0 = dict(cpu_sublib_ops.calls)
        rep = f.SR_subtree_introns(X, sig=sig)
        g, removed = f.remove_introns(X, sig=sig)
        assert cpu_sublib_ops.calls == n0, "a caller's signatures spare the pass"
        plain = f.remove_introns(X)
        assert cpu_sublib_ops.calls["subtree_signatures"] == n0["subtree_signatures"] + 1
        assert _same(g, plain[0]) and torch.equal(removed, plain[1]) and torch.equal(rep, f.SR_subtree_introns(X))
        lib = SemanticLibrary(X, library=_forest(pop=10))
        n1 = dict(cpu_sublib_ops.calls)
        lib.update_library(f, source="subtrees", max_size=5, sig=sig)
        assert cpu_sublib_ops.calls["subtree_signatures"] == n1["subtree_signatures"] and cpu_sublib_ops.calls["library_select"] == n1["library_select"] + 1
        with_sig = lib.library
        lib.update_library(f, source="subtrees", max_size=5)
        assert cpu_sublib_ops.calls["subtree_signatures"] == n1["subtree_signatures"] + 1 and _same(with_sig, lib.library)
        h, lost = f.remove_introns(X, sig=sig % 3 + 1)
        ok = np.arange(40) != 2
        assert _E(f.batch_forward(X)[:, :, 0][ok], h.batch_forward(X)[:, :, 0][ok]) and 0 < int(lost.sum()) <= int(removed.sum())
    for bad in (sig[:, :-1], sig.to(torch.int32), sig.numpy()):
        with pytest.raises(ValueError, match="sig should be"):
            f.SR_subtree_introns(X, sig=bad)
        with pytest.raises(ValueError, match="sig should be"):
            f.subtree_library(X, sig=bad)
    with pytest.raises(ValueError, match="source='subtrees'"):
        lib.update_library(f, sig=sig)


def test_dedup_gives_the_same_bits():
    X, _ = _data()
    f = _forest()
    with np.errstate(all="ignore"):
        plain = f.remove_introns(X)
        n0 = cpu_intron_ops.calls["subtree_introns"]
        once = f.remove_introns(X, dedup=True)
    assert cpu_intron_ops.calls["subtree_introns"] == n0 + 1
    assert _same(plain[0], once[0]) and torch.equal(plain[1], once[1])
    assert int(once[1][7]) == int(once[1][9]) == int(once[1][1]) == 4, "the duplicates take their class's rep"


def test_simplify_with_introns_and_its_idempotence():
    X, y = _data()
    f = _forest()
    with np.errstate(all="ignore"):
        n0 = dict(cpu_intron_ops.calls)
        base, base_loss = f.simplify(X, y)
        assert cpu_intron_ops.calls == n0, "simplify() without the keyword never calls the new ops"
        g, loss = f.simplify(X, y, introns=True)
        assert cpu_intron_ops.calls["subtree_introns"] == n0["subtree_introns"] + 1 and cpu_intron_ops.calls["remove_introns"] == n0["remove_introns"] + 1
        assert np.array_equal(_bits(loss), _bits(base_loss)), "the loss is the one of hoist and fold: the predictions keep their bits"
        want = base.remove_introns(X)[0]
        assert _same(g, want) and (g.batch_subtree_size[:, 0] <= base.batch_subtree_size[:, 0]).all()
        ok = np.arange(40) != 2
        assert _E(base.batch_forward(X)[:, :, 0][ok], g.batch_forward(X)[:, :, 0][ok])
        again, loss2 = g.simplify(X, y, introns=True)
        assert _same(g, again) and np.array_equal(_bits(loss2), _bits(loss)), "simplifying the result again returns it (this forest drops no refused candidate)"
        d, dl = f.simplify(X, y, introns=True, dedup=True)
        assert _same(d, g) and np.array_equal(_bits(dl), _bits(loss))
        # hoist and fold off: the introns alone
        only = f.simplify(X, y, hoist=False, fold_constants=False, introns=True)[0]
        assert _same(only, f.remove_introns(X)[0])


def test_defaults_never_call_the_new_ops():
    X, y = _data()
    f = _forest()
    with np.errstate(all="ignore"):
        n0 = dict(cpu_intron_ops.calls)
        lib = SemanticLibrary(X, library=_forest(pop=10))
        lib.update_library(f)
        lib.update_library(f, source="subtrees", max_size=4)
        f.subtree_library(X)
        p = SymbolicRegression(datapoints=X, labels=y, simplify_every=1)
        out = p.optimize(f)
        assert _same(out, f.simplify(X, y)[0])
        assert SymbolicRegression(datapoints=X, labels=y).optimize(f) is f
    assert cpu_intron_ops.calls == n0 and p.intron_removal_every == 0


# ---- the problem and the pipeline -----------------------------------------------------------------------------------------------------------
def test_problem_removes_introns_on_every_kth_optimize():
    X, y = _data()
    f = _forest()
    rng = np.random.default_rng(1)
    mask = torch.from_numpy(rng.random(D) < 0.3)
    mask[0], mask[1] = True, False
    w = torch.from_numpy(rng.uniform(0.5, 2.0, D).astype(np.float32))
    with np.errstate(all="ignore"):
        p = SymbolicRegression(datapoints=X, labels=y, loss="pinball", loss_param=0.3, sample_weights=w, validation_mask=mask, intron_removal_every=2)
        first = p.optimize(f)
        assert first is f, "call 1 of every second"
        second = p.optimize(f)
        want = f.remove_introns(X)[0]
        assert _same(second, want)
        plain = SymbolicRegression(datapoints=X, labels=y, loss="pinball", loss_param=0.3, sample_weights=w, validation_mask=mask)
        a, b = p.evaluate(second), plain.evaluate(f)
        assert np.array_equal(_bits(a), _bits(b)), "training loss unchanged, bit for bit"
        assert np.array_equal(_bits(p.last_validation_loss), _bits(plain.last_validation_loss)), "and so is the held-out loss"
        # together with simplification, scaling and dedup
        q = SymbolicRegression(datapoints=X, labels=y, simplify_every=1, intron_removal_every=1, dedup=True)
        assert _same(q.optimize(f), f.remove_introns(X)[0].simplify(X, y)[0])
        s = SymbolicRegression(datapoints=X, labels=y, linear_scaling=True, intron_removal_every=1)
        assert np.array_equal(_bits(s.evaluate(s.optimize(f))), _bits(SymbolicRegression(datapoints=X, labels=y, linear_scaling=True).evaluate(f)))


def test_problem_argument_errors():
    X, y = _data()
    for bad in (-1, 1.5, True, "2"):
        with pytest.raises(ValueError, match="intron_removal_every"):
            SymbolicRegression(datapoints=X, labels=y, intron_removal_every=bad)
    with pytest.raises(ValueError, match="intron_removal_every works on single-output"):
        SymbolicRegression(datapoints=X, labels=torch.cat([y, y], 1), intron_removal_every=1)
    with pytest.raises(ValueError, match="multigene cannot be combined with intron_removal_every"):
        SymbolicRegression(datapoints=X, labels=y, multigene=True, intron_removal_every=1)
    SymbolicRegression(datapoints=X, labels=torch.cat([y, y], 1))   # the default keeps taking multi-output problems
    multi = Forest(3, 2, *_forest()._tensors())
    for call in (lambda: multi.SR_subtree_introns(X), lambda: multi.remove_introns(X)):
        with pytest.raises(ValueError, match="single-output"):
            call()
    with pytest.raises(ValueError, match="inputs shape"):
        _forest().remove_introns(X[:, :2])


def test_pipeline_calls_optimize_for_intron_removal_alone():
    from evogp_amd.algorithm import DefaultCrossover, DefaultMutation, DefaultSelection, GeneticProgramming
    from evogp_amd.pipeline import StandardPipeline

    X, y = _data()
    d = GenerateDescriptor(max_tree_len=L, input_len=3, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=4, const_samples=[-1, 0, 1])

    def pipeline(**kw):
        algo = GeneticProgramming(Forest.random_generate(60, d, keys=torch.tensor([1, 2])), DefaultCrossover(), DefaultMutation(0.2, d),
                                  DefaultSelection(0.3, 2))
        return algo, StandardPipeline(algo, SymbolicRegression(datapoints=X, labels=y, **kw), is_show_details=False, generation_limit=2)

    with np.errstate(all="ignore"):
        algo, pipe = pipeline(intron_removal_every=1)
        start = algo.forest
        n0 = cpu_intron_ops.calls["remove_introns"]
        host = pipe.step()
        assert cpu_intron_ops.calls["remove_introns"] == n0 + 1
        want, removed = start.remove_introns(X)
        assert int(removed.sum()) > 0, "fresh trees over -1, 0, 1 hold introns"
        algo0, pipe0 = pipeline()
        n1 = dict(cpu_intron_ops.calls)
        host0 = pipe0.step()
        assert cpu_intron_ops.calls == n1, "the default pipeline never calls the new ops"
        assert np.array_equal(_bits(host), _bits(host0)), "the fitness of the rewritten forest is the fitness of the forest"
        assert torch.equal(pipe.best_tree.node_value, want[int(torch.argmax(host))].node_value), "the rewritten trees are what is scored and bred"
        pipe.step()
        assert cpu_intron_ops.calls["remove_introns"] == n0 + 3


# ---- the C entry points -------------------------------------------------------------------------------------------------------------------
def test_c_entry_points_check_their_arguments():
    Lb = _lib.lib
    p, q, r, s = (ctypes.c_void_p(16 * k) for k in (1, 2, 3, 4))   # never dereferenced: every call below returns from its argument checks
    S, Q = Lb.evogp_hip_sr_subtree_introns, Lb.evogp_hip_remove_introns
    assert S(0, 8, 32, 3, 1, p, p, p, p, p, p, None) == -1 and S(4, 0, 32, 3, 1, p, p, p, p, p, p, None) == -1
    assert S(4, 8, 1025, 3, 1, p, p, p, p, p, p, None) == -1 and S(4, 8, 0, 3, 1, p, p, p, p, p, p, None) == -1
    assert S(4, 8, 32, 0, 1, p, p, p, p, p, p, None) == -1
    assert S(4, 8, 32, 3, 2, p, p, p, p, p, p, None) == -1 and S(4, 8, 32, 3, 0, p, p, p, p, p, p, None) == -1   # multi-output: an argument error
    for k in range(6):
        args = [p] * 6
        args[k] = None
        assert S(4, 8, 32, 3, 1, *args, None) == -2, k
    assert Q(0, 32, p, p, p, p, q, q, q, q, None) == -1 and Q(4, 0, p, p, p, p, q, q, q, q, None) == -1 and Q(4, 1025, p, p, p, p, q, q, q, q, None) == -1
    for k in range(8):
        args = [p, q, r, s, ctypes.c_void_p(80), ctypes.c_void_p(96), ctypes.c_void_p(112), ctypes.c_void_p(128)]
        args[k] = None
        assert Q(4, 32, *args, None) == -2, k
    assert Q(4, 32, p, q, r, s, p, ctypes.c_void_p(96), ctypes.c_void_p(112), q, None) == -1, "not in place"
    assert Q(4, 32, p, q, r, s, ctypes.c_void_p(80), q, ctypes.c_void_p(112), q, None) == -1
    assert Q(4, 32, p, q, r, s, ctypes.c_void_p(80), ctypes.c_void_p(96), r, q, None) == -1
    assert Lb.evogp_hip_abi_version() == _lib.ABI_VERSION
