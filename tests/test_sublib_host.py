"""CPU: the population-built subtree library above the kernels -- Forest.SR_subtree_signatures / subtree_library,
SemanticLibrary.update_library(source="subtrees") and the operators' refresh_every -- with the numpy restatement registered as test-only
CPU kernels (tests/cpu_sublib_ops.py), the forest invariants (dead words, row order, slices) of the signature op on it, and the argument
checks of the three C entry points, which return before any launch.  Importing this module also puts the two ops into the invariance and
binding tables (tests/sublib_tables.py)."""
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
import cpu_semantic_ops  # noqa: E402
import cpu_sublib_ops  # noqa: E402
import forest_invariance as FI  # noqa: E402
import sr_grad_ref as R  # noqa: E402
import sublib_ref as SL  # noqa: E402
import sublib_tables as ST  # noqa: E402
import subtree_ref  # noqa: E402
from interval_cases import B, C, V, rows  # noqa: E402

cpu_ops.register()
cpu_dedup_ops.register()
cpu_semantic_ops.register()
cpu_backprop_ops.register()
cpu_agx_ops.register()
cpu_sublib_ops.register()

from evogp_amd import _lib  # noqa: E402
from evogp_amd.algorithm import (ApproxGeometricCrossover, DefaultCrossover, DefaultMutation, SemanticBackpropMutation,  # noqa: E402
                                 SemanticLibrary)
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


def _same(a: Forest, b: Forest):
    return a.pop_size == b.pop_size and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a._tensors(), b._tensors()))


def _data(n=24):
    rng = np.random.default_rng(11)
    return torch.from_numpy(rng.choice(np.setdiff1d(np.arange(-8, 9), [0]), (n, 3)).astype(np.float32) / 4)


def _descriptor(**kw):
    args = dict(max_tree_len=L, input_len=3, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=3, const_samples=[-1, 0, 1])
    args.update(kw)
    return GenerateDescriptor(**args)


BIG = B(R.F_MUL, B(R.F_ADD, V(0), V(1)), B(R.F_SUB, V(2), C(0.5)))          # seven nodes
EXPRS = [BIG, B(R.F_ADD, V(1), V(0)), V(0), B(R.F_MUL, V(0), C(1.0)), B(R.F_DIV, B(R.F_ADD, V(0), V(1)), V(2))]


# ---- the invariants of the signature op on the CPU stand-in, the tables -----------------------------------------------------------------
@pytest.mark.parametrize("case", FI.cases_for(ST.SIGNATURES))
def test_cpu_stand_in_keeps_the_invariants(case):
    FI.check(ST.SIGNATURES, FI.TABLE[ST.SIGNATURES], FI.build_case(case, min(40, FI.CASES[case]["pop"]), 50), "cpu")


def test_the_ops_are_in_both_tables():
    assert FI.cases_for(ST.SIGNATURES) == ["arith_L64", "all_L64_v13", "all_L1024_v40"]
    assert ST.SELECT in FI.EXEMPT and ST.SIGNATURES in ST.BC.TABLE and ST.SELECT in ST.BC.TABLE


# ---- the two Forest methods -------------------------------------------------------------------------------------------------------------
def test_signatures_shape_tails_and_root_column():
    X = _data()
    f = _forest(EXPRS)
    with np.errstate(all="ignore"):
        sig = f.SR_subtree_signatures(X)
        assert sig.shape == (5, L) and sig.dtype == torch.int64 and torch.equal(sig[:, 0], f.semantic_hash(X))
    live = torch.arange(L)[None, :] < f.batch_subtree_size[:, :1]
    assert (sig[live] != 0).all() and (sig[~live] == 0).all()
    assert sig[0, 1] == sig[1, 0] == sig[4, 1] and sig[2, 0] == sig[3, 0] == sig[3, 1] == sig[0, 2]


def test_subtree_library_rows_and_their_signatures():
    X = _data()
    f = _forest(EXPRS)
    with np.errstate(all="ignore"):
        sig = f.SR_subtree_signatures(X)
        lib, counts, tree, node = f.subtree_library(X)
        n_classes = int(SL.select(sig.numpy(), f.batch_subtree_size.numpy(), 1, L, 1024)[2])
        assert lib.pop_size == n_classes == counts.shape[0] == tree.shape[0] == node.shape[0] and counts.dtype == torch.int32
        assert lib.max_tree_len == L and lib.input_len == 3 and lib.output_len == 1 and lib.func_mask == f.func_mask
        assert torch.equal(lib.semantic_hash(X), sig[tree, node]), "a library row computes what the subtree it was cut from computes"
    t, s = lib.batch_node_type.numpy(), lib.batch_subtree_size.numpy()
    assert all(subtree_ref.check_prefix_tree(t[j], s[j]) for j in range(lib.pop_size)), "well-formed rows with zero tails"
    dead = np.arange(L)[None, :] >= s[:, :1]
    assert not _bits(lib.batch_node_value)[dead].any()
    (wv, wt, ws), wtree, wnode = SL.extract(*(a.numpy() for a in f._tensors()), (tree * L + node).numpy())
    assert np.array_equal(_bits(lib.batch_node_value), wv.view(np.uint32)) and np.array_equal(t, wt) and np.array_equal(s, ws)
    assert counts[0] == counts.max() and (counts[:-1] >= counts[1:]).all() and int(counts.sum()) == int((sig != 0).sum())
    assert (tree[0], node[0]) == (0, 2) and counts[0] == 6, "x0: six occurrences, represented by the first lone leaf"
    with np.errstate(all="ignore"):
        small = f.subtree_library(X, k=2, min_size=2, max_size=3)
    assert small[0].pop_size == 2 and ((small[0].batch_subtree_size[:, 0] >= 2) & (small[0].batch_subtree_size[:, 0] <= 3)).all()
    assert (small[2][0], small[3][0]) == (0, 1) and small[1][0] == 3, "x0 + x1 in either order, three times"


def test_argument_errors():
    X = _data()
    f = _forest(EXPRS)
    multi = Forest(3, 2, *f._tensors())
    for call in (lambda: multi.SR_subtree_signatures(X), lambda: multi.subtree_library(X)):
        with pytest.raises(ValueError, match="single-output"):
            call()
    with pytest.raises(ValueError, match="inputs shape"):
        f.SR_subtree_signatures(X[:, :2])
    for kw, msg in ((dict(k=0), "k should"), (dict(k=1025), "k should"), (dict(k=2.0), "k should"), (dict(min_size=0), "min_size"),
                    (dict(min_size=3, max_size=2), "max_size"), (dict(max_size=True), "max_size")):
        with pytest.raises(ValueError, match=msg):
            f.subtree_library(X, **kw)
    lib = SemanticLibrary(X, library=f)
    for call, msg in ((lambda: lib.update_library(f, source="nodes"), "source"), (lambda: lib.update_library(f, max_size=3), "source='subtrees'"),
                      (lambda: lib.update_library(multi, source="subtrees"), "single-output"),
                      (lambda: lib.update_library(f, source="subtrees", min_size=9), "no well-formed subtree")):
        with pytest.raises(ValueError, match=msg):
            with np.errstate(all="ignore"):
                call()
    d = _descriptor()
    for kw in (dict(refresh_every=-1), dict(refresh_every=1.5), dict(refresh_every=True), dict(refresh_max_size=0), dict(refresh_max_size="7")):
        with pytest.raises(ValueError, match="refresh_"):
            SemanticBackpropMutation(0.5, X, X[:, :1], descriptor=d, **kw)
        with pytest.raises(ValueError, match="refresh_"):
            ApproxGeometricCrossover(X, descriptor=d, **kw)


# ---- the library ------------------------------------------------------------------------------------------------------------------------
def test_update_library_without_arguments_is_the_reduction_of_whole_trees():
    X = _data()
    f = _forest(EXPRS)
    with np.errstate(all="ignore"):
        lib = SemanticLibrary(X, library=_forest([V(1)]))
        n0 = dict(cpu_sublib_ops.calls)
        lib.update_library(f)
        want, _, _ = f.semantic_unique(X, keep="smallest")
        assert n0 == cpu_sublib_ops.calls, "the default never looks at subtrees"
        assert _same(lib.library, want) and np.array_equal(_bits(lib.semantics), _bits(want.batch_forward(X)[:, :, 0]))
        op = SemanticBackpropMutation(0.5, X, X[:, :1], library=_forest([V(1)]))
        op.update_library(f)
        assert _same(op.library, want)


def test_subtrees_of_trees_that_are_all_too_large():
    X = _data()
    f = _forest([BIG, B(R.F_SUB, BIG, V(1))])
    with np.errstate(all="ignore"):
        lib = SemanticLibrary(X, library=_forest([V(1)]))
        lib.update_library(f, source="subtrees", max_size=3)
        sizes = lib.library.batch_subtree_size[:, 0]
        assert lib.library.pop_size == 6 and int(sizes.max()) == 3, "x0, x1, x2, 0.5, x0 + x1, x2 - 0.5"
        assert np.array_equal(_bits(lib.semantics), _bits(lib.library.batch_forward(X)[:, :, 0])) and lib.semantics.shape == (6, 24)
        want = f.subtree_library(X, 1024, 1, 3)[0].semantic_unique(X, keep="smallest")[0]
        assert _same(lib.library, want)
        agx = ApproxGeometricCrossover(X, library=lib)
        rdo = SemanticBackpropMutation(0.5, X, X[:, :1], library=lib)
        agx.update_library(f, source="subtrees", min_size=3, max_size=3)
        assert rdo.library.pop_size == 2 and (rdo.library.batch_subtree_size[:, 0] == 3).all(), "a shared library changes for both"


def test_refresh_every_rebuilds_on_every_nth_call():
    rng = np.random.default_rng(3)
    X = torch.from_numpy(rng.uniform(0.5, 1.5, (24, 3)).astype(np.float32))
    y = (X[:, :1] * X[:, 1:2] + X[:, 2:3]).contiguous()
    d = _descriptor()
    torch.manual_seed(5)
    with np.errstate(all="ignore"):
        shared = SemanticLibrary(X, descriptor=d, library_size=20)
        rdo = SemanticBackpropMutation(0.5, X, y, library=shared, fallback=DefaultMutation(0.5, d), refresh_every=2, refresh_max_size=5)
        agx = ApproxGeometricCrossover(X, library=shared, fallback=DefaultCrossover())
        static = SemanticBackpropMutation(0.5, X, y, library=_forest([V(0), V(1)]))
        f = Forest.random_generate(30, d, keys=torch.tensor([5, 6]))
        seen, builds = [], []
        for call in range(1, 5):
            n0 = cpu_sublib_ops.calls["library_select"]
            before = shared.library
            handed = Forest(3, 1, *(a.clone() for a in f._tensors()))
            f = rdo(f)
            builds.append(cpu_sublib_ops.calls["library_select"] - n0)
            if builds[-1]:
                assert shared.library is not before and agx.library is shared.library
                want = handed.subtree_library(X, 1024, 1, 5)[0].semantic_unique(X, keep="smallest")[0]
                assert _same(shared.library, want) and int(shared.library.batch_subtree_size[:, 0].max()) <= 5
            else:
                assert shared.library is before
            seen.append(shared.library)
            survivors = torch.arange(10)
            f = agx(f, survivors, 30, torch.zeros(30))
            static(f)
        assert builds == [0, 1, 0, 1], "calls 2 and 4 only; the crossover and the static operator never rebuild"
        assert f.pop_size == 30 and shared.library.pop_size <= 1024


# ---- the C entry points -------------------------------------------------------------------------------------------------------------------
def test_c_entry_points_check_their_arguments():
    Lb = _lib.lib
    p = ctypes.c_void_p(16)   # never dereferenced: every call below returns from its argument checks
    S, W, Q = Lb.evogp_hip_sr_subtree_signatures, Lb.evogp_hip_subtree_library_select_workspace_bytes, Lb.evogp_hip_subtree_library_select
    assert S(0, 8, 32, 3, 1, p, p, p, p, p, None) == -1 and S(4, 0, 32, 3, 1, p, p, p, p, p, None) == -1
    assert S(4, 8, 1025, 3, 1, p, p, p, p, p, None) == -1 and S(4, 8, 32, 0, 1, p, p, p, p, p, None) == -1
    assert S(4, 8, 32, 3, 2, p, p, p, p, p, None) == -1 and S(4, 8, 32, 3, 0, p, p, p, p, p, None) == -1      # multi-output: an argument error
    assert S(4, 8, 32, 3, 1, None, p, p, p, p, None) == -2 and S(4, 8, 32, 3, 1, p, p, p, p, None, None) == -2
    b = ctypes.c_ulonglong(0)
    assert W(0, 64, ctypes.byref(b)) == -1 and W(4, 1025, ctypes.byref(b)) == -1 and W(1 << 22, 1024, ctypes.byref(b)) == -1
    assert W(4, 64, None) == -2
    for bad in ((0, 64, 1, 64, 8), (4, 0, 1, 64, 8), (4, 1025, 1, 64, 8), (1 << 22, 1024, 1, 64, 8), (4, 64, 0, 64, 8), (4, 64, 3, 2, 8),
                (4, 64, 1, 64, 0), (4, 64, 1, 64, 1025)):
        assert Q(bad[0], bad[1], p, p, bad[2], bad[3], bad[4], p, p, p, p, None) == -1, bad
    assert Q(4, 64, None, p, 1, 64, 8, p, p, p, p, None) == -2 and Q(4, 64, p, p, 1, 64, 8, p, p, p, None, None) == -2
    assert Lb.evogp_hip_abi_version() == _lib.ABI_VERSION
