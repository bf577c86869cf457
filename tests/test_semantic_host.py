"""CPU: the host logic of semantic duplicate classes (Forest.semantic_hash / semantic_classes / semantic_unique,
SymbolicRegression(semantic_dedup=), GeneticProgramming(duplicate_classes=)) with the numpy restatement registered as test-only CPU
kernels, and the argument checks of the four C entry points, which return before any launch."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cpu_dedup_ops  # noqa: E402
import cpu_ops  # noqa: E402
import cpu_scale_ops  # noqa: E402
import cpu_semantic_ops  # noqa: E402
import semantic_ref as S  # noqa: E402
from semantic_cases import dataset, planted_forest  # noqa: E402

cpu_ops.register()
cpu_dedup_ops.register()
cpu_scale_ops.register()
cpu_semantic_ops.register()

from evogp_amd.tree import Forest, GenerateDescriptor, set_default_device  # noqa: E402
from evogp_amd.tree import utils as _tree_utils  # noqa: E402


@pytest.fixture(autouse=True)
def _cpu_default_device():
    saved = _tree_utils._DEVICE
    set_default_device("cpu")
    yield
    _tree_utils._DEVICE = saved


def _bits(t):
    a = t.numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.fixture(scope="module")
def planted():
    rng = np.random.default_rng(20261019)
    value, type_, size = planted_forest(rng, 120, 64)
    X = dataset(rng, 70)
    from oracle.pyoracle import Oracle

    with np.errstate(all="ignore"):
        P, formed = S.oracle_predictions(Oracle("port"), value, type_, size, X)
    return (value, type_, size), X, S.class_id(P, formed), S.signature(P, formed)


def test_forest_methods(planted):
    (value, type_, size), X, want, want_sig = planted
    pop = len(want)
    f = Forest(3, 1, *(torch.from_numpy(a) for a in (value, type_, size)))
    Xt = torch.from_numpy(X)
    with np.errstate(all="ignore"):
        h = f.semantic_hash(Xt)
        cid, rep = f.semantic_classes(Xt)
        cid_s, rep_s = f.semantic_classes(Xt, keep="smallest")
        fu, inverse, counts = f.semantic_unique(Xt, keep="smallest")
    assert h.dtype == torch.int64 and h.shape == (pop,) and np.array_equal(h.numpy().view(np.uint64), want_sig)
    assert cid.dtype == torch.int32 and rep.dtype == torch.bool and np.array_equal(cid.numpy(), want)
    assert np.array_equal(rep.numpy(), want == np.arange(pop))
    nodes = np.clip(size[:, 0].astype(np.int64), 0, 64)
    small = S.smallest_representative(want, nodes)
    assert cid_s.dtype == torch.int32 and np.array_equal(cid_s.numpy(), small) and np.array_equal(rep_s.numpy(), small == np.arange(pop))
    assert (small != want).any() and small[10] == small[11] == small[12] == 9   # T * 1, T + 0, neg(neg(T)) -> T
    assert (nodes[small] <= nodes).all()
    reps = np.flatnonzero(small == np.arange(pop))
    assert fu.pop_size == len(reps) and inverse.dtype == torch.int64 and np.array_equal(reps[inverse.numpy()], small)
    assert int(counts.sum()) == pop and np.array_equal(counts.numpy(), np.bincount(np.searchsorted(reps, small)))
    for a, b in zip(fu._tensors(), (value, type_, size)):
        assert np.array_equal(_bits(a), _bits(torch.from_numpy(b[reps])))


def test_forest_argument_errors(planted):
    (value, type_, size), X, _, _ = planted
    tensors = [torch.from_numpy(a) for a in (value, type_, size)]
    f = Forest(3, 1, *tensors)
    Xt = torch.from_numpy(X)
    n0 = dict(cpu_semantic_ops.calls)
    with pytest.raises(ValueError, match="keep"):
        f.semantic_classes(Xt, keep="largest")
    with pytest.raises(ValueError, match="inputs shape"):
        f.semantic_hash(Xt[:, :2])
    with pytest.raises(ValueError, match="inputs shape"):
        f.semantic_classes(Xt[:0])
    multi = Forest(3, 2, *tensors)
    for call in (lambda: multi.semantic_hash(Xt), lambda: multi.semantic_classes(Xt), lambda: multi.semantic_unique(Xt)):
        with pytest.raises(ValueError, match="single-output"):
            call()
    assert cpu_semantic_ops.calls == n0   # every check comes before the first launch


def test_problem_masks_everything_but_the_representatives(planted):
    from evogp_amd.problem import SymbolicRegression

    (value, type_, size), X, want, _ = planted
    pop = len(want)
    f = Forest(3, 1, *(torch.from_numpy(a) for a in (value, type_, size)))
    Xt = torch.from_numpy(X)
    y = (Xt[:, :1] * Xt[:, 1:2] - Xt[:, 2:3] / 1.5).contiguous()
    small = S.smallest_representative(want, np.clip(size[:, 0].astype(np.int64), 0, 64))
    n0 = dict(cpu_semantic_ops.calls)
    with np.errstate(all="ignore"):
        plain = SymbolicRegression(datapoints=Xt, labels=y)
        assert plain.semantic_dedup is False and plain.semantic_keep == "smallest"
        base_scores, base_fit = plain.scores(f), plain.evaluate(f)
        assert cpu_semantic_ops.calls == n0   # off by default: the detection never runs
        cid, rep = plain.semantic_classes(f)
        assert np.array_equal(cid.numpy(), small)
        for keep, classes in (("smallest", small), ("first", want)):
            prob = SymbolicRegression(datapoints=Xt, labels=y, semantic_dedup=True, semantic_keep=keep)
            is_rep = classes == np.arange(pop)
            scores, fit = prob.scores(f), prob.evaluate(f)
            assert np.array_equal(_bits(scores)[is_rep], _bits(base_scores)[is_rep]) and np.isneginf(scores.numpy()[~is_rep]).all()
            assert np.array_equal(_bits(fit)[is_rep], _bits(base_fit)[is_rep]) and np.isnan(fit.numpy()[~is_rep]).all()
            assert np.isfinite(scores.numpy()[is_rep]).sum() > 40 and (~is_rep).sum() > 15
        # under linear scaling the UNSCALED predictions are compared: the same classes, the scaled loss of the representatives
        scaled = SymbolicRegression(datapoints=Xt, labels=y, linear_scaling=True)
        both = SymbolicRegression(datapoints=Xt, labels=y, linear_scaling=True, semantic_dedup=True)
        is_rep = small == np.arange(pop)
        a, b = scaled.scores(f), both.scores(f)
        assert np.array_equal(_bits(a)[is_rep], _bits(b)[is_rep]) and np.isneginf(b.numpy()[~is_rep]).all()
        assert np.array_equal(both.semantic_classes(f)[0].numpy(), small)
    with pytest.raises(ValueError, match="multigene"):
        SymbolicRegression(datapoints=Xt, labels=y, multigene=True, semantic_dedup=True)
    with pytest.raises(ValueError, match="semantic_keep"):
        SymbolicRegression(datapoints=Xt, labels=y, semantic_keep="largest")
    with pytest.raises(ValueError, match="single-output"):
        SymbolicRegression(datapoints=Xt, labels=torch.cat([y, y], dim=1), semantic_dedup=True)


def test_regenerate_semantic_duplicates(rng, oracle):
    from evogp_amd.algorithm import DefaultCrossover, DefaultMutation, DefaultSelection, GeneticProgramming
    from evogp_amd.problem import SymbolicRegression

    d = GenerateDescriptor(max_tree_len=32, input_len=2, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=3,
                           const_samples=[-1, 0, 1])
    fitness = torch.from_numpy(rng.uniform(-1, 0, 80).astype(np.float32))
    X = torch.from_numpy(rng.uniform(0.5, 1.5, (20, 2)).astype(np.float32))
    problem = SymbolicRegression(datapoints=X, labels=(X[:, :1] * X[:, 1:2]).contiguous())

    def run(**kw):
        torch.manual_seed(5)
        algo = GeneticProgramming(Forest.random_generate(80, d, keys=torch.tensor([3, 4])), DefaultCrossover(), DefaultMutation(0.2, d),
                                  DefaultSelection(0.3, 4), **kw)
        return algo.step(fitness)

    n0, d0 = dict(cpu_semantic_ops.calls), dict(cpu_dedup_ops.calls)
    with np.errstate(all="ignore"):
        plain = run()
        assert cpu_semantic_ops.calls == n0 and cpu_dedup_ops.calls == d0   # off by default
        structural = run(regenerate_duplicates=d.update(max_layer_cnt=4))
        # the default path is today's: Forest.duplicate_classes, no semantic op
        assert cpu_semantic_ops.calls == n0 and cpu_dedup_ops.calls["tree_classes"] == d0["tree_classes"] + 1
        fresh = run(regenerate_duplicates=d.update(max_layer_cnt=4), duplicate_classes=problem.semantic_classes)
        assert cpu_semantic_ops.calls["semantic_classes"] == n0["semantic_classes"] + 1
        assert cpu_dedup_ops.calls["tree_classes"] == d0["tree_classes"] + 1   # (and no structural pass)
        rep = problem.semantic_classes(plain)[1].numpy()
        first = plain.duplicate_classes()[1].numpy()
        after = problem.semantic_classes(fresh)[1].numpy()
    assert (~rep).sum() > (~first).sum() > 0  # semantic duplicates hold the structural ones and more
    for a, b in zip(plain._tensors(), fresh._tensors()):
        assert np.array_equal(_bits(a)[rep], _bits(b)[rep])                  # representatives: untouched, bit for bit
    assert any(not np.array_equal(_bits(a)[~rep], _bits(b)[~rep]) for a, b in zip(plain._tensors(), fresh._tensors()))
    assert any(not np.array_equal(_bits(a), _bits(b)) for a, b in zip(structural._tensors(), fresh._tensors()))
    t, s = fresh.batch_node_type.numpy(), fresh.batch_subtree_size.numpy()
    assert all(oracle.validate_tree(t[i], s[i]) == 0 for i in np.flatnonzero(~rep))
    assert int(after.sum()) >= int(rep.sum())                                # the semantic class count does not fall
    with pytest.raises(TypeError, match="duplicate_classes"):
        GeneticProgramming(plain, DefaultCrossover(), DefaultMutation(0.2, d), DefaultSelection(0.3, 4), duplicate_classes="semantic")


def test_argument_errors_without_gpu():
    from evogp_amd import _lib

    L = _lib.lib
    p = 8  # (never dereferenced: the host checks come first)
    b = ctypes.c_ulonglong(0)
    for name in ("evogp_hip_sr_semantic_hash_workspace_bytes", "evogp_hip_sr_semantic_classes_workspace_bytes"):
        fn = getattr(L, name)
        assert fn(0, ctypes.byref(b)) == -1 and fn(2**31, ctypes.byref(b)) == -1 and fn(4, None) == -2
    assert L.evogp_hip_sr_semantic_hash_workspace_bytes(1000, ctypes.byref(b)) == 0 and b.value >= 1000
    H, Cl = L.evogp_hip_sr_semantic_hash, L.evogp_hip_sr_semantic_classes
    for bad in ((0, 8, 32, 3, 1), (4, 0, 32, 3, 1), (4, 8, 0, 3, 1), (4, 8, 1025, 3, 1), (4, 8, 32, 0, 1), (4, 8, 32, 3, 0), (2**31, 8, 32, 3, 1)):
        assert H(*bad, p, p, p, p, p, p, None) == -1 and Cl(*bad, p, p, p, p, p, p, p, None) == -1
    assert H(4, 8, 32, 3, 2, p, p, p, p, p, p, None) == -3 and Cl(4, 8, 32, 3, 2, p, p, p, p, p, p, p, None) == -3   # multi-output: unsupported
    for k in range(6):
        args = [p] * 6
        args[k] = None
        assert H(4, 8, 32, 3, 1, *args, None) == -2
    for k in range(7):
        args = [p] * 7
        args[k] = None
        assert Cl(4, 8, 32, 3, 1, *args, None) == -2
    assert L.evogp_hip_abi_version() == _lib.ABI_VERSION
