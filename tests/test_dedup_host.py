"""CPU: the host logic of structural duplicate detection (Forest.structure_hash / duplicate_classes / unique, ``dedup=True`` of
Forest.optimize_constants and Forest.simplify, SymbolicRegression(dedup=), GeneticProgramming(regenerate_duplicates=)) with the numpy
restatements registered as test-only CPU kernels, and the argument checks of the three C entry points, which return before any launch."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cpu_dedup_ops  # noqa: E402
import cpu_grad_ops  # noqa: E402
import cpu_lm_ops  # noqa: E402
import cpu_ops  # noqa: E402
import cpu_subtree_ops  # noqa: E402
import dedup_ref as D  # noqa: E402
import sr_grad_ref  # noqa: E402
import sr_lm_ref  # noqa: E402
import subtree_ref  # noqa: E402
from dedup_cases import half_copies, planted_forest  # noqa: E402

cpu_ops.register()
cpu_grad_ops.register()
cpu_lm_ops.register()
cpu_subtree_ops.register()
cpu_dedup_ops.register()

from evogp_amd.tree import Forest, GenerateDescriptor, set_default_device  # noqa: E402
from evogp_amd.tree import utils as _tree_utils  # noqa: E402


@pytest.fixture(autouse=True)
def _cpu_default_device():
    saved = _tree_utils._DEVICE
    set_default_device("cpu")
    yield
    _tree_utils._DEVICE = saved


def _forest(arrays, out_len=1):
    return Forest(3, out_len, *(torch.from_numpy(a) for a in arrays))


def _bits(t):
    a = t.numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def test_forest_methods(rng):
    value, type_, size = planted_forest(rng, 200, 64)
    f = _forest((value, type_, size), out_len=2)
    h = f.structure_hash()
    assert h.dtype == torch.int64 and h.shape == (200,) and np.array_equal(h.numpy().view(np.uint64), D.tree_hash(value, type_, size))
    cid, first = f.duplicate_classes()
    want = D.class_id(value, type_, size)
    assert cid.dtype == torch.int32 and first.dtype == torch.bool and np.array_equal(cid.numpy(), want)
    assert np.array_equal(first.numpy(), want == np.arange(200))
    fu, inverse, counts = f.unique()
    reps = np.flatnonzero(want == np.arange(200))
    assert fu.pop_size == len(reps) and fu.output_len == 2 and inverse.dtype == torch.int64 and inverse.shape == (200,)
    for a, b in zip(fu._tensors(), (value, type_, size)):
        assert np.array_equal(_bits(a), _bits(torch.from_numpy(b[reps])))   # the representatives, ascending
    assert int(counts.sum()) == 200 and np.array_equal(counts.numpy(), np.bincount(np.searchsorted(reps, want)))
    # forest_u[inverse] is the forest on the live prefixes
    back = fu[inverse]
    live = np.arange(64)[None, :] < np.clip(size[:, :1].astype(np.int64), 1, 64)
    for a, b in zip(back._tensors(), (value, type_, size)):
        assert np.array_equal(_bits(a)[live], _bits(torch.from_numpy(b))[live])
    assert np.array_equal(reps[inverse.numpy()], want)


@pytest.fixture
def handed(monkeypatch):
    """the lengths column of every forest the reference dataset passes are handed, by pass"""
    seen = {"grad": [], "normal_eq": [], "subtree": []}

    def spy(module, name, key):
        real = getattr(module, name)

        def wrapped(value, type_, size, *a, **kw):
            seen[key].append(np.array(size[:, 0]))
            return real(value, type_, size, *a, **kw)

        monkeypatch.setattr(module, name, wrapped)

    spy(sr_grad_ref, "forest_grad", "grad")
    spy(sr_lm_ref, "forest_normal_eq", "normal_eq")
    spy(subtree_ref, "forest_subtree_errors", "subtree")
    return seen


@pytest.mark.parametrize("what", ["descent", "lm", "simplify"])
def test_dedup_changes_no_bit_and_hands_over_the_first_rows_only(rng, handed, what):
    value, type_, size = half_copies(rng, 60, 32)
    f = _forest((value, type_, size))
    keep = [a.clone() for a in f._tensors()]
    X = torch.from_numpy(rng.uniform(0.5, 1.5, (24, 3)).astype(np.float32))
    y = (X[:, :1] * X[:, 1:2] + 0.5).contiguous()
    if what == "simplify":
        run = lambda **kw: f.simplify(X, y, **kw)                                       # noqa: E731
        key, launches = "subtree", 1
    else:
        run = lambda **kw: f.optimize_constants(X, y, steps=2, method=what, **kw)       # noqa: E731
        key, launches = ("grad" if what == "descent" else "normal_eq"), 3
    with np.errstate(all="ignore"):
        plain_f, plain_loss = run()
        assert len(handed[key]) == launches and all(np.array_equal(n, size[:, 0]) for n in handed[key])
        handed[key].clear()
        n_classes = dict(cpu_dedup_ops.calls)
        dedup_f, dedup_loss = run(dedup=True)
    assert cpu_dedup_ops.calls["tree_classes"] == n_classes["tree_classes"] + 1
    for a, b in zip(keep, f._tensors()):
        assert torch.equal(a, b)   # the input forest is untouched
    for a, b in zip(plain_f._tensors(), dedup_f._tensors()):
        assert _same(a, b)
    assert _same(plain_loss, dedup_loss) and torch.isnan(plain_loss).any() and torch.isfinite(plain_loss).any()
    # the dataset passes saw the first rows as they are and every other row as an empty tree
    first = D.class_id(value, type_, size) == np.arange(60)
    assert 25 <= first.sum() <= 32 and first[1] and first[31:].sum() == 1   # (the copy of the n = 0 row is a singleton)
    assert len(handed[key]) == launches
    for n in handed[key]:
        assert np.array_equal(n, np.where(first, size[:, 0], 0))
    assert np.array_equal(dedup_f.batch_subtree_size.numpy()[:, 0] == 0, size[:, 0] == 0)   # no empty row the input did not have


def test_pipeline_scores_are_the_same_with_dedup(rng):
    from evogp_amd.algorithm import DefaultCrossover, DefaultMutation, DefaultSelection, GeneticProgramming
    from evogp_amd.pipeline import StandardPipeline
    from evogp_amd.problem import SymbolicRegression

    d = GenerateDescriptor(max_tree_len=32, input_len=2, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=3,
                           const_samples=[-1, 0, 1])
    X = torch.from_numpy(rng.uniform(0.5, 1.5, (20, 2)).astype(np.float32))
    y = (X[:, :1] * X[:, 1:2]).contiguous()

    def run(dedup):
        torch.manual_seed(11)
        algo = GeneticProgramming(Forest.random_generate(60, d, keys=torch.tensor([1, 2])), DefaultCrossover(), DefaultMutation(0.2, d),
                                  DefaultSelection(0.3, 2))
        problem = SymbolicRegression(datapoints=X, labels=y, const_opt_steps=1, simplify_every=2, dedup=dedup)
        assert problem.dedup is dedup
        pipe = StandardPipeline(algo, problem, generation_limit=3, is_show_details=False)
        with np.errstate(all="ignore"):
            return [pipe.step() for _ in range(3)]

    n0 = cpu_dedup_ops.calls["tree_classes"]
    plain = run(False)
    assert cpu_dedup_ops.calls["tree_classes"] == n0          # off by default: the detection never runs
    deduped = run(True)
    assert cpu_dedup_ops.calls["tree_classes"] == n0 + 3 + 1  # three descents and the simplification of the second generation
    for a, b in zip(plain, deduped):
        assert _same(a, b)


def test_regenerate_duplicates(rng, oracle):
    from evogp_amd.algorithm import DefaultCrossover, DefaultMutation, DefaultSelection, GeneticProgramming

    d = GenerateDescriptor(max_tree_len=32, input_len=2, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=3,
                           const_samples=[-1, 0, 1])
    fitness = torch.from_numpy(rng.uniform(-1, 0, 80).astype(np.float32))

    def run(**kw):
        torch.manual_seed(5)
        algo = GeneticProgramming(Forest.random_generate(80, d, keys=torch.tensor([3, 4])), DefaultCrossover(), DefaultMutation(0.2, d),
                                  DefaultSelection(0.3, 4), **kw)
        return algo.step(fitness)

    n0 = dict(cpu_dedup_ops.calls)
    plain = run()
    assert cpu_dedup_ops.calls == n0   # off by default
    fresh = run(regenerate_duplicates=d.update(max_layer_cnt=4))
    assert cpu_dedup_ops.calls["generate_masked"] == n0["generate_masked"] + 1 and cpu_dedup_ops.calls["tree_classes"] == n0["tree_classes"] + 1
    assert fresh.func_mask == plain.func_mask != 0
    first = plain.duplicate_classes()[1].numpy()
    assert first[0] and 0 < (~first).sum() < 76
    for a, b in zip(plain._tensors(), fresh._tensors()):
        assert np.array_equal(_bits(a)[first], _bits(b)[first])              # first members: untouched, bit for bit
    assert any(not np.array_equal(_bits(a)[~first], _bits(b)[~first]) for a, b in zip(plain._tensors(), fresh._tensors()))
    t, s = fresh.batch_node_type.numpy(), fresh.batch_subtree_size.numpy()
    assert all(oracle.validate_tree(t[i], s[i]) == 0 for i in np.flatnonzero(~first))
    assert int(fresh.duplicate_classes()[1].sum()) >= int(first.sum())       # the class count does not fall
    with pytest.raises(AssertionError):
        GeneticProgramming(plain, DefaultCrossover(), DefaultMutation(0.2, d), DefaultSelection(0.3, 4),
                           regenerate_duplicates=d.update(max_tree_len=16))


def test_argument_errors_without_gpu():
    from evogp_amd import _lib

    L = _lib.lib
    p = 8  # (never dereferenced: the host checks come first)
    assert L.evogp_hip_tree_hash(0, 32, p, p, p, p, None) == -1
    assert L.evogp_hip_tree_hash(4, 0, p, p, p, p, None) == -1
    assert L.evogp_hip_tree_hash(4, 1025, p, p, p, p, None) == -1
    assert L.evogp_hip_tree_hash(4, 32, p, p, None, p, None) == -2
    assert L.evogp_hip_tree_hash(4, 32, p, p, p, None, None) == -2
    b = ctypes.c_ulonglong(0)
    assert L.evogp_hip_tree_classes_workspace_bytes(0, ctypes.byref(b)) == -1
    assert L.evogp_hip_tree_classes_workspace_bytes(4, None) == -2
    assert L.evogp_hip_tree_classes(0, 32, p, p, p, p, p, p, None) == -1
    assert L.evogp_hip_tree_classes(4, 1025, p, p, p, p, p, p, None) == -1
    assert L.evogp_hip_tree_classes(4, 32, p, p, p, None, p, p, None) == -2
    assert L.evogp_hip_tree_classes(4, 32, p, p, p, p, p, None, None) == -2
    assert L.evogp_hip_abi_version() == _lib.ABI_VERSION
