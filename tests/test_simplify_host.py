"""CPU: the host logic of tree simplification (Forest.SR_subtree_errors, Forest.simplify, SymbolicRegression(simplify_every=),
StandardPipeline) with the numpy restatement registered as test-only CPU kernels (tests/cpu_subtree_ops.py), and the argument
checks of the two new C entry points, which return before any launch."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cpu_grad_ops  # noqa: E402
import cpu_ops  # noqa: E402
import cpu_subtree_ops  # noqa: E402
import sr_grad_ref as R  # noqa: E402
import subtree_ref as S  # noqa: E402
from grad_trees import ALL_FUNCS, random_forest  # noqa: E402

cpu_ops.register()
cpu_grad_ops.register()
cpu_subtree_ops.register()

from evogp_amd.tree import Forest, GenerateDescriptor, set_default_device  # noqa: E402
from evogp_amd.tree import utils as _tree_utils  # noqa: E402


@pytest.fixture(autouse=True)
def _cpu_default_device():
    saved = _tree_utils._DEVICE
    set_default_device("cpu")
    yield
    _tree_utils._DEVICE = saved


def _data(rng, D=40, var_len=2):
    X = rng.uniform(0.5, 1.5, (D, var_len)).astype(np.float32)
    y = (X[:, :1] * X[:, 1:2]).astype(np.float32)
    return torch.from_numpy(X), torch.from_numpy(y)


def test_forest_simplify_invariants(rng):
    value, type_, size = random_forest(rng, 80, 32, ALL_FUNCS, 2, 1, max_depth=4)
    size[3, 0] = 0   # malformed
    # x0 * x1 * 3 with y = x0 * x1: the product is hoisted
    value[4, :5] = [R.F_MUL, R.F_MUL, 0, 1, 3.0]
    type_[4, :5] = [R.T_BFUNC, R.T_BFUNC, R.T_VAR, R.T_VAR, R.T_CONST]
    size[4, :5] = [5, 3, 1, 1, 1]
    X, y = _data(rng)
    f0 = Forest(2, 1, *(torch.from_numpy(a) for a in (value, type_, size)), func_mask=(1 << 29) - 1)
    keep = [a.clone() for a in f0._tensors()]
    node_err, node_const = f0.SR_subtree_errors(X, y)
    assert node_err.shape == node_const.shape == (80, 32) and node_err.dtype == torch.float32
    f1, loss = f0.simplify(X, y)
    for a, b in zip(keep, f0._tensors()):
        assert torch.equal(a, b)   # the input forest is untouched
    assert f1 is not f0 and f1.func_mask == f0.func_mask != 0
    v1, t1, s1 = (a.numpy() for a in f1._tensors())
    assert np.all(s1[:, 0] <= np.maximum(size[:, 0], 0)) and (s1[:, 0] < size[:, 0]).any()
    assert list(t1[4, :4]) == [R.T_BFUNC, R.T_VAR, R.T_VAR, 0] and list(s1[4, :4]) == [3, 1, 1, 0] and float(loss[4]) == 0.0
    assert np.isnan(float(loss[3])) and np.array_equal(v1[3].view(np.uint32), value[3].view(np.uint32)) and np.array_equal(s1[3], size[3])
    for t in range(80):
        if t != 3:
            assert S.check_prefix_tree(t1[t], s1[t])
    # the returned loss is the returned forest's own loss, and simplifying again changes nothing
    e1, _ = f1.SR_subtree_errors(X, y)
    assert np.array_equal(e1[:, 0].numpy().view(np.uint32)[np.arange(80) != 3], loss.numpy().view(np.uint32)[np.arange(80) != 3])
    f2, loss2 = f1.simplify(X, y)
    for a, b in zip(f1._tensors(), f2._tensors()):
        assert torch.equal(a, b)
    assert np.array_equal(loss.numpy().view(np.uint32), loss2.numpy().view(np.uint32))
    # the switches reach the op
    f3, _ = f0.simplify(X, y, hoist=False, fold_constants=False)
    live = np.arange(32)[None, :] < np.clip(size[:, :1], 0, 32)
    ok = np.arange(80) != 3
    assert np.array_equal(f3.batch_node_type.numpy()[ok][live[ok]], type_[ok][live[ok]])
    assert np.array_equal(f3.batch_subtree_size.numpy()[ok][:, 0], size[ok][:, 0])


def test_simplify_refuses_multi_output_forests(rng):
    value, type_, size = random_forest(rng, 4, 32, ALL_FUNCS, 2, 3, max_depth=3)
    f = Forest(2, 3, *(torch.from_numpy(a) for a in (value, type_, size)))
    X = torch.zeros(5, 2)
    y = torch.zeros(5, 3)
    with pytest.raises(AssertionError):
        f.simplify(X, y)
    with pytest.raises(AssertionError):
        f.SR_subtree_errors(X, y)


def test_optimize_simplifies_on_every_kth_call(rng):
    from evogp_amd.problem import SymbolicRegression

    value, type_, size = random_forest(rng, 20, 32, ALL_FUNCS, 2, 1, max_depth=4)
    forest = Forest(2, 1, *(torch.from_numpy(a) for a in (value, type_, size)))
    X, y = _data(rng)
    # the defaults: the very same forest object comes back and no kernel runs
    before = dict(cpu_subtree_ops.calls)
    plain = SymbolicRegression(datapoints=X, labels=y)
    assert plain.simplify_every == 0 and plain.const_opt_steps == 0
    assert plain.optimize(forest) is forest and plain.optimize(forest) is forest
    assert cpu_subtree_ops.calls == before
    for k in (1, 3):
        prob = SymbolicRegression(datapoints=X, labels=y, simplify_every=k)
        rewrote = []
        for _ in range(7):
            n0 = cpu_subtree_ops.calls["prune"]
            out = prob.optimize(forest)
            did = cpu_subtree_ops.calls["prune"] - n0
            assert did in (0, 1) and (out is forest) == (did == 0)
            rewrote.append(did)
        assert rewrote == [1 if (i + 1) % k == 0 else 0 for i in range(7)]
    with pytest.raises(AssertionError):
        SymbolicRegression(datapoints=X, labels=y, simplify_every=-1)
    # together with the constant descent: simplify first, then the descent on the simplified forest
    both = SymbolicRegression(datapoints=X, labels=y, simplify_every=1, const_opt_steps=2)
    out = both.optimize(forest)
    want = forest.simplify(X, y)[0].optimize_constants(X, y, 2, 0.1)[0]
    for a, b in zip(out._tensors(), want._tensors()):
        assert torch.equal(a, b)


def test_pipeline_scores_and_breeds_the_simplified_forest(rng):
    from evogp_amd.algorithm import DefaultCrossover, DefaultMutation, DefaultSelection, GeneticProgramming
    from evogp_amd.pipeline import StandardPipeline
    from evogp_amd.problem import SymbolicRegression

    d = GenerateDescriptor(max_tree_len=32, input_len=2, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=4,
                           const_samples=[-1, 0, 1])
    X, y = _data(rng)

    def pipeline(**kw):
        algo = GeneticProgramming(Forest.random_generate(60, d, keys=torch.tensor([1, 2])), DefaultCrossover(), DefaultMutation(0.2, d),
                                  DefaultSelection(0.3, 2))
        return algo, StandardPipeline(algo, SymbolicRegression(datapoints=X, labels=y, **kw), generation_limit=2, is_show_details=False)

    algo, pipe = pipeline(simplify_every=1)
    start = algo.forest
    simplified = start.simplify(X, y)[0]
    n0 = cpu_subtree_ops.calls["prune"]
    host = pipe.step()
    assert cpu_subtree_ops.calls["prune"] == n0 + 1
    want = -simplified.SR_fitness(X, y)
    np.testing.assert_allclose(host.numpy(), torch.where(torch.isnan(want), torch.full_like(want, float("-inf")), want).numpy(), rtol=1e-5)
    best = int(torch.argmax(host))
    assert torch.equal(pipe.best_tree.node_value, simplified[best].node_value)
    pipe.step()
    assert cpu_subtree_ops.calls["prune"] == n0 + 2
    # with both options at 0 the pipeline never calls optimize's kernels and scores the forest it was given
    algo, pipe = pipeline()
    start = algo.forest
    n0 = dict(cpu_subtree_ops.calls)
    host = pipe.step()
    assert cpu_subtree_ops.calls == n0
    want = -start.SR_fitness(X, y)
    np.testing.assert_allclose(host.numpy(), torch.where(torch.isnan(want), torch.full_like(want, float("-inf")), want).numpy(), rtol=1e-5)


def test_argument_errors_without_gpu():
    from evogp_amd import _lib

    L = _lib.lib
    p = 8  # (never dereferenced: the host checks come first)
    assert L.evogp_hip_sr_subtree_errors(0, 8, 32, 3, 1, 1, p, p, p, p, p, p, p, None) == -1
    assert L.evogp_hip_sr_subtree_errors(4, 0, 32, 3, 1, 1, p, p, p, p, p, p, p, None) == -1
    assert L.evogp_hip_sr_subtree_errors(4, 8, 1025, 3, 1, 1, p, p, p, p, p, p, p, None) == -1
    assert L.evogp_hip_sr_subtree_errors(4, 8, 32, 3, 2, 1, p, p, p, p, p, p, p, None) == -1      # multi-output
    assert L.evogp_hip_sr_subtree_errors(4, 8, 32, 3, 0, 1, p, p, p, p, p, p, p, None) == -1
    assert L.evogp_hip_sr_subtree_errors(4, 8, 32, 3, 1, 1, p, p, p, p, p, p, None, None) == -2
    assert L.evogp_hip_sr_subtree_errors(4, 8, 32, 3, 1, 1, None, p, p, p, p, p, p, None) == -2
    q = 16
    assert L.evogp_hip_prune_rows(0, 32, 1, 1, 1, p, p, p, p, p, q, q, q, q, q, None) == -1
    assert L.evogp_hip_prune_rows(4, 1025, 1, 1, 1, p, p, p, p, p, q, q, q, q, q, None) == -1
    assert L.evogp_hip_prune_rows(4, 32, 2, 1, 1, p, p, p, p, p, q, q, q, q, q, None) == -1       # multi-output
    assert L.evogp_hip_prune_rows(4, 32, 1, 1, 1, p, p, p, p, p, p, q, q, q, q, None) == -1       # in place
    assert L.evogp_hip_prune_rows(4, 32, 1, 1, 1, p, p, p, None, p, q, q, q, q, q, None) == -2
    assert L.evogp_hip_prune_rows(4, 32, 1, 1, 1, p, p, p, p, p, q, q, q, q, None, None) == -2
    assert _lib.ABI_VERSION == 9 == L.evogp_hip_abi_version()
