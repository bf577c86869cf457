"""CPU: the host logic of the classification statistics (Forest.class_stats, Classification(metric=, validation_mask=), StandardPipeline's
validation tracking on a classifier) with the numpy restatement registered as a test-only CPU kernel (tests/cpu_cls_ops.py), and the
argument checks of the new C entry point, which return before any launch.  Importing this module also puts the op into the invariance
and binding tables (tests/cls_tables.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cls_ref as CR  # noqa: E402
import cls_tables  # noqa: E402,F401
import cpu_cls_ops  # noqa: E402
import cpu_ops  # noqa: E402
from grad_trees import ARITH, random_forest  # noqa: E402

cpu_ops.register()
cpu_cls_ops.register()

from evogp_amd import _lib  # noqa: E402
from evogp_amd.problem import Classification  # noqa: E402
from evogp_amd.problem.classification import METRICS  # noqa: E402
from evogp_amd.tree import Forest, GenerateDescriptor, set_default_device  # noqa: E402
from evogp_amd.tree import utils as _tree_utils  # noqa: E402

D, V, C = 60, 3, 3


@pytest.fixture(autouse=True)
def _cpu_default_device():
    saved = _tree_utils._DEVICE
    set_default_device("cpu")
    yield
    _tree_utils._DEVICE = saved


def _data(rng):
    X = rng.uniform(-1.5, 1.5, (D, V)).astype(np.float32)
    y = rng.integers(0, C, D).astype(np.float32)      # float labels holding integers, as the sklearn loaders give them
    return torch.from_numpy(X), torch.from_numpy(y)


def _forest(rng, pop=24):
    value, type_, size = random_forest(rng, pop, 32, ARITH, V, C, max_depth=4)
    return Forest(V, C, *(torch.from_numpy(a) for a in (value, type_, size)))


def _mask(rng):
    m = torch.from_numpy(rng.random(D) < 0.35)
    m[0], m[1] = True, False
    return m


def _sklearn_scores(metric, forest, X, y):
    import sklearn.metrics as sk
    f = tuple(a.numpy() for a in forest._tensors())
    outs = CR.outputs(*f, X.numpy(), C)
    pred = CR.predict(outs)
    yi = y.numpy().astype(np.int64)
    out = np.zeros(len(pred))
    for t in range(len(pred)):
        if metric == "accuracy":
            out[t] = sk.accuracy_score(yi, pred[t])
        elif metric == "balanced_accuracy":
            out[t] = sk.balanced_accuracy_score(yi, pred[t])
        elif metric == "f1_macro":
            out[t] = sk.f1_score(yi, pred[t], average="macro", labels=sorted(set(yi.tolist())))
        elif metric == "mcc":
            out[t] = sk.matthews_corrcoef(yi, pred[t])
        else:
            o = outs[t].astype(np.float64)
            if not np.isfinite(o).all():
                out[t] = -np.inf
                continue
            z = o - o.max(1, keepdims=True)
            prob = np.exp(z) / np.exp(z).sum(1, keepdims=True)
            out[t] = -sk.log_loss(yi, np.clip(prob, 1e-15, 1.0), labels=list(range(C)))
    return out


@pytest.mark.filterwarnings("ignore")
@pytest.mark.parametrize("metric", METRICS)
def test_every_metric_against_sklearn(rng, metric):
    X, y = _data(rng)
    forest = _forest(rng)
    got = Classification(X, y, metric=metric).evaluate(forest)
    assert got.dtype == torch.float32 and got.shape == (forest.pop_size,)
    want = _sklearn_scores(metric, forest, X, y)
    got = got.numpy().astype(np.float64)
    assert np.array_equal(np.isneginf(got), np.isneginf(want))
    fin = np.isfinite(want)
    assert fin.sum() >= forest.pop_size // 2
    assert np.abs(got[fin] - want[fin]).max() <= 1e-5 + 1e-6 * np.abs(want[fin]).max()


def test_accuracy_is_the_old_path_and_equals_the_new_one(rng):
    X, y = _data(rng)
    forest = _forest(rng)
    prob = Classification(X, y)
    n0 = cpu_cls_ops.calls["class_stats"]
    old = prob.evaluate(forest)
    assert cpu_cls_ops.calls["class_stats"] == n0, "metric='accuracy' without a mask takes the reference's path"
    assert torch.equal(old, prob._accuracy(forest.batch_forward(X)))
    assert torch.equal(prob._score(prob.class_stats(forest), 0), old)
    hits, predicted, loss = prob.class_stats(forest)
    assert hits.shape == (forest.pop_size, 1, C) == predicted.shape and loss.shape == (forest.pop_size, 1)
    assert hits.dtype == torch.int32 == predicted.dtype and loss.dtype == torch.float64
    assert bool((predicted.sum((1, 2)) == D).all()) and bool((hits <= predicted).all())


@pytest.mark.parametrize("metric", METRICS)
def test_a_validation_mask_column_equals_a_call_on_those_rows(rng, metric):
    X, y = _data(rng)
    forest = _forest(rng)
    m = _mask(rng)
    prob = Classification(X, y, metric=metric, validation_mask=m)
    n0 = cpu_cls_ops.calls["class_stats"]
    train = prob.evaluate(forest)
    held = prob.validation_scores(forest, train)
    assert cpu_cls_ops.calls["class_stats"] == n0 + 1, "the validation scores come out of the launch behind the fitness"
    own_train = Classification(X[~m], y[~m], metric=metric).evaluate(forest)
    own_held = Classification(X[m], y[m], metric=metric).evaluate(forest)
    own_train, own_held = (torch.where(torch.isnan(a), torch.full_like(a, float("-inf")), a) for a in (own_train, own_held))
    assert torch.equal(train, own_train)
    assert torch.equal(held, torch.where(train == float("-inf"), torch.full_like(own_held, float("-inf")), own_held))
    assert torch.equal(prob.validation_scores(forest), held)
    # the cache follows the forest: an edit in place is a new forest
    n1 = cpu_cls_ops.calls["class_stats"]
    prob.evaluate(forest)
    assert cpu_cls_ops.calls["class_stats"] == n1
    forest.batch_node_value[0, 0] += 1.0
    prob.evaluate(forest)
    assert cpu_cls_ops.calls["class_stats"] == n1 + 1


def test_forest_class_stats_takes_bool_and_int_groups(rng):
    X, y = _data(rng)
    forest = _forest(rng)
    m = _mask(rng)
    f = tuple(a.numpy() for a in forest._tensors())
    h, p, l = forest.class_stats(X, y, m)
    wh, wp, wl, _ = CR.forest_stats(f, X.numpy(), y.numpy(), C, m.numpy().astype(np.int32), 2)
    assert np.array_equal(h.numpy(), wh) and np.array_equal(p.numpy(), wp) and np.array_equal(np.isnan(l.numpy()), np.isnan(wl))
    g = torch.from_numpy(np.arange(D) % 10 - 1)       # int64, values -1 .. 8 with 8 splits: -1 and 8 are skipped
    h8, p8, l8 = forest.class_stats(X, y.to(torch.int64), g, 8)
    assert h8.shape == (forest.pop_size, 8, C) and int(p8[0].sum()) == int(((g >= 0) & (g < 8)).sum())
    one = forest.class_stats(X, y)
    assert one[0].shape == (forest.pop_size, 1, C) and torch.equal(one[0][:, 0], h.sum(1))


def test_the_value_errors(rng):
    X, y = _data(rng)
    forest = _forest(rng)
    n0 = cpu_cls_ops.calls["class_stats"]
    with pytest.raises(ValueError):
        Classification(X, y, metric="auc")
    for kw in (dict(metric="mcc"), dict(validation_mask=_mask(rng))):
        with pytest.raises(ValueError):
            Classification(X, y, multi_output=False, **kw)
    with pytest.raises(ValueError):
        Classification(X, y + 0.5, metric="cross_entropy")            # labels that name no class
    for bad in (torch.zeros(D), torch.zeros(D + 1, dtype=torch.bool)):
        with pytest.raises(ValueError):
            Classification(X, y, validation_mask=bad)
    with pytest.raises(ValueError):
        Classification(X, y).validation_scores(forest)
    single = Forest(V, 1, *(torch.from_numpy(a) for a in random_forest(rng, 4, 32, ARITH, V, 1, max_depth=3)))
    with pytest.raises(ValueError):
        single.class_stats(X, y)
    for args in ((X[:, :2], y), (X, y[:-1]), (X, y + 0.5), (X, y > 0), (X, y, torch.zeros(D)), (X, y, torch.zeros(D, dtype=torch.int32)),
                 (X, y, torch.zeros(D, dtype=torch.int32), 9), (X, y, torch.zeros(D, dtype=torch.int32), 0), (X, y, None, 2),
                 (X, y, torch.zeros(D + 1, dtype=torch.bool))):
        with pytest.raises(ValueError):
            forest.class_stats(*args)
    assert cpu_cls_ops.calls["class_stats"] == n0   # every check comes before the first launch


def test_pipeline_with_validation_patience_ends_and_reports_the_validation_tree(rng, capsys):
    from evogp_amd.algorithm import DefaultCrossover, DefaultMutation, DefaultSelection, GeneticProgramming
    from evogp_amd.pipeline import StandardPipeline

    X, y = _data(rng)
    d = GenerateDescriptor(max_tree_len=32, input_len=V, output_len=C, using_funcs=["+", "-", "*", "/"], max_layer_cnt=4, const_samples=[-1, 0, 1])
    algo = GeneticProgramming(Forest.random_generate(40, d, keys=torch.tensor([1, 2])), DefaultCrossover(), DefaultMutation(0.2, d), DefaultSelection(0.3, 2))
    prob = Classification(X, y, metric="cross_entropy", validation_mask=_mask(rng))
    pipe = StandardPipeline(algo, prob, is_show_details=False, generation_limit=50, validation_patience=2)
    start = algo.forest
    held = prob.validation_scores(start)
    host = pipe.step()
    top = float(held.max())
    assert float(pipe.best_validation_fitness) == top and np.isfinite(top)
    assert torch.equal(pipe.best_validation_tree.node_value, start[int(torch.nonzero(held == top)[0])].node_value)
    assert float(pipe.best_fitness) == float(host.max())
    # a validation fitness that cannot be beaten: the run ends after exactly two generations and returns the tracked tree
    pipe.best_validation_fitness = torch.tensor(float("inf"))
    steps = []
    step = pipe.step
    pipe.step = lambda: steps.append(1) or step()
    pipe.validation_stale = 0
    assert pipe.run() is pipe.best_validation_tree and len(steps) == 2
    assert "validation" in capsys.readouterr().out


def test_c_abi_argument_errors():
    L = _lib.lib
    none = [None] * 6
    call = lambda pop, D_, gp, var, out, G, ptrs=none, outs=(None, None, None): L.evogp_hip_batch_class_stats(  # noqa: E731
        pop, D_, gp, var, out, *ptrs, G, *outs, None)
    assert call(4, 8, 32, 3, 1, 1) == -1 and call(4, 8, 32, 3, 2, 0) == -1 and call(4, 8, 32, 3, 2, 9) == -1      # BADARG
    assert call(0, 8, 32, 3, 2, 1) == -1 and call(4, 0, 32, 3, 2, 1) == -1 and call(4, 8, 1025, 3, 2, 1) == -1
    assert call(4, 8, 32, 3, 2, 1) == -2                                                                             # NULLPTR
    assert L.evogp_hip_abi_version() == _lib.ABI_VERSION
