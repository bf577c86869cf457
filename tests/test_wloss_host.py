"""CPU: the host logic of the weighted losses (Forest.SR_weighted_loss, SymbolicRegression(loss=, loss_param=, sample_weights=,
validation_mask=), StandardPipeline's validation tracking) with the numpy restatement registered as a test-only CPU kernel
(tests/cpu_wloss_ops.py), and the argument checks of the new C entry point, which return before any launch."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cpu_dedup_ops  # noqa: E402
import cpu_grad_ops  # noqa: E402
import cpu_ops  # noqa: E402
import cpu_scale_ops  # noqa: E402
import cpu_structure_ops  # noqa: E402
import cpu_wloss_ops  # noqa: E402
import weighted_loss_ref as WL  # noqa: E402
from grad_trees import ALL_FUNCS, ARITH, random_forest  # noqa: E402

cpu_ops.register()
cpu_grad_ops.register()
cpu_dedup_ops.register()
cpu_scale_ops.register()
cpu_structure_ops.register()
cpu_wloss_ops.register()

from evogp_amd.problem import SymbolicRegression  # noqa: E402
from evogp_amd.tree import Forest, GenerateDescriptor, set_default_device  # noqa: E402
from evogp_amd.tree import utils as _tree_utils  # noqa: E402

D = 40


@pytest.fixture(autouse=True)
def _cpu_default_device():
    saved = _tree_utils._DEVICE
    set_default_device("cpu")
    yield
    _tree_utils._DEVICE = saved


def _data(rng, var_len=2):
    X = rng.uniform(0.5, 1.5, (D, var_len)).astype(np.float32)
    y = (2.0 * X[:, :1] * X[:, 1:2] - 0.5).astype(np.float32)
    return torch.from_numpy(X), torch.from_numpy(y)


def _forest(rng, pop=30, funcs=ARITH):
    value, type_, size = random_forest(rng, pop, 32, funcs, 2, 1, max_depth=4)
    return Forest(2, 1, *(torch.from_numpy(a) for a in (value, type_, size)))


def _bits(t):
    return t.contiguous().numpy().view(np.uint32)


def _mask(rng):
    m = torch.from_numpy(rng.random(D) < 0.3)
    m[0], m[1] = True, False
    return m


def _scrub(loss):
    return torch.where(torch.isnan(loss), torch.full_like(loss, float("-inf")), -loss)


def test_default_problem_calls_none_of_the_new_ops(rng):
    forest = _forest(rng)
    X, y = _data(rng)
    before = dict(cpu_wloss_ops.calls)
    prob = SymbolicRegression(datapoints=X, labels=y)
    assert prob.loss is None and prob.sample_weights is None and prob.validation_mask is None and prob.last_validation_loss is None
    fit = forest.SR_fitness(X, y)
    assert np.array_equal(_bits(prob.evaluate(forest)), _bits(-fit))
    assert np.array_equal(_bits(prob.scores(forest)), _bits(_scrub(fit)))
    mae = forest.SR_fitness(X, y, False)
    assert np.array_equal(_bits(prob.evaluate(forest, use_MSE=False)), _bits(-mae))
    assert cpu_wloss_ops.calls == before
    with pytest.raises(ValueError):
        prob.validation_scores(forest)


def test_value_errors(rng):
    X, y = _data(rng)
    m, w = _mask(rng), torch.ones(D)
    new = [dict(loss="mae"), dict(loss="huber", loss_param=1.0), dict(sample_weights=w), dict(validation_mask=m)]
    for opt in new:
        SymbolicRegression(datapoints=X, labels=y, **opt)
        for other in (dict(linear_scaling=True), dict(const_opt_steps=2), dict(simplify_every=1)):
            with pytest.raises(ValueError):
                SymbolicRegression(datapoints=X, labels=y, **opt, **other)
        with pytest.raises(ValueError):
            SymbolicRegression(datapoints=X, labels=torch.cat([y, y], dim=1), **opt)   # labels that are not (D, 1)
        with pytest.raises(ValueError):
            SymbolicRegression(datapoints=X, labels=y[:, 0], **opt)
    X3 = torch.cat([X, X[:, :1]], dim=1)
    with pytest.raises(ValueError):
        SymbolicRegression(datapoints=X3, labels=y, multigene=True, loss="mae")
    # loss names and parameters
    for bad in (dict(loss="cauchy"), dict(loss="huber"), dict(loss="huber", loss_param=0.0), dict(loss="huber", loss_param=float("inf")),
                dict(loss="huber", loss_param=float("nan")), dict(loss="pinball", loss_param=1.0), dict(loss="pinball", loss_param=0.0),
                dict(loss="pinball"), dict(loss="mse", loss_param=1.0), dict(loss_param=1.0), dict(loss="huber", loss_param="1")):
        with pytest.raises(ValueError):
            SymbolicRegression(datapoints=X, labels=y, **bad)
    # weights: shape, dtype, values (checked once, here)
    for bad in (torch.ones(D + 1), torch.ones(D, 1), torch.ones(D, dtype=torch.int64), [1.0] * D, -w, w * float("nan"),
                torch.zeros(D), torch.cat([w[:-1], torch.tensor([float("inf")])])):
        with pytest.raises(ValueError):
            SymbolicRegression(datapoints=X, labels=y, sample_weights=bad)
    # mask: a (D,) bool tensor that is neither all-true nor all-false
    for bad in (m.to(torch.float32), m[:-1], m[:, None], torch.ones(D, dtype=torch.bool), torch.zeros(D, dtype=torch.bool), m.tolist()):
        with pytest.raises(ValueError):
            SymbolicRegression(datapoints=X, labels=y, validation_mask=bad)
    forest = _forest(rng, 4)
    prob = SymbolicRegression(datapoints=X, labels=y, loss="huber", loss_param=1.0)
    for call in (prob.evaluate, prob.scores):
        with pytest.raises(ValueError):
            call(forest, use_MSE=False)
    # Forest.SR_weighted_loss: names, shapes and dtypes on the host
    for kw in (dict(loss="cauchy"), dict(loss="huber"), dict(loss="pinball", param=1.5), dict(loss="mae", param=1.0),
               dict(weights=torch.ones(D + 1)), dict(weights=torch.ones(9, D)), dict(weights=torch.ones(0, D)),
               dict(weights=torch.ones(1, 1, D)), dict(weights=torch.ones(D, dtype=torch.int32))):
        with pytest.raises(ValueError):
            forest.SR_weighted_loss(X, y, **kw)
    with pytest.raises(ValueError):
        forest.SR_weighted_loss(X, y[:, 0])
    with pytest.raises(ValueError):
        forest.SR_weighted_loss(X[:, :1], y)
    multi = Forest(2, 3, *(torch.from_numpy(a) for a in random_forest(rng, 4, 32, ALL_FUNCS, 2, 3, max_depth=3)))
    with pytest.raises(ValueError):
        multi.SR_weighted_loss(X, torch.zeros(D, 3))


def test_forest_method_shapes_and_dedup(rng):
    forest = _forest(rng, 40, ALL_FUNCS)
    forest.batch_subtree_size[3, 0] = 0   # malformed
    X, y = _data(rng)
    W = torch.from_numpy(rng.uniform(0, 2, (3, D)).astype(np.float32))
    P = cpu_scale_ops.predictions(*(a.numpy() for a in forest._tensors()), X.numpy())
    n0 = cpu_wloss_ops.calls["weighted_loss"]
    plain = forest.SR_weighted_loss(X, y)
    assert plain.shape == (40,) and plain.dtype == torch.float32 and cpu_wloss_ops.last["weights"] is None
    assert cpu_wloss_ops.last["kind"] == "mse" and cpu_wloss_ops.calls["weighted_loss"] == n0 + 1
    one = forest.SR_weighted_loss(X, y, W[0], "huber", 0.75)
    assert one.shape == (40,) and cpu_wloss_ops.last["weights"].shape == (1, D) and cpu_wloss_ops.last["param"] == 0.75
    many = forest.SR_weighted_loss(X, y, W.to(torch.float64), "pinball", 0.25)
    assert many.shape == (40, 3) and cpu_wloss_ops.last["weights"].dtype == torch.float32
    assert forest.SR_weighted_loss(X, y, W[:1], "logcosh").shape == (40, 1)
    # (the CPU stand-in IS the restatement: this checks the plumbing, the arithmetic is tests/test_gpu_weighted_loss.py's)
    assert np.array_equal(_bits(many), WL.weighted_loss(P, y.numpy(), W.numpy(), "pinball", 0.25).view(np.uint32))
    assert np.isnan(many[3].numpy()).all() and np.isnan(float(plain[3])) and np.isfinite(many.numpy()).all(1).sum() > 20
    twice = forest + forest[:10]
    h0 = cpu_dedup_ops.calls["tree_classes"]
    a, b = twice.SR_weighted_loss(X, y, W, "huber", 0.5), twice.SR_weighted_loss(X, y, W, "huber", 0.5, dedup=True)
    assert cpu_dedup_ops.calls["tree_classes"] == h0 + 1
    assert a.shape == b.shape == (50, 3) and np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a[40:]), _bits(a[:10]))


def test_mask_columns_equal_two_single_row_calls(rng):
    forest = _forest(rng, 40, ALL_FUNCS)
    X, y = _data(rng)
    m = _mask(rng)
    w = torch.from_numpy(rng.uniform(0.1, 2, D).astype(np.float32))
    for opts, kind, prm in ((dict(), "mse", None), (dict(loss="huber", loss_param=0.5), "huber", 0.5),
                            (dict(loss="pinball", loss_param=0.8, sample_weights=w), "pinball", 0.8)):
        prob = SymbolicRegression(datapoints=X, labels=y, validation_mask=m, **opts)
        ws = opts.get("sample_weights", torch.ones(D))
        n0 = cpu_wloss_ops.calls["weighted_loss"]
        ev = prob.evaluate(forest)
        assert cpu_wloss_ops.calls["weighted_loss"] == n0 + 1, "ONE call with two weight rows"
        assert torch.equal(cpu_wloss_ops.last["weights"], torch.stack([ws * (~m), ws * m]))
        train = forest.SR_weighted_loss(X, y, ws * (~m), kind, prm)
        held = forest.SR_weighted_loss(X, y, ws * m, kind, prm)
        assert np.array_equal(_bits(ev), _bits(-train)) and np.array_equal(_bits(prob.last_validation_loss), _bits(held))
        assert np.array_equal(_bits(prob.scores(forest)), _bits(_scrub(train)))
        assert np.array_equal(_bits(prob.validation_scores(forest)), _bits(torch.where(torch.isnan(train), float("-inf"), _scrub(held))))
    # without a mask: one weight row, (pop,); loss=None follows use_MSE
    prob = SymbolicRegression(datapoints=X, labels=y, sample_weights=w)
    assert np.array_equal(_bits(prob.evaluate(forest)), _bits(-forest.SR_weighted_loss(X, y, w)))
    assert np.array_equal(_bits(prob.evaluate(forest, use_MSE=False)), _bits(-forest.SR_weighted_loss(X, y, w, "mae")))
    assert prob.last_validation_loss is None
    prob = SymbolicRegression(datapoints=X, labels=y, loss="logcosh", dedup=True)
    h0 = cpu_dedup_ops.calls["tree_classes"]
    assert np.array_equal(_bits(prob.evaluate(forest)), _bits(-forest.SR_weighted_loss(X, y, None, "logcosh")))
    assert cpu_dedup_ops.calls["tree_classes"] == h0 + 1 and cpu_wloss_ops.last["weights"] is None


def test_torch_mode_is_the_same_definition(rng):
    forest = _forest(rng, 40, ALL_FUNCS)   # (well-formed trees: the CPU oracle behind batch_forward has no NaN row for a malformed one)
    X, y = _data(rng)
    m = _mask(rng)
    w = torch.from_numpy(rng.uniform(0, 2, D).astype(np.float32))
    w[5] = 0
    P = cpu_scale_ops.predictions(*(a.numpy() for a in forest._tensors()), X.numpy())
    n0 = cpu_wloss_ops.calls["weighted_loss"]
    for kind, prm in (("mse", None), ("mae", None), ("huber", 1.0), ("pinball", 0.3), ("logcosh", None)):
        prob = SymbolicRegression(datapoints=X, labels=y, loss=kind, loss_param=prm, sample_weights=w, validation_mask=m,
                                  execute_mode="torch")
        ev = prob.evaluate(forest)
        want = WL.weighted_loss(P, y.numpy(), torch.stack([w * (~m), w * m]).numpy(), kind, prm)
        WL.check(-ev.numpy(), want[:, 0], D, kind, what=f"torch mode {kind} training")
        WL.check(prob.last_validation_loss.numpy(), want[:, 1], D, kind, what=f"torch mode {kind} validation")
        alone = SymbolicRegression(datapoints=X, labels=y, loss=kind, loss_param=prm, execute_mode="torch")
        WL.check(-alone.evaluate(forest).numpy(), WL.weighted_loss(P, y.numpy(), None, kind, prm)[:, 0], D, kind)
    assert cpu_wloss_ops.calls["weighted_loss"] == n0, "torch mode calls no kernel of the new file"


def test_validation_scores_are_minus_inf_where_the_training_score_is(rng):
    forest = _forest(rng, 40, ARITH)
    X, y = _data(rng)
    m = _mask(rng)
    # a structural limit sends some trees to -inf on the training side: they are no candidates on the held-out rows either
    prob = SymbolicRegression(datapoints=X, labels=y, validation_mask=m, loss="mae", max_depth=3)
    train, held = prob.scores(forest), prob.validation_scores(forest)
    out = ~prob.structure_mask(forest)
    assert out.any() and (~out).any()
    assert bool((train[out] == float("-inf")).all()) and bool((held[out] == float("-inf")).all())
    raw = forest.SR_weighted_loss(X, y, (m).to(torch.float32), "mae")
    keep = ~out & ~torch.isnan(raw) & (train != float("-inf"))
    assert keep.any() and np.array_equal(_bits(held[keep]), _bits(-raw[keep]))
    assert bool((held[torch.isnan(raw)] == float("-inf")).all())
    # the scores of a pass that has just been made are taken over
    n0 = cpu_wloss_ops.calls["weighted_loss"]
    again = prob.validation_scores(forest, train)
    assert cpu_wloss_ops.calls["weighted_loss"] == n0 and np.array_equal(_bits(again), _bits(held))


def _pipeline(rng, X, y, pop=60, **kw):
    from evogp_amd.algorithm import DefaultCrossover, DefaultMutation, DefaultSelection, GeneticProgramming
    from evogp_amd.pipeline import StandardPipeline

    d = GenerateDescriptor(max_tree_len=32, input_len=2, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=4,
                           const_samples=[-1, 0, 1])
    pipe_kw = {k: kw.pop(k) for k in ("validation_patience", "generation_limit") if k in kw}
    algo = GeneticProgramming(Forest.random_generate(pop, d, keys=torch.tensor([1, 2])), DefaultCrossover(), DefaultMutation(0.2, d),
                              DefaultSelection(0.3, 2))
    return algo, StandardPipeline(algo, SymbolicRegression(datapoints=X, labels=y, **kw), is_show_details=False,
                                  **{"generation_limit": 2, **pipe_kw})


def test_pipeline_tracks_the_best_validation_tree(rng):
    X, y = _data(rng)
    m = _mask(rng)
    algo, pipe = _pipeline(rng, X, y, validation_mask=m, loss="huber", loss_param=1.0)
    start = algo.forest
    # two copies of one tree tie on every row: the smaller index wins
    for a in start._tensors():
        a[50] = a[20]
    both = start.SR_weighted_loss(X, y, torch.stack([(~m).float(), m.float()]), "huber", 1.0)
    n0 = cpu_wloss_ops.calls["weighted_loss"]
    host = pipe.step()
    assert cpu_wloss_ops.calls["weighted_loss"] == n0 + 1, "the validation scores come out of the pass behind the fitness"
    assert np.array_equal(_bits(host), _bits(_scrub(both[:, 0])))
    held = torch.where(host == float("-inf"), float("-inf"), _scrub(both[:, 1]))
    top = float(held.max())
    first = int(torch.nonzero(held == top)[0])
    assert float(pipe.best_validation_fitness) == top and torch.equal(pipe.best_validation_tree.node_value, start[first].node_value)
    assert pipe.validation_stale == 0 and float(pipe.best_fitness) == float(host.max())
    assert torch.equal(pipe.best_tree.node_value, start[int(torch.argmax(host))].node_value), "best_tree keeps its meaning"

    # the tie rule, forced: every tree a copy of one with a finite score
    algo, pipe = _pipeline(rng, X, y, pop=60, validation_mask=m)
    j = int(torch.argmax(pipe.problem.scores(algo.forest)))
    for a in algo.forest._tensors():
        a[:] = a[j].clone()
    tree = algo.forest[0]
    pipe.step()
    assert torch.equal(pipe.best_validation_tree.node_value, tree.node_value)
    held = pipe.problem.validation_scores(Forest(2, 1, *(x[None].contiguous() for x in (tree.node_value, tree.node_type, tree.subtree_size))))
    assert float(held[0]) == float(pipe.best_validation_fitness)


def test_validation_patience_stops_the_run(rng, capsys):
    from evogp_amd.pipeline import StandardPipeline

    X, y = _data(rng)
    m = _mask(rng)
    algo, pipe = _pipeline(rng, X, y, validation_mask=m, validation_patience=2, generation_limit=50)
    # a validation fitness that cannot be beaten: no generation brings a new best, so the run ends after exactly two
    pipe.best_validation_fitness = torch.tensor(float("inf"))
    sentinel = object()
    pipe.best_validation_tree = sentinel
    steps = []
    step = pipe.step
    pipe.step = lambda: steps.append(1) or step()
    assert pipe.run() is sentinel and len(steps) == 2 and pipe.validation_stale == 2
    assert "validation" in capsys.readouterr().out
    # without patience the run goes to its generation limit and returns best_tree
    algo, pipe = _pipeline(rng, X, y, validation_mask=m, generation_limit=3)
    best = pipe.run()
    assert best is pipe.best_tree and pipe.best_validation_tree is not None and np.isfinite(float(pipe.best_validation_fitness))
    # a seeded run with patience returns the tree it tracked
    algo, pipe = _pipeline(rng, X, y, validation_mask=m, validation_patience=1, generation_limit=6)
    out = pipe.run()
    assert out is pipe.best_validation_tree and pipe.validation_stale <= 1
    for bad in (0, -1, True, 1.5):
        with pytest.raises(ValueError):
            StandardPipeline(algo, pipe.problem, validation_patience=bad)
    with pytest.raises(ValueError):
        StandardPipeline(algo, SymbolicRegression(datapoints=X, labels=y), validation_patience=2)


def test_pipeline_without_a_mask_never_touches_the_new_attributes(rng):
    X, y = _data(rng)
    for kw in (dict(), dict(loss="mae"), dict(sample_weights=torch.ones(D))):
        algo, pipe = _pipeline(rng, X, y, **kw)
        n0 = cpu_wloss_ops.calls["weighted_loss"]
        start = algo.forest
        host = pipe.step()
        assert cpu_wloss_ops.calls["weighted_loss"] == n0 + (1 if kw else 0)
        for name in ("best_validation_tree", "best_validation_fitness", "validation_stale"):
            assert not hasattr(pipe, name), name
        assert pipe.validation_patience is None and pipe.problem.last_validation_loss is None
        assert torch.equal(pipe.best_tree.node_value, start[int(torch.argmax(host))].node_value)
    # the default problem's step gives the bits of -SR_fitness, scrubbed
    algo, pipe = _pipeline(rng, X, y)
    fit = algo.forest.SR_fitness(X, y)
    assert np.array_equal(_bits(pipe.step()), _bits(_scrub(fit)))


def test_argument_errors_without_gpu():
    from evogp_amd import _lib

    L = _lib.lib
    p, q = 8, 16  # (never dereferenced: the host checks come first)

    def call(pop=4, D=8, gp_len=32, var_len=3, out_len=1, value=p, X=p, y=p, weights=p, n_weights=2, kind=0, param=0.0, out=q):
        return L.evogp_hip_sr_weighted_loss(pop, D, gp_len, var_len, out_len, value, p, p, X, y, weights, n_weights, kind, param, out, None)

    for kw in (dict(pop=0), dict(D=0), dict(gp_len=0), dict(gp_len=1025), dict(var_len=0), dict(out_len=0)):
        assert call(**kw) == -1, kw
    for kw in (dict(n_weights=0), dict(n_weights=9), dict(weights=None, n_weights=2), dict(weights=None, n_weights=0)):
        assert call(**kw) == -1, kw
    for kw in (dict(kind=-1), dict(kind=5), dict(kind=2, param=0.0), dict(kind=2, param=-1.0), dict(kind=2, param=float("inf")),
               dict(kind=2, param=float("nan")), dict(kind=3, param=0.0), dict(kind=3, param=1.0), dict(kind=3, param=float("nan")),
               dict(kind=0, param=float("nan")), dict(kind=4, param=float("nan"))):
        assert call(**kw) == -1, kw
    assert call(out_len=2) == -3                                   # multi-output: unsupported
    assert call(out_len=2, n_weights=9) == -1                      # (the argument checks come first)
    for kw in (dict(value=None), dict(X=None), dict(y=None), dict(out=None), dict(weights=None, n_weights=1, out=None)):
        assert call(**kw) == -2, kw
    assert L.evogp_hip_abi_version() == _lib.ABI_VERSION
