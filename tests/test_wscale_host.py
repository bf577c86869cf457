"""CPU: the host logic of weighted linear scaling (Forest.SR_weighted_scaled_fitness, SymbolicRegression(linear_scaling=True,
scaling_loss="problem", sample_weights=, validation_mask=), StandardPipeline's scaled best trees) with the numpy restatement registered as
a test-only CPU kernel (tests/cpu_wscale_ops.py), and the argument checks of the new C entry point, which return before any launch."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cpu_dedup_ops  # noqa: E402
import cpu_derivative_ops  # noqa: E402
import cpu_grad_ops  # noqa: E402
import cpu_interval_ops  # noqa: E402
import cpu_ops  # noqa: E402
import cpu_scale_ops  # noqa: E402
import cpu_structure_ops  # noqa: E402
import cpu_wgrad_ops  # noqa: E402
import cpu_wloss_ops  # noqa: E402
import cpu_wscale_ops  # noqa: E402
import linear_scaling_ref as LS  # noqa: E402
import weighted_scaling_ref as WS  # noqa: E402
from grad_trees import ALL_FUNCS, ARITH, random_forest  # noqa: E402

for _m in (cpu_ops, cpu_grad_ops, cpu_dedup_ops, cpu_scale_ops, cpu_structure_ops, cpu_interval_ops, cpu_derivative_ops, cpu_wloss_ops,
           cpu_wgrad_ops, cpu_wscale_ops):
    _m.register()

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
    m[0], m[1], m[2], m[3] = True, False, False, True
    return m


def _scrub(loss):
    return torch.where(torch.isnan(loss), torch.full_like(loss, float("-inf")), -loss)


def _predictions(forest, X):
    return cpu_scale_ops.predictions(*(a.numpy() for a in forest._tensors()), X.numpy())


OWN = dict(linear_scaling=True, scaling_loss="problem")


def test_forest_method_checks_shapes_and_dedup(rng):
    forest = _forest(rng, 40, ALL_FUNCS)
    forest.batch_subtree_size[3, 0] = 0   # malformed
    X, y = _data(rng)
    W = torch.from_numpy(rng.uniform(0.5, 2, (3, D)).astype(np.float32))
    P = _predictions(forest, X)
    n0 = cpu_wscale_ops.calls["weighted_scaling"]
    loss, slope, icpt = forest.SR_weighted_scaled_fitness(X, y)
    assert loss.shape == slope.shape == icpt.shape == (40,) and loss.dtype == slope.dtype == icpt.dtype == torch.float32
    assert cpu_wscale_ops.last["weights"] is None and cpu_wscale_ops.calls["weighted_scaling"] == n0 + 1
    one = forest.SR_weighted_scaled_fitness(X, y, W[0])
    assert one[0].shape == (40,) and cpu_wscale_ops.last["weights"].shape == (1, D)
    many = forest.SR_weighted_scaled_fitness(X, y, W.to(torch.float64))
    assert many[0].shape == (40, 3) and many[1].shape == many[2].shape == (40,) and cpu_wscale_ops.last["weights"].dtype == torch.float32
    assert forest.SR_weighted_scaled_fitness(X, y, W[:1])[0].shape == (40, 1)
    # (the CPU stand-in IS the restatement: this checks the plumbing -- argument order, the (intercept, slope) columns -- the arithmetic
    # is tests/test_gpu_weighted_scaling.py's)
    ref = WS.scaling(P, y.numpy(), W.numpy())
    WS.check_against(ref, many[0].numpy(), many[2].numpy(), many[1].numpy(), D, what="CPU op (plumbing)")
    assert np.isnan(many[0][3].numpy()).all() and np.isnan(float(many[1][3])) and np.isfinite(many[0].numpy()).all(1).sum() > 20
    twice = forest + forest[:10]
    h0 = cpu_dedup_ops.calls["tree_classes"]
    a, b = twice.SR_weighted_scaled_fitness(X, y, W), twice.SR_weighted_scaled_fitness(X, y, W, dedup=True)
    assert cpu_dedup_ops.calls["tree_classes"] == h0 + 1 and a[0].shape == (50, 3)
    for u, v in zip(a, b):
        assert np.array_equal(_bits(u), _bits(v)) and np.array_equal(_bits(u[40:]), _bits(u[:10]))
    # names, shapes and dtypes on the host
    for kw in (dict(weights=torch.ones(D + 1)), dict(weights=torch.ones(9, D)), dict(weights=torch.ones(0, D)),
               dict(weights=torch.ones(1, 1, D)), dict(weights=torch.ones(D, dtype=torch.int32))):
        with pytest.raises(ValueError):
            forest.SR_weighted_scaled_fitness(X, y, **kw)
    with pytest.raises(ValueError):
        forest.SR_weighted_scaled_fitness(X, y[:, 0])
    with pytest.raises(ValueError):
        forest.SR_weighted_scaled_fitness(X[:, :1], y)
    multi = Forest(2, 3, *(torch.from_numpy(a) for a in random_forest(rng, 4, 32, ALL_FUNCS, 2, 3, max_depth=3)))
    with pytest.raises(ValueError):
        multi.SR_weighted_scaled_fitness(X, torch.zeros(D, 3))


def test_value_errors_and_combinations(rng):
    X, y = _data(rng)
    m, w = _mask(rng), torch.ones(D)
    # scaling_loss=None: every ValueError of before stays
    for opt in (dict(loss="mse"), dict(sample_weights=w), dict(validation_mask=m)):
        with pytest.raises(ValueError):
            SymbolicRegression(datapoints=X, labels=y, linear_scaling=True, **opt)
        prob = SymbolicRegression(datapoints=X, labels=y, **OWN, **opt)
        assert prob.scaling_loss == "problem" and prob.linear_scaling
    SymbolicRegression(datapoints=X, labels=y, **OWN, loss="mse", sample_weights=w, validation_mask=m, dedup=True)
    SymbolicRegression(datapoints=X, labels=y, **OWN, validation_mask=m, const_opt_steps=1, const_opt_loss="problem")
    SymbolicRegression(datapoints=X, labels=y, **OWN, validation_mask=m, const_opt_steps=1, const_opt_loss="problem", const_opt_method="lm")
    SymbolicRegression(datapoints=X, labels=y, **OWN, validation_mask=m, monotonic={0: 1}, max_depth=4)
    for bad in (dict(loss="mae"), dict(loss="huber", loss_param=1.0), dict(loss="pinball", loss_param=0.5), dict(loss="logcosh")):
        with pytest.raises(ValueError):
            SymbolicRegression(datapoints=X, labels=y, **OWN, validation_mask=m, **bad)
    with pytest.raises(ValueError):
        SymbolicRegression(datapoints=X, labels=y, scaling_loss="problem", validation_mask=m)            # without linear_scaling
    with pytest.raises(ValueError):
        SymbolicRegression(datapoints=X, labels=y, scaling_loss="problem")
    with pytest.raises(ValueError):
        SymbolicRegression(datapoints=X, labels=y, linear_scaling=True, scaling_loss="mse")              # an unknown name
    with pytest.raises(ValueError):
        SymbolicRegression(datapoints=X, labels=y, **OWN, validation_mask=m, const_opt_steps=1)          # tuning the unweighted MSE
    with pytest.raises(ValueError):
        SymbolicRegression(datapoints=X, labels=y, **OWN, validation_mask=m, simplify_every=1)
    with pytest.raises(ValueError):
        SymbolicRegression(datapoints=X, labels=torch.cat([y, y], dim=1), **OWN, validation_mask=m)
    with pytest.raises(ValueError):
        SymbolicRegression(datapoints=X, labels=y, **OWN, sample_weights=-w)
    forest = _forest(rng, 4)
    prob = SymbolicRegression(datapoints=X, labels=y, **OWN, validation_mask=m)
    for call in (prob.evaluate, prob.scores):
        with pytest.raises(ValueError):
            call(forest, use_MSE=False)
    # no loss option at all: plain linear scaling, the new op is not called
    n0, s0 = cpu_wscale_ops.calls["weighted_scaling"], cpu_scale_ops.calls["linear_scaling"]
    plain = SymbolicRegression(datapoints=X, labels=y, **OWN)
    assert np.array_equal(_bits(plain.evaluate(forest)), _bits(SymbolicRegression(datapoints=X, labels=y, linear_scaling=True).evaluate(forest)))
    assert cpu_wscale_ops.calls["weighted_scaling"] == n0 and cpu_scale_ops.calls["linear_scaling"] == s0 + 2
    with pytest.raises(ValueError):
        plain.validation_scores(forest)


def test_scores_are_column_0_and_validation_scores_column_1(rng):
    forest = _forest(rng, 40, ALL_FUNCS)
    forest.batch_subtree_size[5, 0] = 0   # malformed
    X, y = _data(rng)
    m = _mask(rng)
    w = torch.from_numpy(rng.uniform(0.1, 2, D).astype(np.float32))
    for opts in (dict(), dict(sample_weights=w), dict(loss="mse", sample_weights=w, dedup=True)):
        prob = SymbolicRegression(datapoints=X, labels=y, validation_mask=m, **OWN, **opts)
        ws = opts.get("sample_weights", torch.ones(D))
        rows = torch.stack([ws * (~m), ws * m])
        loss, slope, icpt = forest.SR_weighted_scaled_fitness(X, y, rows)
        n0 = cpu_wscale_ops.calls["weighted_scaling"]
        sc = prob.scores(forest)
        assert cpu_wscale_ops.calls["weighted_scaling"] == n0 + 1, "ONE call of the op per scores"
        assert torch.equal(cpu_wscale_ops.last["weights"], rows)
        assert np.array_equal(_bits(sc), _bits(_scrub(loss[:, 0])))
        assert np.array_equal(_bits(prob.last_validation_loss), _bits(loss[:, 1]))
        vs = prob.validation_scores(forest, sc)
        assert cpu_wscale_ops.calls["weighted_scaling"] == n0 + 1, "the validation column of the pass behind the scores"
        assert np.array_equal(_bits(vs), _bits(torch.where(torch.isnan(loss[:, 0]), float("-inf"), _scrub(loss[:, 1]))))
        assert np.array_equal(_bits(prob.validation_scores(forest)), _bits(vs))
        assert np.array_equal(_bits(prob.evaluate(forest)), _bits(-loss[:, 0]))
        l2, s2, i2 = prob.scaled_fitness(forest)
        assert np.array_equal(_bits(l2), _bits(loss[:, 0])) and np.array_equal(_bits(s2), _bits(slope)) and np.array_equal(_bits(i2), _bits(icpt))
        # the held-out error belongs to the model fitted WITHOUT the held-out rows: the training-only fit gives the same coefficients
        lt, st, it = forest.SR_weighted_scaled_fitness(X, y, rows[0])
        assert np.array_equal(_bits(st), _bits(slope)) and np.array_equal(_bits(it), _bits(icpt)) and np.array_equal(_bits(lt), _bits(loss[:, 0]))
        assert torch.isnan(sc[5]) or sc[5] == float("-inf")
        assert np.isfinite(loss.numpy()).all(1).sum() > 20
        # scaled: the training row's coefficients written in, last_validation_loss untouched
        keep = prob.last_validation_loss
        wrapped = prob.scaled(forest)
        assert prob.last_validation_loss is keep
        for a, b in zip(wrapped._tensors(), forest.apply_scaling(slope, icpt, grow=True)[0]._tensors()):
            assert torch.equal(a, b)
    # one weight row, no mask: (pop,), no validation column
    prob = SymbolicRegression(datapoints=X, labels=y, sample_weights=w, **OWN)
    loss, slope, icpt = forest.SR_weighted_scaled_fitness(X, y, w)
    assert np.array_equal(_bits(prob.evaluate(forest)), _bits(-loss)) and prob.last_validation_loss is None
    assert cpu_wscale_ops.last["weights"].shape == (1, D)
    prob = SymbolicRegression(datapoints=X, labels=y, loss="mse", **OWN)
    assert np.array_equal(_bits(prob.evaluate(forest)), _bits(-forest.SR_weighted_scaled_fitness(X, y)[0]))
    assert cpu_wscale_ops.last["weights"] is None


def test_torch_mode_is_the_same_definition(rng):
    forest = _forest(rng, 40, ALL_FUNCS)   # (well-formed trees: the CPU oracle behind batch_forward has no NaN row for a malformed one)
    X, y = _data(rng)
    m = _mask(rng)
    w = torch.from_numpy(rng.uniform(0.5, 2, D).astype(np.float32))
    w[5] = 0
    P = _predictions(forest, X)
    n0 = cpu_wscale_ops.calls["weighted_scaling"]
    for opts, rows in ((dict(sample_weights=w, validation_mask=m), torch.stack([w * (~m), w * m])), (dict(sample_weights=w), w[None]),
                       (dict(loss="mse"), None)):
        twin = SymbolicRegression(datapoints=X, labels=y, execute_mode="torch", **OWN, **opts)
        loss, slope, icpt = twin.scaled_fitness(forest)
        ref = WS.scaling(P, y.numpy(), None if rows is None else rows.numpy())
        got = loss.numpy()[:, None] if rows is None or rows.shape[0] == 1 else np.stack([loss.numpy(), twin.last_validation_loss.numpy()], 1)
        assert WS.check_against(ref, got, icpt.numpy(), slope.numpy(), D, what=f"torch mode {sorted(opts)}") <= 0.10
        assert np.array_equal(_bits(twin.evaluate(forest)), _bits(-loss)) and np.array_equal(_bits(twin.scores(forest)), _bits(_scrub(loss)))
        prob = SymbolicRegression(datapoints=X, labels=y, **OWN, **opts)
        n1 = cpu_wscale_ops.calls["weighted_scaling"]
        dl, ds, di = prob.scaled_fitness(forest)
        assert cpu_wscale_ops.calls["weighted_scaling"] == n1 + 1
        dgot = dl.numpy()[:, None] if rows is None or rows.shape[0] == 1 else np.stack([dl.numpy(), prob.last_validation_loss.numpy()], 1)
        assert WS.check_against(ref, dgot, di.numpy(), ds.numpy(), D, what=f"op path {sorted(opts)}") <= 0.10
        n0 += 1
    assert cpu_wscale_ops.calls["weighted_scaling"] == n0, "torch mode calls no kernel of the new file"
    # a division by zero on a held-out row: the torch twin follows the rule too
    Xz = X.clone()
    value, type_, size = (np.zeros((2, 32), d) for d in (np.float32, np.int16, np.int16))
    for t in range(2):   # 1 / (x0 - c), c the x0 of row 0 (held out) or of row 1 (a training row)
        for i, (v, ty, s) in enumerate([(4, 3, 5), (1.0, 1, 1), (2, 3, 3), (0, 0, 1), (float(Xz[t, 0]), 1, 1)]):
            value[t, i], type_[t, i], size[t, i] = v, ty, s
    div = Forest(2, 1, *(torch.from_numpy(a) for a in (value, type_, size)))
    twin = SymbolicRegression(datapoints=Xz, labels=y, execute_mode="torch", validation_mask=m, **OWN)
    loss, slope, icpt = twin.scaled_fitness(div)
    assert torch.isfinite(loss[0]) and torch.isfinite(slope[0]) and torch.isnan(twin.last_validation_loss[0])
    assert torch.isnan(loss[1]) and torch.isnan(slope[1]) and torch.isnan(icpt[1]) and torch.isnan(twin.last_validation_loss[1])


def test_masks_penalties_and_the_sign_check_work_on_top(rng):
    forest = _forest(rng, 40, ARITH)
    X, y = _data(rng)
    m = _mask(rng)
    base = SymbolicRegression(datapoints=X, labels=y, validation_mask=m, **OWN)
    loss, slope, _ = base.scaled_fitness(forest)
    # a structural limit sends trees to -inf on both sides; a penalty lowers the training score only
    hard = SymbolicRegression(datapoints=X, labels=y, validation_mask=m, max_depth=3, **OWN)
    out = ~hard.structure_mask(forest)
    assert out.any() and (~out).any()
    train, held = hard.scores(forest), hard.validation_scores(forest)
    assert bool((train[out] == float("-inf")).all()) and bool((held[out] == float("-inf")).all())
    assert np.array_equal(_bits(train[~out]), _bits(base.scores(forest)[~out]))
    soft = SymbolicRegression(datapoints=X, labels=y, validation_mask=m, max_depth=3, structure_penalty=0.5, **OWN)
    viol = soft.structure(forest)[5]
    want = torch.where(viol > 0, base.scores(forest) - 0.5 * viol.to(torch.float32), base.scores(forest))
    assert np.array_equal(_bits(soft.scores(forest)), _bits(want))
    # the sign check: under a +1 constraint a negative slope fails
    up = SymbolicRegression(datapoints=X, labels=y, validation_mask=m, monotonic={0: 1}, input_bounds=(0.0, 2.0), **OWN)
    l_up, s_up, _ = up.scaled_fitness(forest)
    assert np.array_equal(_bits(s_up), _bits(slope))
    neg = slope < 0
    assert neg.any() and bool(torch.isnan(l_up[neg]).all()) and np.array_equal(_bits(l_up[~neg]), _bits(loss[~neg]))
    assert bool((up.scores(forest)[neg] == float("-inf")).all())
    # const_opt_loss="problem" tunes on the training row and the scaled fitness of the tuned forest is what is scored
    tune = SymbolicRegression(datapoints=X, labels=y, validation_mask=m, const_opt_steps=1, const_opt_loss="problem", **OWN)
    n0 = cpu_wgrad_ops.calls["weighted_gradient"]
    tuned = tune.optimize(forest)
    assert tuned.pop_size == forest.pop_size and cpu_wgrad_ops.calls["weighted_gradient"] > n0
    assert np.array_equal(_bits(tune.scores(tuned)), _bits(base.scores(tuned)))


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


def test_pipeline_reports_scaled_best_trees_that_reproduce_the_stated_losses(rng):
    X, y = _data(rng)
    m = _mask(rng)
    w = torch.from_numpy(rng.uniform(0.5, 2, D).astype(np.float32))
    algo, pipe = _pipeline(rng, X, y, validation_mask=m, sample_weights=w, **OWN)
    start = algo.forest
    rows = torch.stack([w * (~m), w * m])
    loss, slope, icpt = start.SR_weighted_scaled_fitness(X, y, rows)
    n0 = cpu_wscale_ops.calls["weighted_scaling"]
    host = pipe.step()
    # one pass for the population, one one-tree pass for each of the two reported trees
    assert cpu_wscale_ops.calls["weighted_scaling"] == n0 + 3
    assert np.array_equal(_bits(host), _bits(_scrub(loss[:, 0])))
    best = int(torch.argmax(host))
    held = torch.where(host == float("-inf"), float("-inf"), _scrub(loss[:, 1]))
    first = int(torch.nonzero(held == held.max())[0])
    assert float(pipe.best_fitness) == float(host[best]) and float(pipe.best_validation_fitness) == float(held.max())
    P = _predictions(start, X)
    for tree, i, col in ((pipe.best_tree, best, 0), (pipe.best_validation_tree, first, 1)):
        wrapped = start[i:i + 1].apply_scaling(slope[i:i + 1], icpt[i:i + 1], grow=True)[0][0]
        assert tree.node_value.shape == (36,) and torch.equal(tree.node_value, wrapped.node_value)
        assert torch.equal(tree.subtree_size, wrapped.subtree_size) and torch.equal(tree.node_type, wrapped.node_type)
        # the reported tree IS the model: its plain weighted MSE on the column's rows is the stated loss, up to the float32 evaluation
        # of b p + a inside the tree (linear_scaling_ref.refit_bound) and the float32 rounding of the two losses
        one = Forest(2, 1, *(x[None].contiguous() for x in (tree.node_value, tree.node_type, tree.subtree_size)))
        mse = float(one.SR_weighted_loss(X, y, rows[col], "mse")[0])
        stated = float(loss[i, col])
        bound = LS.refit_bound(P[i:i + 1], icpt[i:i + 1].numpy(), slope[i:i + 1].numpy(), np.array([stated]))[0] + 2e-6 * abs(stated)
        assert abs(mse - stated) <= bound, (col, mse, stated, bound)
    # validation_patience returns the scaled validation tree
    algo, pipe = _pipeline(rng, X, y, validation_mask=m, validation_patience=1, generation_limit=4, **OWN)
    out = pipe.run()
    assert out is pipe.best_validation_tree and out.node_value.shape == (36,)
    # without linear scaling the validation tree stays as it stands in the forest
    algo, pipe = _pipeline(rng, X, y, validation_mask=m)
    start = algo.forest
    pipe.step()
    assert pipe.best_validation_tree.node_value.shape == (32,)


def test_argument_errors_without_gpu():
    from evogp_amd import _lib

    L = _lib.lib
    p, q = 8, 16  # (never dereferenced: the host checks come first)

    def call(pop=4, D=8, gp_len=32, var_len=3, out_len=1, value=p, X=p, y=p, weights=p, n_weights=2, loss=q, coef=q):
        return L.evogp_hip_sr_weighted_scaling(pop, D, gp_len, var_len, out_len, value, p, p, X, y, weights, n_weights, loss, coef, None)

    for kw in (dict(pop=0), dict(D=0), dict(gp_len=0), dict(gp_len=1025), dict(var_len=0), dict(out_len=0)):
        assert call(**kw) == -1, kw
    for kw in (dict(n_weights=0), dict(n_weights=9), dict(weights=None, n_weights=2), dict(weights=None, n_weights=0)):
        assert call(**kw) == -1, kw
    assert call(out_len=2) == -3                                   # multi-output: unsupported
    assert call(out_len=2, n_weights=9) == -1                      # (the argument checks come first)
    for kw in (dict(value=None), dict(X=None), dict(y=None), dict(loss=None), dict(coef=None), dict(weights=None, n_weights=1, coef=None)):
        assert call(**kw) == -2, kw
    assert L.evogp_hip_abi_version() == _lib.ABI_VERSION
