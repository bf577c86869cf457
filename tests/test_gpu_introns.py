"""GPU: exact semantic intron removal (csrc/sr_introns.hip), bit for bit and without a tolerance.  ``rep`` of sr_intron_kernel against the
numpy restatement (tests/intron_ref.py) fed with the device's own signatures and with values from an independent kernel -- every subtree
extracted into a row of its own and evaluated by the register interpreter (batch_forward) -- on every path of the launch plan (LDS and
global tapes, one to four waves, ragged tiles); the rewrite against the restatement; the rewritten forest's predictions against the
original's on every row, also under garbage signatures; the fixed point; the hand-built plants; determinism on one stream and on two; the
forest invariants and the binding contract of both ops; and five generations of a pipeline that removes introns in front of every
evaluation."""
import os
import sys

import numpy as np
import pytest
import torch

import evogp_amd  # noqa: F401  (registers the ops)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forest_invariance as FI  # noqa: E402
import intron_ref as IR  # noqa: E402
import intron_tables as IT  # noqa: E402
import sr_grad_ref as R  # noqa: E402
import subtree_ref as S  # noqa: E402
from intron_ref import c, iff, op, un, x  # noqa: E402

from evogp_amd.algorithm import DefaultCrossover, DefaultMutation, DefaultSelection, GeneticProgramming  # noqa: E402
from evogp_amd.pipeline import StandardPipeline  # noqa: E402
from evogp_amd.problem import SymbolicRegression  # noqa: E402
from evogp_amd.tree import Forest, GenerateDescriptor  # noqa: E402

pytestmark = pytest.mark.gpu
hip = torch.ops.evogp_hip


def _dev(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _head(forest, X):
    return (forest[0].shape[0], X.shape[0], forest[0].shape[1], X.shape[1], 1)


def signatures(forest, X):
    return hip.tree_SR_subtree_signatures(*_head(forest, X), *_dev(*forest), _dev(X)[0]).cpu().numpy().view(np.uint64)


def introns(forest, X, sig):
    return hip.tree_SR_subtree_introns(*_head(forest, X), *_dev(*forest), _dev(X)[0], _dev(np.ascontiguousarray(sig).view(np.int64))[0]).cpu().numpy()


def remove(forest, rep):
    return tuple(a.cpu().numpy() for a in hip.tree_remove_introns(*_dev(*forest), _dev(rep)[0]))


def forward(forest, X):
    """(pop, D) float32 of the register interpreter"""
    if not forest[0].shape[0]:
        return np.zeros((0, X.shape[0]), np.float32)
    f = Forest(X.shape[1], 1, *_dev(*forest))
    return f.batch_forward(_dev(X)[0])[:, :, 0].contiguous().cpu().numpy()


_truth = {}


def truth_values(name, pop=257):
    """the values of every subtree of the shared forest on its MAX_D rows, once per forest: a data set of D rows is the first D of them"""
    if (name, pop) not in _truth:
        forest, X = IR.shared_forest(name, pop)
        trees = IR.formed_trees(forest[1], forest[2])
        rows, offsets = IR.subtree_rows(*forest, trees)
        _truth[name, pop] = (forward(rows, X), offsets, {t: k for k, t in enumerate(trees)})
    return _truth[name, pop]


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def check_forest(name, D, pop=257, coverage=True):
    """truth, rewrite, end to end, garbage signatures and the fixed point on the first D rows of a shared forest; ``coverage``: also the
    condition on the inputs (a third of the trees shrink, a third do not), which is a statement about data sets of more than one row"""
    forest, X = IR.shared_forest(name, pop)
    X = np.ascontiguousarray(X[:D])
    P, offsets, at = truth_values(name, pop)
    values_of = lambda t: P[offsets[at[t]]:offsets[at[t] + 1], :D]   # noqa: E731
    formed = sorted(at)
    L = forest[0].shape[1]
    sig = signatures(forest, X)
    before = forward(forest, X)
    live = np.arange(L)[None, :] < np.clip(forest[2][:, :1], 0, L)
    for what, s in (("the device's signatures", sig), ("garbage signatures", sig % np.uint64(3) + np.uint64(1))):
        rep = introns(forest, X, s)
        assert rep.dtype == np.int16 and rep.shape == (pop, L)
        want = IR.forest_rep(forest[1], forest[2], s, values_of)
        diff = np.argwhere(rep != want)
        assert not len(diff), (what, len(diff), diff[:4].tolist(), rep[tuple(diff[0])], want[tuple(diff[0])])
        out = remove(forest, rep)
        wout = IR.rewrite(*forest, want)
        for k, (g, w) in enumerate(zip(out, wout)):
            assert g.dtype == w.dtype and np.array_equal(_bits(g), _bits(w)), (what, "output", k, np.argwhere(_bits(g) != _bits(w))[:4].tolist())
        after = forward(out[:3], X)
        assert IR.equal(before[formed], after[formed]).all(), (what, "a prediction changed", np.argwhere(~IR.equal(before[formed], after[formed]))[:4].tolist())
        assert all(S.check_prefix_tree(out[1][t], out[2][t]) for t in formed)
        if what.startswith("the device"):
            rep2 = introns(out[:3], X, signatures(out[:3], X))   # the fixed point
            out2 = remove(out[:3], rep2)
            lost = out[3][formed] > 0
            assert not coverage or (lost.mean() >= 1 / 3 and (~lost).mean() >= 1 / 3), (name, D, lost.mean())
            assert (rep2 == np.arange(L)[None, :]).all() and not out2[3].any(), "removing the introns of the result changes nothing"
            assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(out2[:3], out[:3]))
            assert (rep[~live] == np.broadcast_to(np.arange(L), rep.shape)[~live]).all()
            print(f"{name} D {D}: {out[3].sum()} of {int(np.clip(forest[2][:, 0], 0, L).sum())} nodes removed, {lost.mean():.0%} of the trees shrink")
        else:
            assert out[3].sum() > 0, "one word in three still finds some"


# ---- 1. the kernels against the restatement on every path of the plan ------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 63, 64, 65, 300])
@pytest.mark.parametrize("gp_len", [64, 1024])
@pytest.mark.parametrize("funcs", ["arith", "all"])
def test_rep_rewrite_and_predictions_equal_the_restatement(funcs, gp_len, D):
    # one row (one tile, lanes 1 to 63 repeat row 0): most subtrees are "equal" there, so the coverage condition alone does not apply
    check_forest(f"{funcs}_L{gp_len}", D, coverage=D > 1)


def test_a_population_that_fills_the_chip_takes_one_wave_per_tree():
    pop, D = 4100, 70
    assert pop >= 16 * torch.cuda.get_device_properties(0).multi_processor_count, "the plan gives a tree one wave from 16 trees per compute unit on"
    forest, X = IR.shared_forest("arith_L64", pop)
    X = np.ascontiguousarray(X[:D])
    sig = signatures(forest, X)
    rep = introns(forest, X, sig)
    out = remove(forest, rep)
    formed = IR.formed_trees(forest[1], forest[2])
    assert IR.equal(forward(forest, X)[formed], forward(out[:3], X)[formed]).all()
    pick = np.arange(0, pop, 7)   # the restatement on every seventh tree: a per-tree op
    sub = tuple(a[pick] for a in forest)
    values = IR.values_from(lambda v, t, s: forward((v, t, s), X), *sub)
    want = IR.forest_rep(sub[1], sub[2], sig[pick], values)
    assert np.array_equal(rep[pick], want)
    wout = IR.rewrite(*sub, want)
    assert all(np.array_equal(_bits(g[pick]), _bits(w)) for g, w in zip(out, wout)) and 0.3 < (out[3][formed] > 0).mean() < 0.7


def test_wide_inputs():
    check_forest("all_L64_v40", 65)


# ---- 2. the plants ----------------------------------------------------------------------------------------------------------------------
def test_the_plants_on_the_device():
    rng = np.random.default_rng(7)
    x0 = rng.uniform(0.5, 1.5, 130).astype(np.float32)
    X = np.stack([x0, (x0 + rng.uniform(0.25, 1.0, 130)).astype(np.float32), rng.uniform(-2.0, 2.0, 130).astype(np.float32)], 1)
    X[129, 2] = -0.5   # (the last, ragged tile holds a negative row)
    prod = op(R.F_MUL, x(2), c(0.0))
    nan = op(R.F_DIV, x(1), c(0.0))
    s = op(R.F_ADD, x(0), x(1))
    a = op(R.F_MUL, x(0), x(2))
    trees = [IR.WRAPS[n](a, x(1)) for n in sorted(IR.WRAPS)]
    want = [a] * len(trees)
    trees += [un(R.F_NEG, un(R.F_NEG, un(R.F_NEG, un(R.F_NEG, x(0))))), op(R.F_ADD, x(0), nan), prod, op(R.F_DIV, c(1.0), prod),
              op(R.F_LOOSE_DIV, c(1.0), prod), op(R.F_MIN, iff(x(0), x(1), x(2)), x(0)), op(R.F_MAX, s, s),
              op(R.F_MIN, op(R.F_MUL, s, c(1.0)), s), op(R.F_MUL, x(0), c(0.0))]
    want += [x(0), nan, prod, op(R.F_DIV, c(1.0), prod), op(R.F_LOOSE_DIV, c(1.0), prod), x(0), s, s, c(0.0)]
    forest, wforest = IR.forest(trees, 64), IR.forest(want, 64)
    sig = signatures(forest, X)
    rep = introns(forest, X, sig)
    out = remove(forest, rep)
    for t in range(len(trees)):
        assert all(np.array_equal(_bits(o[t]), _bits(w[t])) for o, w in zip(out[:3], wforest)), (t, out[1][t, :8], out[2][t, :8])
    k = len(IR.WRAPS)
    assert sig[k + 2, 0] == sig[k + 2, 2] and rep[k + 2, 0] == 0, "x2 * 0.0: the signature proposes the constant, the tape refuses (-0.0)"
    assert rep[k + 5, 0] == 2 and rep[k + 5, 1] == 3, "the hierarchy plant: the root names the x0 inside the IF, the IF names x1"
    assert np.array_equal(out[3], [len(a_) - len(b_) for a_, b_ in zip(trees, want)])
    P = forward(out[:3], X)
    assert (P[k + 4][X[:, 2] < 0] == np.float32(-1e9)).all() and (P[k + 4][X[:, 2] > 0] == np.float32(1e9)).all(), "the zero's sign survives"
    assert IR.equal(forward(forest, X), P).all()
    # a collision is refused and no second candidate is tried; split words collapse nothing
    tree = op(R.F_ADD, op(R.F_MUL, x(0), x(1)), op(R.F_ADD, x(2), c(0.0)))
    one = IR.forest([tree], 64)
    true = signatures(one, X)
    lie = true.copy()
    lie[0, 3] = lie[0, 1] = lie[0, 0]
    assert introns(one, X, true)[0, :7].tolist() == [0, 1, 2, 3, 5, 5, 6] and introns(one, X, lie)[0, :7].tolist() == [0, 1, 2, 3, 5, 5, 6]
    assert (introns(one, X, np.arange(1, 65, dtype=np.uint64)[None, :]) == np.arange(64)).all()
    assert (introns(one, X, np.zeros((1, 64), np.uint64)) == np.arange(64)).all(), "a zero word is never a candidate's parent"
    # garbage rep into the rewrite: the restatement's forest
    (value, type_, size), _ = IR.shared_forest("all_L64")
    for kind in range(3):
        g = (rng.integers(-5, 70, value.shape) if kind == 0 else np.arange(64)[None, :] + rng.integers(-1, 4, value.shape) if kind == 1
             else np.full(value.shape, 32767)).astype(np.int16)
        got, wout = remove((value, type_, size), g), IR.rewrite(value, type_, size, g)
        assert all(np.array_equal(_bits(a_), _bits(b_)) for a_, b_ in zip(got, wout)), kind


# ---- 3. determinism -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gp_len", [64, 1024])
def test_two_calls_and_two_streams_give_the_same_bits(gp_len):
    f, X = IR.shared_forest(f"all_L{gp_len}")
    pop, var_len = f[0].shape[0], X.shape[1]
    forest, X = _dev(*f), _dev(X)[0]

    def both():
        sig = hip.tree_SR_subtree_signatures(pop, IR.MAX_D, gp_len, var_len, 1, *forest, X)
        rep = hip.tree_SR_subtree_introns(pop, IR.MAX_D, gp_len, var_len, 1, *forest, X, sig)
        return (rep,) + tuple(hip.tree_remove_introns(*forest, rep))

    first, second = both(), both()
    outs = []
    for _ in range(2):
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            outs.append(both())
        stream.synchronize()
    torch.cuda.synchronize()
    assert int(first[4].sum()) > 100
    for other in (second, outs[0], outs[1]):
        assert all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
                   for a, b in zip(first, other))


# ---- 4. the tables ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op_name", [IT.INTRONS, IT.REWRITE])
@pytest.mark.parametrize("case", FI.cases_for(IT.INTRONS))
def test_ops_keep_the_invariants(case, op_name):
    FI.check(op_name, FI.TABLE[op_name], FI.build_case(case), "cuda")
    torch.cuda.synchronize()


@pytest.mark.parametrize("op_name", sorted(IT.ROWS))
def test_binding_contract(op_name):
    IT.BC.test_valid_call_and_one_fault_at_a_time(op_name)
    row = IT.ROWS[op_name]()
    out = getattr(hip, op_name.split("::")[1])(*[a for _, a in row["args"]])
    if op_name == IT.INTRONS:   # four CONST leaves: nothing below them
        assert out.cpu().tolist() == [list(range(IT.BC.L))] * IT.BC.POP
    else:                       # rep 0 everywhere: no entry names a descendant, the rows come back
        assert all(torch.equal(o, a) for o, (_, a) in zip(out[:3], row["args"][:3])) and out[3].cpu().tolist() == [0] * IT.BC.POP


# ---- 5. end to end -------------------------------------------------------------------------------------------------------------------------
def test_five_generations_with_intron_removal_under_a_pinball_loss_and_a_validation_mask():
    rng = np.random.default_rng(8)
    X = torch.from_numpy(rng.uniform(-2, 2, (128, 3)).astype(np.float32)).cuda()
    y = (X[:, :1] * X[:, 1:2] + X[:, 2:3] / (1.5 + X[:, :1] ** 2)).contiguous()
    mask = torch.from_numpy(rng.random(128) < 0.25).cuda()
    d = GenerateDescriptor(max_tree_len=64, input_len=3, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=5, const_samples=[-1, 0, 1, 2])
    kw = dict(datapoints=X, labels=y, loss="pinball", loss_param=0.3, validation_mask=mask)
    algo = GeneticProgramming(Forest.random_generate(512, d, keys=torch.tensor([1, 2], dtype=torch.uint32, device="cuda")), DefaultCrossover(),
                              DefaultMutation(0.3, d.update(max_layer_cnt=3)), DefaultSelection(0.3, 4))
    problem, plain = SymbolicRegression(intron_removal_every=1, **kw), SymbolicRegression(**kw)
    pipe = StandardPipeline(algo, problem, is_show_details=False, generation_limit=5)
    removed_total = 0
    for gen in range(5):
        handed = Forest(3, 1, *(a.clone() for a in algo.forest._tensors()))
        want, removed = handed.remove_introns(X)
        removed_total += int(removed.sum())
        want_fit, want_val = plain.scores(handed), plain.last_validation_loss.clone()
        fitness = pipe.step()
        assert torch.equal(fitness.view(torch.int32).cpu(), want_fit.view(torch.int32).cpu()), "the fitness of the forest with its introns"
        assert IR.equal(problem.last_validation_loss.cpu().numpy(), want_val.cpu().numpy()).all(), "and its held-out loss"
        scored = plain.scores(want)
        assert torch.equal(scored.view(torch.int32), want_fit.view(torch.int32)), "removal changes no score"
    assert removed_total > 0 and algo.forest.pop_size == 512 and pipe.best_validation_tree is not None
    t, s = algo.forest.batch_node_type.cpu().numpy(), algo.forest.batch_subtree_size.cpu().numpy()
    assert all(S.check_prefix_tree(t[i], s[i]) for i in range(512))
