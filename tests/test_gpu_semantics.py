"""GPU: semantic duplicate classes (csrc/sr_semantic.hip: tree_SR_semantic_hash, tree_SR_semantic_classes) against the numpy
restatement (tests/semantic_ref.py) on ``Forest.batch_forward``'s predictions of the same forest -- every output word, exactly: the
definition is on those bits, for all 29 functions -- under planted hash collisions and from run to run; the Forest methods,
SymbolicRegression(semantic_dedup=), GeneticProgramming(duplicate_classes=) on the fused step, and the binding's checks of the two ops."""
import os
import sys

import numpy as np
import pytest
import torch

import evogp_amd  # noqa: F401
from evogp_amd.tree import Forest, GenerateDescriptor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import semantic_ref as S  # noqa: E402
import test_gpu_binding_contract as BC  # noqa: E402
from semantic_cases import dataset, planted_forest  # noqa: E402
from test_semantic_ref import check_planted  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def _bits(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _ops(f, X, hash_=None):
    """(sig, class_id) of the two ops; ``hash_``: what the classes pass is given instead of the signatures"""
    shape = (f.pop_size, X.shape[0], f.max_tree_len, f.input_len, 1)
    sig = torch.ops.evogp_hip.tree_SR_semantic_hash(*shape, *f._tensors(), X)
    cid = torch.ops.evogp_hip.tree_SR_semantic_classes(*shape, *f._tensors(), X, sig if hash_ is None else hash_)
    return sig, cid


def _reference(f, X, type_, size):
    """(class_id, signature, keys) of the restatement on batch_forward's predictions"""
    P = f.batch_forward(X)[:, :, 0].cpu().numpy()
    formed = S.formed_mask(type_, size)
    return S.class_id(P, formed), S.signature(P, formed), S.keys(P)


def _compare(rng, pop, gp_len, D, var_len):
    value, type_, size = planted_forest(rng, pop, gp_len, var_len)
    f = Forest(var_len, 1, *_dev(value, type_, size))
    X, = _dev(dataset(rng, D, var_len))
    want_c, want_sig, K = _reference(f, X, type_, size)
    sig, cid = _ops(f, X)
    assert sig.dtype == torch.int64 and sig.shape == (pop,) and cid.dtype == torch.int32 and cid.shape == (pop,)
    got_sig, got_c = sig.cpu().numpy().view(np.uint64), cid.cpu().numpy()
    bad = np.flatnonzero(got_sig != want_sig)
    assert bad.size == 0, f"{bad.size} signatures differ, first rows {bad[:8]}, lengths {size[bad[:8], 0]}"
    bad = np.flatnonzero(got_c != want_c)
    assert bad.size == 0, f"{bad.size} class ids differ, first rows {bad[:8]}: got {got_c[bad[:8]]}, want {want_c[bad[:8]]}"
    if pop >= 63:
        check_planted(got_c, got_sig, K, size, gp_len, D)
    # determinism: a second call returns the same bits
    again_sig, again_c = _ops(f, X)
    assert torch.equal(again_sig, sig) and torch.equal(again_c, cid)
    return f, X, size, want_c, sig, cid


@pytest.mark.parametrize("D", [1, 130, 1100])
@pytest.mark.parametrize("pop", [1, 63, 200, 5000])
@pytest.mark.parametrize("gp_len", [64, 1024])
def test_hash_and_classes_match_the_restatement(rng, gp_len, pop, D):
    f, X, size, want_c, sig, cid = _compare(rng, pop, gp_len, D, 3)
    # the Forest methods are these two ops; keep="smallest" is the restatement's
    assert torch.equal(f.semantic_hash(X), sig)
    c1, r1 = f.semantic_classes(X)
    assert torch.equal(c1, cid) and r1.dtype == torch.bool and np.array_equal(r1.cpu().numpy(), want_c == np.arange(pop))
    small = S.smallest_representative(want_c, np.clip(size[:, 0].astype(np.int64), 0, gp_len))
    c2, r2 = f.semantic_classes(X, keep="smallest")
    assert c2.dtype == torch.int32 and np.array_equal(c2.cpu().numpy(), small) and np.array_equal(r2.cpu().numpy(), small == np.arange(pop))
    fu, inverse, counts = f.semantic_unique(X, keep="smallest")
    reps = np.flatnonzero(small == np.arange(pop))
    assert fu.pop_size == len(reps) and int(counts.sum()) == pop and np.array_equal(reps[inverse.cpu().numpy()], small)


def test_more_variables_than_the_register_tuples_hold(rng):
    """var_len 40 > 32: every tree goes through the scratch-stack kernel"""
    _compare(rng, 200, 64, 130, 40)


def test_multi_output_forests_are_refused(rng):
    value, type_, size = planted_forest(rng, 63, 64)
    f = Forest(3, 2, *_dev(value, type_, size))
    X, = _dev(dataset(rng, 8))
    for call in (lambda: f.semantic_hash(X), lambda: f.semantic_classes(X), lambda: f.semantic_unique(X)):
        with pytest.raises(ValueError, match="single-output"):
            call()


@pytest.mark.parametrize("gp_len", [64, 1024])
def test_classes_do_not_depend_on_the_hashes(rng, gp_len):
    value, type_, size = planted_forest(rng, 200, gp_len)
    f = Forest(3, 1, *_dev(value, type_, size))
    X, = _dev(dataset(rng, 130))
    want, _, _ = _reference(f, X, type_, size)
    assert np.array_equal(_ops(f, X)[1].cpu().numpy(), want)
    # one run of 200 colliding trees
    assert np.array_equal(_ops(f, X, torch.zeros(200, dtype=torch.int64, device="cuda"))[1].cpu().numpy(), want)
    # two interleaved runs of distinct classes: classes alternate between the two hash words (equal trees still share a word)
    rank = np.cumsum(want == np.arange(200)) - 1
    two = torch.from_numpy((rank[want] % 2).astype(np.int64) * 0x7000000000000001 - 5).cuda()
    assert np.array_equal(_ops(f, X, two)[1].cpu().numpy(), want)
    # every tree a run of its own is only legal when no two trees are equal: on the representatives alone
    reps = np.flatnonzero(want == np.arange(200))
    fr = Forest(3, 1, *_dev(value[reps], type_[reps], size[reps]))
    own = torch.arange(len(reps), dtype=torch.int64, device="cuda") * -7
    assert np.array_equal(_ops(fr, X, own)[1].cpu().numpy(), np.arange(len(reps)))


def test_problem_scores_only_the_representatives(rng):
    from evogp_amd.problem import SymbolicRegression

    pop = 200
    value, type_, size = planted_forest(rng, pop, 64)
    f = Forest(3, 1, *_dev(value, type_, size))
    X, = _dev(dataset(rng, 130))
    y = (X[:, :1] * X[:, 1:2] - X[:, 2:3] / 1.5).contiguous()
    want, _, _ = _reference(f, X, type_, size)
    small = S.smallest_representative(want, np.clip(size[:, 0].astype(np.int64), 0, 64))
    plain = SymbolicRegression(datapoints=X, labels=y)
    base_scores, base_fit = plain.scores(f), plain.evaluate(f)
    assert np.array_equal(plain.semantic_classes(f)[0].cpu().numpy(), small)
    for keep, classes in (("smallest", small), ("first", want)):
        prob = SymbolicRegression(datapoints=X, labels=y, semantic_dedup=True, semantic_keep=keep)
        is_rep = classes == np.arange(pop)
        scores, fit = prob.scores(f), prob.evaluate(f)
        assert np.array_equal(_bits(scores)[is_rep], _bits(base_scores)[is_rep]) and np.isneginf(scores.cpu().numpy()[~is_rep]).all()
        assert np.array_equal(_bits(fit)[is_rep], _bits(base_fit)[is_rep]) and np.isnan(fit.cpu().numpy()[~is_rep]).all()
        assert np.isfinite(scores.cpu().numpy()[is_rep]).sum() > 40 and (~is_rep).sum() > 20
    scaled = SymbolicRegression(datapoints=X, labels=y, linear_scaling=True)
    both = SymbolicRegression(datapoints=X, labels=y, linear_scaling=True, semantic_dedup=True)
    is_rep = small == np.arange(pop)
    a, b = scaled.scores(f), both.scores(f)
    assert np.array_equal(_bits(a)[is_rep], _bits(b)[is_rep]) and np.isneginf(b.cpu().numpy()[~is_rep]).all()
    with pytest.raises(ValueError, match="multigene"):
        SymbolicRegression(datapoints=X, labels=y, multigene=True, semantic_dedup=True)


def test_regenerate_semantic_duplicates_on_the_fused_step(oracle):
    from evogp_amd.algorithm import DefaultCrossover, DefaultMutation, DefaultSelection, GeneticProgramming
    from evogp_amd.problem import SymbolicRegression

    d = GenerateDescriptor(max_tree_len=32, input_len=2, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=3,
                           const_samples=[-1, 0, 1])
    data = np.random.default_rng(7)
    fitness = torch.from_numpy(data.uniform(-1, 0, 500).astype(np.float32)).cuda()
    X = torch.from_numpy(data.uniform(0.5, 1.5, (100, 2)).astype(np.float32)).cuda()
    problem = SymbolicRegression(datapoints=X, labels=(X[:, :1] * X[:, 1:2]).contiguous())
    keys = torch.tensor([3, 4], dtype=torch.uint32, device="cuda")

    def run(**kw):
        torch.manual_seed(5)
        algo = GeneticProgramming(Forest.random_generate(500, d, keys=keys), DefaultCrossover(), DefaultMutation(0.2, d),
                                  DefaultSelection(0.3, 5), **kw)
        assert algo._native_plan() is not None   # the fused step
        return algo.step(fitness)

    plain = run()
    fresh = run(regenerate_duplicates=d.update(max_layer_cnt=4), duplicate_classes=problem.semantic_classes)
    assert fresh.func_mask == plain.func_mask != 0
    rep = problem.semantic_classes(plain)[1].cpu().numpy()
    first = plain.duplicate_classes()[1].cpu().numpy()
    assert 0 < (~first).sum() < (~rep).sum() < 495   # semantic duplicates hold the structural ones and more
    for a, b in zip(plain._tensors(), fresh._tensors()):
        assert np.array_equal(_bits(a)[rep], _bits(b)[rep])                  # representatives: untouched, bit for bit
    assert any(not np.array_equal(_bits(a)[~rep], _bits(b)[~rep]) for a, b in zip(plain._tensors(), fresh._tensors()))
    t, s = fresh.batch_node_type.cpu().numpy(), fresh.batch_subtree_size.cpu().numpy()
    assert all(oracle.validate_tree(t[i], s[i]) == 0 for i in np.flatnonzero(~rep))
    assert int(problem.semantic_classes(fresh)[1].sum()) >= int(rep.sum())   # the semantic class count does not fall


# The two new ops join the binding-contract table (tests/test_gpu_binding_contract.py: one row per op, every argument faulted in turn;
# its test_the_table_covers_every_op reads the table when it runs).  The rows are checked below, by that module's own test body.
_SCALARS = dict(BC.SIZES, out_len=(2,), data_points=(0,), var_len=(0,))
_SEMANTIC_ROWS = {
    "evogp_hip::tree_SR_semantic_hash": lambda: dict(args=BC._data_head(use_mse=False) + BC._forest() + [BC._f("variables", BC.D, BC.V)],
                                                     outs=[((BC.POP,), BC.I64)], scalars=_SCALARS),
    "evogp_hip::tree_SR_semantic_classes": lambda: dict(
        args=BC._data_head(use_mse=False) + BC._forest() + [BC._f("variables", BC.D, BC.V),
                                                            ("hash", torch.zeros(BC.POP, dtype=BC.I64, device="cuda"))],
        outs=[((BC.POP,), BC.I32)], scalars=_SCALARS),
}
BC.TABLE.update(_SEMANTIC_ROWS)


@pytest.mark.parametrize("op", sorted(_SEMANTIC_ROWS))
def test_binding_contract_of_the_new_ops(op):
    BC.test_valid_call_and_one_fault_at_a_time(op)
    row = _SEMANTIC_ROWS[op]()
    out = getattr(torch.ops.evogp_hip, op.split("::")[1])(*[a for _, a in row["args"]])
    if op.endswith("classes"):   # four equal CONST leaves: one class
        assert out.cpu().tolist() == [0, 0, 0, 0]
    else:
        assert len(set(out.cpu().tolist())) == 1 and out[0].item() != 0
