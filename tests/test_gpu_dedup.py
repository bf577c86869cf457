"""GPU: structural duplicate detection (csrc/dedup.hip: tree_hash, tree_classes) against the numpy restatement (tests/dedup_ref.py),
bit for bit, under planted hash collisions and from run to run; ``dedup=True`` of Forest.optimize_constants / Forest.simplify against
the plain calls, bit for bit; GeneticProgramming(regenerate_duplicates=) on the fused step."""
import os
import sys

import numpy as np
import pytest
import torch

import evogp_amd  # noqa: F401
from evogp_amd.tree import Forest, GenerateDescriptor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dedup_ref as D  # noqa: E402
from dedup_cases import half_copies, planted_forest  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def _bits(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _hash(v, t, s):
    return torch.ops.evogp_hip.tree_hash(v, t, s)


def _classes(v, t, s, h):
    return torch.ops.evogp_hip.tree_classes(v, t, s, h).cpu().numpy()


@pytest.mark.parametrize("pop", [1, 63, 200, 5000])
@pytest.mark.parametrize("gp_len", [64, 1024])
def test_hash_and_classes_match_the_restatement(rng, gp_len, pop):
    value, type_, size = planted_forest(rng, pop, gp_len)
    want_h, want_c = D.tree_hash(value, type_, size), D.class_id(value, type_, size)
    v, t, s = _dev(value, type_, size)
    h = _hash(v, t, s)
    assert h.dtype == torch.int64 and h.shape == (pop,)
    assert np.array_equal(h.cpu().numpy().view(np.uint64), want_h)
    got = torch.ops.evogp_hip.tree_classes(v, t, s, h)
    assert got.dtype == torch.int32 and got.shape == (pop,)
    assert np.array_equal(got.cpu().numpy(), want_c)
    if pop >= 63:   # the planted rows (tests/dedup_cases.py), spelled out
        c = want_c
        assert c[10] == c[40] == c[pop - 20] == c[pop - 1] == c[3] and c[21] == c[20] and c[53] == c[50] and size[50, 0] == gp_len
        assert c[22] != c[23] and c[24] != c[25] and c[26] != c[27] and c[28] != c[29]
        assert [int(c[k]) for k in (30, 31, 32, 33)] == [30, 31, 32, 33] and all(want_h[k] == 0 for k in (30, 31, 32, 33))
        if gp_len > 64:
            assert size[41, 0] > 64 and c[44] == c[41] and c[47] == 47
    # determinism: a second call returns the same bits
    assert torch.equal(_hash(v, t, s), h) and torch.equal(torch.ops.evogp_hip.tree_classes(v, t, s, h), got)
    # the Forest methods are these two ops
    f = Forest(3, 2, v, t, s)
    cid, first = f.duplicate_classes()
    assert torch.equal(f.structure_hash(), h) and torch.equal(cid, got) and np.array_equal(first.cpu().numpy(), want_c == np.arange(pop))
    fu, inverse, counts = f.unique()
    assert fu.pop_size == int((want_c == np.arange(pop)).sum()) and int(counts.sum()) == pop
    assert np.array_equal(np.flatnonzero(want_c == np.arange(pop))[inverse.cpu().numpy()], want_c)


@pytest.mark.parametrize("gp_len", [64, 1024])
def test_classes_do_not_depend_on_the_hashes(rng, gp_len):
    value, type_, size = planted_forest(rng, 200, gp_len)
    want = D.class_id(value, type_, size)
    v, t, s = _dev(value, type_, size)
    assert np.array_equal(_classes(v, t, s, _hash(v, t, s)), want)
    # one run of 200 colliding rows
    assert np.array_equal(_classes(v, t, s, torch.zeros(200, dtype=torch.int64, device="cuda")), want)
    # two interleaved runs of distinct trees: classes alternate between the two hash words (equal rows still share a word)
    rank = np.cumsum(want == np.arange(200)) - 1
    two = torch.from_numpy((rank[want] % 2).astype(np.int64) * 0x7000000000000001 - 5).cuda()
    assert np.array_equal(_classes(v, t, s, two), want)
    # every row a run of its own is only legal when no two rows are equal: on the representatives alone
    reps = np.flatnonzero(want == np.arange(200))
    vr, tr, sr = _dev(value[reps], type_[reps], size[reps])
    own = torch.arange(len(reps), dtype=torch.int64, device="cuda") * -7
    assert np.array_equal(_classes(vr, tr, sr, own), np.arange(len(reps)))


@pytest.fixture(scope="module", params=[64, 1024])
def copies(request):
    """pop 256, half of it copies, D = 130 (three tiles of 64 rows, the last one ragged)"""
    gp_len = request.param
    rng = np.random.default_rng([20261018, gp_len])
    value, type_, size = half_copies(rng, 256, gp_len)
    X = rng.uniform(0.5, 1.5, (130, 3)).astype(np.float32)
    y = (X[:, :1] * X[:, 1:2] + 0.5 * X[:, 2:3]).astype(np.float32)
    first = D.class_id(value, type_, size) == np.arange(256)
    assert 90 <= first.sum() <= 130   # (the random half holds a few equal small trees of its own)
    return Forest(3, 1, *_dev(value, type_, size)), _dev(X, y), size


@pytest.mark.parametrize("what", ["descent", "lm", "simplify"])
def test_dedup_changes_no_bit(copies, what):
    f, (X, y), size = copies
    keep = [a.clone() for a in f._tensors()]
    if what == "simplify":
        plain_f, plain_loss = f.simplify(X, y)
        dedup_f, dedup_loss = f.simplify(X, y, dedup=True)
    else:
        plain_f, plain_loss = f.optimize_constants(X, y, steps=2, method=what)
        dedup_f, dedup_loss = f.optimize_constants(X, y, steps=2, method=what, dedup=True)
    for a, b in zip(keep, f._tensors()):
        assert torch.equal(a, b)   # the input forest is untouched
    # DESIGN.md sections 3.7, 3.10, 3.11: a tree's reduction order is fixed, so its bits cannot depend on its neighbours
    for name, a, b in zip(("value", "type", "size"), plain_f._tensors(), dedup_f._tensors()):
        differ = np.flatnonzero((_bits(a) != _bits(b)).any(axis=1))
        assert differ.size == 0, f"{what}: {name} differs in rows {differ[:8]}"
    differ = np.flatnonzero(_bits(plain_loss) != _bits(dedup_loss))
    assert differ.size == 0, f"{what}: loss differs in rows {differ[:8]}"
    loss = plain_loss.cpu().numpy()
    assert np.isnan(loss[[1, 2]]).all() and np.isfinite(loss).sum() > 200
    if what != "simplify":
        assert not torch.equal(plain_f.batch_node_value, f.batch_node_value)   # (something was tuned)
    assert np.array_equal(dedup_f.batch_subtree_size.cpu().numpy()[:, 0] == 0, size[:, 0] == 0)   # no empty row the input did not have


def test_regenerate_duplicates_on_the_fused_step(oracle):
    from evogp_amd.algorithm import DefaultCrossover, DefaultMutation, DefaultSelection, GeneticProgramming

    d = GenerateDescriptor(max_tree_len=32, input_len=2, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=3,
                           const_samples=[-1, 0, 1])
    fitness = torch.from_numpy(np.random.default_rng(7).uniform(-1, 0, 500).astype(np.float32)).cuda()
    keys = torch.tensor([3, 4], dtype=torch.uint32, device="cuda")

    def run(**kw):
        torch.manual_seed(5)
        algo = GeneticProgramming(Forest.random_generate(500, d, keys=keys), DefaultCrossover(), DefaultMutation(0.2, d),
                                  DefaultSelection(0.3, 5), **kw)
        assert algo._native_plan() is not None   # the fused step
        return algo.step(fitness)

    plain = run()
    fresh = run(regenerate_duplicates=d.update(max_layer_cnt=4))
    assert fresh.func_mask == plain.func_mask != 0
    first = plain.duplicate_classes()[1].cpu().numpy()
    assert first[0] and 0 < (~first).sum() < 495
    for a, b in zip(plain._tensors(), fresh._tensors()):
        assert np.array_equal(_bits(a)[first], _bits(b)[first])              # first members: untouched, bit for bit
    assert any(not np.array_equal(_bits(a)[~first], _bits(b)[~first]) for a, b in zip(plain._tensors(), fresh._tensors()))
    t, s = fresh.batch_node_type.cpu().numpy(), fresh.batch_subtree_size.cpu().numpy()
    assert all(oracle.validate_tree(t[i], s[i]) == 0 for i in np.flatnonzero(~first))
    assert int(fresh.duplicate_classes()[1].sum()) >= int(first.sum())       # the class count does not fall
