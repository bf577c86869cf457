"""GPU: the per-subtree signatures (csrc/sr_subtree_sig.hip sr_subtree_sig_kernel) against an independent kernel -- every subtree
extracted into a row of its own and hashed by tree_SR_semantic_hash, the register interpreter -- on every path of the launch plan (LDS
and global tapes, one to four waves, ragged tiles), the library's choice (evogp_hip_subtree_library_select) against the dict loop of
tests/sublib_ref.py, exactly, determinism on one stream and on two, the forest invariants and the binding contract of the two ops, and
five generations with a library rebuilt from the population's subtrees in front of every mutation."""
import os
import sys

import numpy as np
import pytest
import torch

import evogp_amd  # noqa: F401  (registers the ops)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forest_invariance as FI  # noqa: E402
import sublib_ref as SL  # noqa: E402
import sublib_tables as ST  # noqa: E402
import subtree_ref as S  # noqa: E402
from grad_trees import ALL_FUNCS, ARITH, random_forest  # noqa: E402
from test_gpu_subtree import _all_subtrees, _malform  # noqa: E402

from evogp_amd.algorithm import (ApproxGeometricCrossover, BaseMutation, DefaultCrossover, DefaultMutation, DefaultSelection,  # noqa: E402
                                 GeneticProgramming, SemanticBackpropMutation, SemanticLibrary)
from evogp_amd.problem import SymbolicRegression  # noqa: E402
from evogp_amd.tree import Forest, GenerateDescriptor  # noqa: E402

pytestmark = pytest.mark.gpu
hip = torch.ops.evogp_hip


def _dev(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def signatures(forest, X):
    pop, L = forest[0].shape
    return hip.tree_SR_subtree_signatures(pop, X.shape[0], L, X.shape[1], 1, *_dev(*forest), _dev(X)[0]).cpu().numpy().view(np.uint64)


def tree_hash(forest, X):
    pop, L = forest[0].shape
    return hip.tree_SR_semantic_hash(pop, X.shape[0], L, X.shape[1], 1, *_dev(*forest), _dev(X)[0]).cpu().numpy().view(np.uint64)


def select(sig, size, min_size, max_size, k):
    m, c, n = hip.subtree_library_select(*_dev(np.ascontiguousarray(sig).view(np.int64), size), min_size, max_size, k)
    torch.cuda.synchronize()
    return m.cpu().numpy(), c.cpu().numpy(), int(n.item())


def _data(rng, D, var_len):
    return rng.uniform(0.5, 1.5, (D, var_len)).astype(np.float32)


# ---- 1. signatures against the register interpreter on extracted subtrees -----------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 63, 64, 65, 300])
@pytest.mark.parametrize("gp_len", [64, 1024])
@pytest.mark.parametrize("funcs", ["arith", "all"])
def test_every_live_node_carries_the_signature_of_its_extracted_row(rng, funcs, gp_len, D):
    pop, var_len = 24, 3
    forest = random_forest(rng, pop, gp_len, ARITH if funcs == "arith" else ALL_FUNCS, var_len, 1, max_depth=5)
    X = _data(rng, D, var_len)
    bad = _malform(*forest)
    good = [t for t in range(pop) if t not in bad]
    sig = signatures(forest, X)
    sub, owner, node = _all_subtrees(*forest, trees=good)
    want = np.zeros_like(sig)
    want[owner, node] = tree_hash(sub, X)
    live = np.arange(gp_len)[None, :] < forest[2][:, :1]
    live[list(bad)] = False
    assert len(owner) == live.sum() and (want[live] != 0).all()
    diff = np.argwhere(sig != want)
    assert not len(diff), (len(diff), diff[:4].tolist(), [hex(int(sig[tuple(d)])) for d in diff[:4]])
    assert not sig[~live].any() and not sig[list(bad)].any()
    assert np.array_equal(sig[:, 0], tree_hash(forest, X))


def test_a_population_that_fills_the_chip_takes_one_wave_per_tree(rng):
    pop, L, D, var_len = 4100, 64, 70, 3
    assert pop >= 16 * torch.cuda.get_device_properties(0).multi_processor_count, "the plan gives a tree one wave from 16 trees per compute unit on"
    forest = random_forest(rng, pop, L, ARITH, var_len, 1, max_depth=3)
    X = _data(rng, D, var_len)
    sig = signatures(forest, X)
    assert np.array_equal(sig[:, 0], tree_hash(forest, X))
    live = np.argwhere((np.arange(L)[None, :] < forest[2][:, :1]) & (np.arange(L)[None, :] > 0))
    pick = live[rng.choice(len(live), 200, replace=False)]
    rows, _, _ = SL.extract(*forest, pick[:, 0] * L + pick[:, 1])
    assert np.array_equal(sig[pick[:, 0], pick[:, 1]], tree_hash(rows, X))
    assert not sig[np.arange(L)[None, :] >= forest[2][:, :1]].any()


def test_wide_inputs(rng):
    pop, L, D, var_len = 24, 64, 65, 40
    forest = random_forest(rng, pop, L, ALL_FUNCS, var_len, 1, max_depth=5)
    X = _data(rng, D, var_len)
    sig = signatures(forest, X)
    sub, owner, node = _all_subtrees(*forest)
    assert np.array_equal(sig[owner, node], tree_hash(sub, X)) and (sig != 0).sum() == len(owner)


# ---- 2. the selection against the restatement ---------------------------------------------------------------------------------------------
_SELECT_CASES = {"257x64": (257, 64, 5), "4100x64": (4100, 64, 3), "24x1024": (24, 1024, 7)}
_cache = {}


def _select_case(name):
    if name not in _cache:
        pop, L, depth = _SELECT_CASES[name]
        rng = np.random.default_rng([20261021, pop, L])
        forest = random_forest(rng, pop, L, ARITH, 3, 1, max_depth=depth)
        sig = signatures(forest, _data(rng, 70, 3))
        _cache[name] = (forest[2], sig)
    return _cache[name]


@pytest.mark.parametrize("window", [(1, 1024), (2, 7)])
@pytest.mark.parametrize("k", [1, 7, 1024])
@pytest.mark.parametrize("name", sorted(_SELECT_CASES))
def test_selection_equals_the_restatement(name, k, window):
    size, sig = _select_case(name)
    key = (name, window)
    if key not in _cache:   # (one dict loop per forest and window: k only truncates)
        _cache[key] = SL.select(sig, size, *window, 1024)
    wm, wc, wn = _cache[key]
    member, count, n = select(sig, size, *window, k)
    print(f"{name} window {window} k {k}: {n} classes, the largest of {int(wc[0])} members")
    assert n == wn and n > 7, (n, wn)
    assert np.array_equal(member, wm[:k]) and np.array_equal(count, wc[:k])
    if name == "4100x64" and window[0] == 1:
        assert count[0] > 1000, "a class of thousands of members (a variable)"


def test_selection_of_nothing_and_of_a_planted_zero(rng):
    forest = random_forest(rng, 24, 64, ARITH, 3, 1, max_depth=4)
    X = _data(rng, 70, 3)
    broken = tuple(a.copy() for a in forest)
    broken[1][:, :] = S.T_CONST
    broken[2][:, 0] = 5           # every row: leaves only under n = 5
    sig = signatures(broken, X)
    assert not sig.any()
    member, count, n = select(sig, broken[2], 1, 64, 16)
    assert n == 0 and (member == -1).all() and not count.any()
    sig = signatures(forest, X)
    wm, wc, wn = SL.select(sig, forest[2], 1, 64, 1024)
    lone = int(wm[np.flatnonzero(wc == 1)[0]])      # a class of one member: without its word the class is gone
    sig.reshape(-1)[lone] = 0
    member, count, n = select(sig, forest[2], 1, 64, 1024)
    wm2, wc2, wn2 = SL.select(sig, forest[2], 1, 64, 1024)
    assert n == wn2 == wn - 1 and lone not in member.tolist() and np.array_equal(member, wm2) and np.array_equal(count, wc2)
    few = select(sig, forest[2], 64, 64, 1024)       # no subtree of 64 nodes: a window nothing falls into
    assert few[2] == 0 and (few[0] == -1).all()


# ---- 3. determinism -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gp_len", [64, 1024])
def test_two_calls_and_two_streams_give_the_same_bits(rng, gp_len):
    pop, D, var_len = 300, 300, 3
    forest = _dev(*random_forest(rng, pop, gp_len, ALL_FUNCS, var_len, 1, max_depth=5))
    X = _dev(_data(rng, D, var_len))[0]

    def both():
        sig = hip.tree_SR_subtree_signatures(pop, D, gp_len, var_len, 1, *forest, X)
        return (sig,) + tuple(hip.subtree_library_select(sig, forest[2], 1, 9, 1024))

    first, second = both(), both()
    outs = []
    for _ in range(2):
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            outs.append(both())
        stream.synchronize()
    torch.cuda.synchronize()
    assert (first[0] != 0).any() and int(first[3].item()) > 100
    for other in (second, outs[0], outs[1]):
        assert all(torch.equal(a, b) for a, b in zip(first, other))


# ---- 4. the tables ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FI.cases_for(ST.SIGNATURES))
def test_op_keeps_the_invariants(case):
    FI.check(ST.SIGNATURES, FI.TABLE[ST.SIGNATURES], FI.build_case(case), "cuda")
    torch.cuda.synchronize()


@pytest.mark.parametrize("op", sorted(ST.ROWS))
def test_binding_contract(op):
    ST.BC.test_valid_call_and_one_fault_at_a_time(op)
    row = ST.ROWS[op]()
    out = getattr(hip, op.split("::")[1])(*[a for _, a in row["args"]])
    if op == ST.SELECT:       # every word 1, every size 1: one class of POP * L members, represented by word 0
        assert out[0].cpu().tolist() == [0] + [-1] * (ST.K - 1) and out[1].cpu().tolist() == [ST.BC.POP * ST.BC.L] + [0] * (ST.K - 1)
        assert out[2].cpu().tolist() == [1]
    else:                     # four CONST leaves: one signature in column 0, zeros behind it
        sig = out.cpu().numpy()
        assert len(set(sig[:, 0].tolist())) == 1 and sig[0, 0] != 0 and not sig[:, 1:].any()


# ---- 5. end to end -------------------------------------------------------------------------------------------------------------------------
class _Recording(BaseMutation):
    """hands the call on and keeps a copy of the forest the operator was handed"""
    takes_skip_rows = True

    def __init__(self, op):
        self.op, self.handed = op, []

    def __call__(self, forest, skip_rows=0):
        self.handed.append(Forest(forest.input_len, 1, *(a.clone() for a in forest._tensors())))
        return self.op(forest, skip_rows)


def test_five_generations_with_a_library_rebuilt_from_the_population():
    rng = np.random.default_rng(8)
    X = torch.from_numpy(rng.uniform(-2, 2, (128, 3)).astype(np.float32)).cuda()
    y = (X[:, :1] * X[:, 1:2] + X[:, 2:3] / (1.5 + X[:, :1] ** 2)).contiguous()
    d = GenerateDescriptor(max_tree_len=64, input_len=3, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=5, const_samples=[-1, 0, 1, 2])
    torch.manual_seed(3)
    shared = SemanticLibrary(X, descriptor=d.update(max_layer_cnt=3), library_size=64)
    rdo = SemanticBackpropMutation(0.3, X, y, library=shared, fallback=DefaultMutation(0.3, d.update(max_layer_cnt=3)), refresh_every=1, refresh_max_size=7)
    agx = ApproxGeometricCrossover(X, library=shared, fallback=DefaultCrossover())
    rec = _Recording(rdo)
    algo = GeneticProgramming(Forest.random_generate(512, d, keys=torch.tensor([1, 2], dtype=torch.uint32, device="cuda")), agx, rec, DefaultSelection(0.3, 4))
    problem = SymbolicRegression(datapoints=X, labels=y)
    for gen in range(5):
        algo.step(problem.scores(algo.forest))
        handed = rec.handed[gen]
        lib = shared.library
        assert agx.library is lib and 1 <= lib.pop_size <= 1024 and lib.max_tree_len == 64
        assert int(lib.batch_subtree_size[:, 0].max()) <= 7 and int(lib.batch_subtree_size[:, 0].min()) >= 1
        assert torch.equal(shared.semantics.view(torch.int32), lib.batch_forward(X)[:, :, 0].contiguous().view(torch.int32))
        # every member is a subtree of the forest the operator was handed: tree / node reproduce the candidates word for word
        cand, counts, tree, node = handed.subtree_library(X, 1024, 1, 7)
        assert cand.pop_size == counts.shape[0] >= lib.pop_size and int(counts.sum()) <= int((handed.batch_subtree_size <= 7).sum())
        hv, ht, hs = (a.cpu().numpy() for a in handed._tensors())
        (wv, wt, ws), wtree, wnode = SL.extract(hv, ht, hs, (tree * 64 + node).cpu().numpy())
        cv, ct, cs = (a.cpu().numpy() for a in cand._tensors())
        assert np.array_equal(cv.view(np.uint32), wv.view(np.uint32)) and np.array_equal(ct, wt) and np.array_equal(cs, ws)
        have = {cv[j].tobytes() + ct[j].tobytes() + cs[j].tobytes() for j in range(cand.pop_size)}
        lv, lt, ls = (a.cpu().numpy() for a in lib._tensors())
        assert all(lv[j].tobytes() + lt[j].tobytes() + ls[j].tobytes() in have for j in range(lib.pop_size))
    assert len(rec.handed) == 5 and algo.forest.pop_size == 512
    t, s = algo.forest.batch_node_type.cpu().numpy(), algo.forest.batch_subtree_size.cpu().numpy()
    assert all(S.check_prefix_tree(t[i], s[i]) for i in range(512))
