"""GPU: csrc/sr_rank.hip against tests/rank_ref.py fed with ``batch_forward`` of the same forest: words, status, scores and fused sums EQUAL (the
formula's three operations are correctly rounded on both sides); a segment, permutation, population, run or stream changes no bit; five generations."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import evogp_amd  # noqa: F401  (registers the ops)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forest_invariance as FI  # noqa: E402
import pair_cases as PC  # noqa: E402
import rank_ref as RR  # noqa: E402
import rank_tables as RT  # noqa: E402
import semantic_ref as S  # noqa: E402

from evogp_amd.algorithm import DefaultCrossover, DefaultMutation, DefaultSelection, GeneticProgramming  # noqa: E402
from evogp_amd.pipeline import StandardPipeline  # noqa: E402
from evogp_amd.problem import RankFitness  # noqa: E402
from evogp_amd.tree import Forest, GenerateDescriptor  # noqa: E402

pytestmark = pytest.mark.gpu
hip = torch.ops.evogp_hip

LAYOUTS = {
    "n1-n2": [0, 1, 3],
    "63-64-65": [0, 63, 127, 192],
    "1000": [0, 1000],                                  # padding inside one wave's network
    "1024": [0, 1024],                                  # the last shape of the small build
    "1025": [0, 1025],                                  # the first of the large one
    "8192": [0, 8192],
    "ragged-small": [0, 5, 70, 326, 1000, 1024],
    "ragged-large": [0, 300, 1500, 1501, 4001, 4100],   # below and above 1024 in one call
}
# (funcs, gp_len, pop, var_len): + - * / (constant trees, +-inf, NaN); sin exp log (the FULL build); a comb deeper than the register
# stack (gp_len 1024); var_len 33 (the general kernel alone)
FORESTS = {"arith": ("arith", 64, 128, 3), "all": ("all", 64, 128, 3), "deep": ("arith", 1024, 64, 3), "v33": ("all", 64, 64, 33)}
CASES = [(lay, "arith") for lay in LAYOUTS] + [("63-64-65", "all"), ("ragged-large", "all"), ("1000", "deep"), ("ragged-large", "deep"),
                                               ("63-64-65", "v33"), ("1025", "v33")]


def _dev(*arrs):
    return [torch.from_numpy(np.array(a, order="C")).cuda() for a in arrs]   # (a copy: the shared arrays are read-only)


def labels(D, var_len):
    """float32 labels with ties, -0.0 and +0.0, and their 0 / 1 split"""
    y = np.round(PC.pair_data(D, var_len)[1], 1)
    y[::max(2, D // 3)] = 0.0
    y[0] = -0.0
    return y, (y > np.median(y)).astype(np.int32)


def stats(f, X, q, seg, metric=0):
    """(words, fused, scores, status) of the op as numpy arrays"""
    seg = np.asarray(seg, np.int32)
    out = hip.tree_SR_rank_stats(*_dev(*f), *_dev(X, np.asarray(q, np.int32), seg), int(np.diff(seg).max()), metric, True, True, True)
    return [o.cpu().numpy() for o in out]


@functools.lru_cache(maxsize=None)
def truth(layout, forest):
    """the forest, the data and the restatement's words on batch_forward's predictions, once per case"""
    funcs, gp_len, pop, var_len = FORESTS[forest]
    seg = np.asarray(LAYOUTS[layout], np.int64)
    f = PC.pair_forest(funcs, gp_len, pop, var_len)
    X = PC.pair_data(int(seg[-1]), var_len)[0]
    y, y01 = labels(int(seg[-1]), var_len)
    P = Forest(var_len, 1, *_dev(*f)).batch_forward(_dev(X)[0])[:, :, 0].contiguous().cpu().numpy()
    q = RR.rank_rows(y, seg)[0]
    return f, X, seg, P, q, y01, RR.words(P, S.formed_mask(f[1], f[2]), q, seg)


@pytest.mark.parametrize("layout,forest,metric", [c + ("spearman",) for c in CASES] + [("ragged-large", "all", "auc")])   # (n = 1: one class)
def test_words_status_and_fused_sums_equal_the_restatement(layout, forest, metric):
    f, X, seg, P, q, y01, (want, status) = truth(layout, forest)
    ok = status == 0
    if metric == "auc":
        q, want = y01, RR.words(P, ok, y01, seg)[0]
    sc = RR.scores(want, RR.consts(q, seg), seg, metric)
    # the case holds what it is about, by the restatement alone: an unusable tree, an undefined segment, a tie run longer than a wave
    assert status.any() and ok.sum() >= 8 and (~np.isnan(sc[ok])).any() and np.isnan(sc[ok]).any()
    if np.diff(seg).max() > 64:
        a, b = [(a, b) for a, b in zip(seg[:-1], seg[1:]) if b - a > 64][0]
        assert max(np.unique(RR.keys(p[a:b]), return_counts=True)[1].max() for p in P[ok]) > 64
    w, fu, got, st = stats(f, X, q, seg, metric=["spearman", "auc"].index(metric))
    assert w.dtype == np.int64 and st.dtype == np.uint8 and np.array_equal(st, status), np.flatnonzero(st != status)[:8]
    assert np.array_equal(w, want), np.argwhere(w != want)[:8]
    # three correctly rounded operations on both sides: held to the BITS (measured equal; the derived bound (19 G + 2 G^2) 2^-53 is not needed)
    assert np.array_equal(got.view(np.int64)[ok], sc.view(np.int64)[ok]) and np.isnan(got[~ok]).all()
    assert np.array_equal(fu.view(np.int64)[ok], RR.fused(sc, status).view(np.int64)[ok]) and np.isnan(fu[~ok]).all()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_rank_rows_equals_the_restatement(layout):
    seg = np.asarray(LAYOUTS[layout], np.int32)
    (y, y01), mx = labels(int(seg[-1]), 3), int(np.diff(seg).max())
    for v in (y, np.where(np.arange(len(y)) == len(y) - 1, np.float32("nan"), y)):   # the second one: a NaN in the last segment
        r2, c, st = (t.cpu().numpy() for t in hip.rank_rows(*_dev(v), None, *_dev(seg), mx))
        wr2, wc, wst = RR.rank_rows(v, seg)
        assert np.array_equal(st, wst) and np.array_equal(r2, wr2) and np.array_equal(c, wc)
    c = hip.rank_rows(*_dev(y), *_dev(y01, seg), mx)[1].cpu().numpy()
    assert np.array_equal(c, RR.consts(y01, seg))


@pytest.mark.parametrize("forest", ["all", "deep"])
def test_words_depend_on_the_tree_and_the_segment_alone(forest):
    f, X, seg, P, q, y01, (want, status) = truth("ragged-large", forest)
    rng = np.random.default_rng(3)
    w = stats(f, X, q, seg)[0]
    # a segment alone (another build where it is short), its rows permuted with their payload
    for g in (0, 1, 3):
        a, b = seg[g], seg[g + 1]
        perm = a + rng.permutation(b - a)
        for rows in (np.arange(a, b), perm):
            alone = stats(f, X[rows], q[rows], [0, b - a])[0][:, 0]
            assert np.array_equal(alone[status == 0], w[status == 0, g])   # (a tree with a NaN in ANOTHER segment is usable alone)
    pick = rng.permutation(len(status))[:37]   # other neighbours, another batch, another population
    w2, _, _, st2 = stats(tuple(a[pick] for a in f), X, q, seg)
    assert np.array_equal(w2, w[pick]) and np.array_equal(st2, status[pick])


def test_two_calls_and_two_streams_give_the_same_bits():
    f, X, seg, P, q, y01, _ = truth("ragged-large", "all")
    args = _dev(*f) + _dev(X, q.astype(np.int32), seg.astype(np.int32)) + [int(np.diff(seg).max()), 0, True, True, True]
    outs = [hip.tree_SR_rank_stats(*args), hip.tree_SR_rank_stats(*args)]
    for _ in range(2):
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            outs.append(hip.tree_SR_rank_stats(*args))
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for other in outs[1:] for a, b in zip(outs[0], other))


@pytest.mark.parametrize("case", FI.cases_for(RT.RANK))
def test_op_keeps_the_invariants(case):
    FI.check(RT.RANK, FI.TABLE[RT.RANK], FI.build_case(case), "cuda")
    torch.cuda.synchronize()


def test_five_generations_under_rank_fitness():
    rng = np.random.default_rng(8)
    X = torch.from_numpy(rng.uniform(-2, 2, (600, 3)).astype(np.float32)).cuda()
    y = (X[:, 0] * X[:, 1] + X[:, 2]).contiguous()
    dates = torch.from_numpy(rng.integers(0, 6, 600)).cuda()
    d = GenerateDescriptor(max_tree_len=64, input_len=3, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=5, const_samples=[-1, 0, 1, 2])
    algo = GeneticProgramming(Forest.random_generate(512, d, keys=torch.tensor([1, 2], dtype=torch.uint32, device="cuda")), DefaultCrossover(),
                              DefaultMutation(0.2, d.update(max_layer_cnt=3)), DefaultSelection(0.3, 4))
    pipe = StandardPipeline(algo, RankFitness(X, y, metric="spearman", segments=dates), generation_limit=5, is_show_details=False)
    best = [float(pipe.step().max()) for _ in range(5)]   # (elites are copied: a generation's best never falls)
    assert pipe.best_tree is not None and np.isfinite(best).all() and all(b >= a for a, b in zip(best, best[1:])) and -1.0 <= best[-1] <= 1.0 + 1e-12
