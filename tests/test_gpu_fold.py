"""GPU: NAN_TREE programs (evogp_amd/csrc/sr_tc.hip, compile_pack_arith) change no fitness word.

Every call runs twice in one process, with the arithmetic line's NaN-poisoned trees compiled to NAN_TREE (the default) and compiled
as before (evogp_hip_debug_tc_fold(0), what EVOGP_TC_FOLD=0 selects): the fitness WORDS must be identical.  The handler histogram of
the compiled programs must hold one NAN_TREE per tree the host restatement of the rule marks (tests/nan_trees.py), the same number
of SKIP words (trees left to the register kernels) and fewer words per tree."""
import ctypes
import json
import os

import numpy as np
import pytest

from nan_trees import crafted_forest, poisoned, special_dataset

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import gpu_capi

    return gpu_capi


def histogram(g, pop):
    """{handler name: words} of the programs the last sr_fitness call compiled (both flavours, twins counted with their handler)"""
    import torch

    nh = g.L.evogp_hip_debug_tc_nhandlers()
    hist = torch.zeros(2 * nh, dtype=torch.int64, device=g.DEV)
    rc = g.L.evogp_hip_debug_tc_histogram(pop, ctypes.c_void_p(hist.data_ptr()), 2 * nh, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, g.L.evogp_hip_error_string(rc)
    h = hist.cpu().numpy()
    table = json.load(open(os.path.join(ROOT, "evogp_amd", "lib", "tc_handlers.json")))["K8_short"]["handlers"]
    out = {}
    for name, v in table.items():
        base = name[:-3] if name.endswith("_np") else name
        out[base] = out.get(base, 0) + int(h[v["id"]] + h[nh + v["id"]])
    return out


def both_ways(g, call, pop):
    """(words, histogram) with NAN_TREE, then without"""
    out = []
    try:
        for fold in (1, 0):
            assert g.L.evogp_hip_debug_tc_fold(fold) == 0
            w = np.asarray(call()).view(np.uint32).copy()
            out.append((w, histogram(g, pop)))
    finally:
        assert g.L.evogp_hip_debug_tc_fold(-1) == 0
    return out


def check(g, call, pop, marked, what):
    (w1, h1), (w0, h0) = both_ways(g, call, pop)
    diff = np.nonzero(w1 != w0)[0]
    assert len(diff) == 0, f"{what}: {len(diff)} fitness words differ, first trees {diff[:5]}: {w1[diff[:5]]} against {w0[diff[:5]]}"
    assert h0.get("nan_tree", 0) == 0, f"{what}: NAN_TREE words with the rule off"
    assert h1["skip"] == h0["skip"], f"{what}: SKIP {h1['skip']} against {h0['skip']}"
    assert h1["nan_tree"] == int(marked.sum()), f"{what}: {h1['nan_tree']} NAN_TREE words, the rule marks {int(marked.sum())} trees"
    assert np.isnan(w1.view(np.float32)[marked]).all(), f"{what}: a marked tree is not NaN"
    words1, words0 = sum(h1.values()), sum(h0.values())
    if marked.any():
        assert words1 < words0, f"{what}: {words1} program words with the rule, {words0} without"
    return w1, h1, h0


def headline_census(forest, n):
    v = forest.batch_node_value[:n].cpu().numpy(); t = forest.batch_node_type[:n].cpu().numpy(); s = forest.batch_subtree_size[:n].cpu().numpy()
    return np.concatenate([poisoned(v[i:i + 100_000], t[i:i + 100_000], s[i:i + 100_000]) for i in range(0, n, 100_000)])


@pytest.mark.parametrize("pop", [1_000_000, 100_000])   # the headline call and configs[1]
@pytest.mark.parametrize("division", [2, 0])              # short (the default), ieee
def test_headline_forest(g, pop, division):
    import torch

    import bench

    forest, Xd, yd, X, y = bench.sr_inputs(0, pop, g.DEV)
    marked = headline_census(forest, pop)
    try:
        assert g.L.evogp_hip_set_sr_division(division) == 0
        w, h1, h0 = check(g, lambda: forest.SR_fitness(Xd, yd).cpu().numpy(), pop, marked, f"headline pop={pop} division={division}")
        # the unhinted operator (torch.ops.evogp_cuda.tree_SR_fitness) through the C ABI: the same words
        if pop == 100_000:
            v = forest.batch_node_value.cpu().numpy(); t = forest.batch_node_type.cpu().numpy(); s = forest.batch_subtree_size.cpu().numpy()
            check(g, lambda: g.sr_fitness(v, t, s, X, y), pop, marked, f"unhinted pop={pop} division={division}")
    finally:
        assert g.L.evogp_hip_set_sr_division(2) == 0
    assert h1["skip"] == 0 and h0["skip"] == 0
    per1, per0 = (sum(h1.values()) - h1["nan_tree"]) / pop, sum(h0.values()) / pop
    assert per1 < 0.8 * per0, f"interpreted words per tree {per1:.2f} against {per0:.2f}"
    torch.cuda.synchronize()


@pytest.mark.parametrize("D", [8, 100, 600, 12000])   # K1, K4, K8; the last runs in pieces
@pytest.mark.parametrize("mse", [True, False])
def test_crafted_forest(g, oracle, D, mse):
    from helpers import depth2leaf, roulette_uniform

    cv, ct, cs = crafted_forest()
    hv, ht, hs = oracle.generate(3000, 64, 6, 1, 0.5, 0.5, [D, 3], depth2leaf(6), roulette_uniform([1, 2, 3, 4]), [-1.0, 0.0, 1.0, np.inf, np.nan])
    v, t, s = (np.concatenate(p) for p in ((cv, hv), (ct, ht), (cs, hs)))
    pop = v.shape[0]
    X, y = special_dataset(D, 6, D)
    marked = poisoned(v, t, s)
    for division in (2, 0):
        try:
            assert g.L.evogp_hip_set_sr_division(division) == 0
            w, _, _ = check(g, lambda: g.sr_fitness(v, t, s, X, y, mse), pop, marked, f"crafted D={D} mse={mse} division={division}")
        finally:
            assert g.L.evogp_hip_set_sr_division(2) == 0
        want = oracle.sr_fitness(v, t, s, X, y, mse)
        got = w.view(np.float32)
        assert np.array_equal(np.isnan(got), np.isnan(want)), f"D={D} mse={mse}: NaN classes differ from the oracle"
