"""GPU: the Z rule's NAN_TREE programs (evogp_amd/csrc/sr_tc.hip, compile_pack_arith, level 2 of evogp_hip_debug_tc_fold) change no
fitness word.

Every call runs twice in one process: at level 2 (the default: a tree with a NaN constant, or with a division whose divisor is proved +-0
or NaN in every row, is the one word NAN_TREE) and at level 0 (nothing marked, every tree interpreted in full).  The fitness WORDS must be
identical, in all three division modes (ieee, fast, short).  The handler histogram of the compiled programs must hold one NAN_TREE per
tree the host restatement of the rule marks (tests/zero_or_nan_trees.py), the same number of SKIP words (trees left to the register
kernels) and fewer words at level 2."""
import ctypes
import json
import os

import numpy as np
import pytest

from nan_trees import crafted_forest, poisoned, special_dataset
from zero_or_nan_trees import proved_nan

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIVISIONS = {0: "ieee", 1: "fast", 2: "short"}


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


def at_levels(g, call, pop, levels=(2, 0)):
    """[(words, histogram)] of the call at each level"""
    out = []
    try:
        for level in levels:
            assert g.L.evogp_hip_debug_tc_fold(level) == 0
            w = np.asarray(call()).view(np.uint32).copy()
            out.append((w, histogram(g, pop)))
    finally:
        assert g.L.evogp_hip_debug_tc_fold(-1) == 0
    return out


def check(g, call, pop, marked, what):
    (w2, h2), (w0, h0) = at_levels(g, call, pop)
    diff = np.nonzero(w2 != w0)[0]
    assert len(diff) == 0, f"{what}: {len(diff)} fitness words differ, first trees {diff[:5]}: {w2[diff[:5]]} against {w0[diff[:5]]}"
    assert h0.get("nan_tree", 0) == 0, f"{what}: NAN_TREE words at level 0"
    assert h2["skip"] == h0["skip"], f"{what}: SKIP {h2['skip']} against {h0['skip']}"
    assert h2["nan_tree"] == int(marked.sum()), f"{what}: {h2['nan_tree']} NAN_TREE words, the rule marks {int(marked.sum())} trees"
    assert np.isnan(w2.view(np.float32)[marked]).all(), f"{what}: a marked tree is not NaN"
    words2, words0 = sum(h2.values()), sum(h0.values())
    print(f"{what}: {h2['nan_tree']} NAN_TREE, program words {words2} against {words0}")
    if marked.any():
        assert words2 < words0, f"{what}: {words2} program words with the rule, {words0} without"
    return w2, h2, h0


def census(forest, n, rule):
    v = forest.batch_node_value[:n].cpu().numpy(); t = forest.batch_node_type[:n].cpu().numpy(); s = forest.batch_subtree_size[:n].cpu().numpy()
    return np.concatenate([rule(v[i:i + 100_000], t[i:i + 100_000], s[i:i + 100_000]) for i in range(0, n, 100_000)])


@pytest.mark.parametrize("pop", [1_000_000, 100_000])   # the headline call and configs[1]
@pytest.mark.parametrize("division", [2, 1, 0])
def test_headline_forest(g, pop, division):
    import torch

    import bench

    forest, Xd, yd, X, y = bench.sr_inputs(0, pop, g.DEV)
    marked = census(forest, pop, proved_nan)
    share = marked.mean()
    assert 0.34 < share < 0.37, f"{share:.4f} of the headline forest marked (the census of its first 100 000 trees: 0.354)"
    what = f"headline pop={pop} division={DIVISIONS[division]}"
    try:
        assert g.L.evogp_hip_set_sr_division(division) == 0
        w, h2, h0 = check(g, lambda: forest.SR_fitness(Xd, yd).cpu().numpy(), pop, marked, what)
        # level 1 is the rule of before: one NAN_TREE per tree tests/nan_trees.py marks, the same words
        (w1, h1), = at_levels(g, lambda: forest.SR_fitness(Xd, yd).cpu().numpy(), pop, levels=(1,))
        assert np.array_equal(w1, w) and h1["nan_tree"] == int(census(forest, pop, poisoned).sum())
        # the unhinted operator (torch.ops.evogp_cuda.tree_SR_fitness) through the C ABI: the same words
        if pop == 100_000:
            v = forest.batch_node_value.cpu().numpy(); t = forest.batch_node_type.cpu().numpy(); s = forest.batch_subtree_size.cpu().numpy()
            wu, _, _ = check(g, lambda: g.sr_fitness(v, t, s, X, y), pop, marked, "unhinted " + what)
            assert np.array_equal(wu, w), f"{what}: the unhinted call's words differ from the hinted call's"
    finally:
        assert g.L.evogp_hip_set_sr_division(2) == 0
    assert h2["skip"] == 0 and h0["skip"] == 0
    # the census: the Z rule's trees hold 18.5 % of the words the interpreter executes at level 1; at least half of that must be gone
    per2, per1, per0 = (sum(h2.values()) - h2["nan_tree"]) / pop, (sum(h1.values()) - h1["nan_tree"]) / pop, sum(h0.values()) / pop
    print(f"{what}: interpreted words per tree {per2:.3f} at level 2, {per1:.3f} at level 1, {per0:.3f} at level 0")
    assert per2 < 0.9 * per1 and per1 < 0.8 * per0, f"interpreted words per tree {per2:.2f} / {per1:.2f} / {per0:.2f} at levels 2 / 1 / 0"
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
    marked = proved_nan(v, t, s)
    assert marked.sum() > poisoned(v, t, s).sum()
    want = oracle.sr_fitness(v, t, s, X, y, mse)
    for division in (2, 1, 0):
        try:
            assert g.L.evogp_hip_set_sr_division(division) == 0
            w, _, _ = check(g, lambda: g.sr_fitness(v, t, s, X, y, mse), pop, marked, f"crafted D={D} mse={mse} division={DIVISIONS[division]}")
        finally:
            assert g.L.evogp_hip_set_sr_division(2) == 0
        got = w.view(np.float32)
        assert np.array_equal(np.isnan(got), np.isnan(want)), f"D={D} mse={mse} division={DIVISIONS[division]}: NaN classes differ from the oracle"


def test_level_is_checked(g):
    assert g.L.evogp_hip_debug_tc_fold(3) != 0 and g.L.evogp_hip_debug_tc_fold(-2) != 0
    assert g.L.evogp_hip_debug_tc_fold(-1) == 0
