"""GPU: END_LEAN and the one-word leaf programs LEAF_C / LEAF_V (evogp_amd/csrc/gen/gen_tc_asm.py; sr_tc.hip TcCompileParams::end_id,
leaf_id) change no fitness word.

Every case runs twice in one process: with the switch on (evogp_hip_debug_tc_end(1): a launch that is single-output, MSE, without a ragged
tile and not in pieces ends its programs in END_LEAN, and a tree of one leaf is the one word LEAF_C / LEAF_V) and off (0: END, and push + END
for such a tree -- the words of before).  The fitness WORDS must be identical, and both must agree with the CPU oracle (same NaN / inf
classes, rtol 1e-5 on the finite values: helpers.assert_close_classes at the tolerance the parity tests use for + - * /).  The handler
histogram of the compiled programs says which END a launch got, so that a case that must keep END is known to have kept it."""
import ctypes
import json
import os

import numpy as np
import pytest

from helpers import ARITH, assert_close_classes, depth2leaf, roulette_uniform

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-5
CS3 = [-1.0, 0.0, 1.0]
T_VAR, T_CONST, T_UFUNC, T_BFUNC = 0, 1, 2, 3
ADD, SUB, MUL = 1, 2, 3
NEG, ABS = 25, 26
VARS = 10
NEW = ("end_lean", "leaf_c", "leaf_v")


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


def rows_to_forest(trees, L=64):
    pop = len(trees)
    v = np.zeros((pop, L), np.float32); t = np.zeros((pop, L), np.int16); s = np.zeros((pop, L), np.int16)
    for i, tr in enumerate(trees):
        assert len(tr) <= L and tr[0][2] == len(tr), i
        for j, (ty, val, sz) in enumerate(tr):
            t[i, j], v[i, j], s[i, j] = ty, val, sz
    return v, t, s


def leaf_forest():
    """every tree of one leaf: each variable, an index beyond the last variable (the engine clamps it), the constants 0, -0, 1, -1,
    +-inf, NaN and a denormal -- twice over, so that such trees are neighbours in a batch as well as first and last of one"""
    consts = [0.0, -0.0, 1.0, -1.0, float("inf"), -float("inf"), float("nan"), 1e-40]
    trees = [[(T_VAR, k, 1)] for k in range(VARS)] + [[(T_VAR, VARS + 5, 1)]] + [[(T_CONST, c, 1)] for c in consts]
    return rows_to_forest(trees + trees[::-1])


def for_the_oracle(forest):
    """the forest with variable indices clamped as the engine clamps them (the oracle indexes the row as it is told)"""
    v, t, s = (a.copy() for a in forest)
    m = (t == T_VAR) & (np.arange(v.shape[1])[None, :] < s[:, :1])
    v[m] = np.clip(v[m], 0, VARS - 1)
    return v, t, s


def one_leaf_words(forest):
    """trees that are one leaf and not the NaN constant (that one is NAN_TREE whatever the switch says)"""
    v, t, s = forest
    return int(((s[:, 0] == 1) & ~((t[:, 0] == T_CONST) & np.isnan(v[:, 0]))).sum())


def unary_forest():
    """chains of neg / abs (one instruction each) over a small sum, a variable added every seventh level: programs of 22 to 57
    instructions, so both sides of the 31 a record holds -- the longer ones continue behind NEXT in their overflow block"""
    r = np.random.default_rng(7)
    trees = []
    for i in range(240):
        tree = [(T_BFUNC, (ADD, SUB, MUL)[i % 3], 3), (T_VAR, i % VARS, 1), ((T_VAR, (i + 3) % VARS, 1) if i % 2 else (T_CONST, 0.5, 1))]
        for level in range(20 + i % 36):
            if level % 7 == 6 and len(tree) + 2 <= 62:
                tree = [(T_BFUNC, (ADD, SUB)[level % 2], len(tree) + 2)] + tree + [(T_VAR, int(r.integers(VARS)), 1)]
            elif len(tree) + 1 <= 62:
                tree = [(T_UFUNC, (NEG, ABS)[int(r.integers(2))], len(tree) + 1)] + tree
        trees.append(tree)
    return rows_to_forest(trees)


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def arith_and_leaves(oracle):
    def make():
        a = oracle.generate(777, 64, VARS, 1, 0.5, 0.5, [42, 0], depth2leaf(6), roulette_uniform(ARITH), CS3)
        return tuple(np.concatenate(p) for p in zip(a, leaf_forest()))
    return cached("arith+leaves", make)


def dataset(D, out_len=1):
    def make():
        r = np.random.default_rng(1000 + D)
        return r.uniform(-5, 5, (D, VARS)).astype(np.float32), r.uniform(-5, 5, (D, out_len)).astype(np.float32)
    return cached(("data", D, out_len), make)


def on_and_off(g, call, pop):
    """[(words, histogram)] with the switch on, then off"""
    out = []
    try:
        for mode in (1, 0):
            assert g.L.evogp_hip_debug_tc_end(mode) == 0
            w = np.asarray(call()).view(np.uint32).copy()
            out.append((w, histogram(g, pop)))
    finally:
        assert g.L.evogp_hip_debug_tc_end(-1) == 0
    return out


def check(g, oracle, name, forest, D, mse=True, out_len=1, lean=True):
    X, y = dataset(D, out_len)
    pop = forest[0].shape[0]
    (w1, h1), (w0, h0) = on_and_off(g, lambda: g.sr_fitness(*forest, X, y, mse), pop)
    print(f"{name} D={D} mse={mse}: on {({k: h1.get(k, 0) for k in NEW + ('end', 'next', 'skip')})}, off {({k: h0.get(k, 0) for k in NEW + ('end', 'next', 'skip')})}")
    diff = np.nonzero(w1 != w0)[0]
    assert len(diff) == 0, f"{name} D={D} mse={mse}: {len(diff)} fitness words differ, first trees {diff[:5]}: {w1[diff[:5]]} against {w0[diff[:5]]}"
    want = cached(("want", name, D, mse), lambda: oracle.sr_fitness(*for_the_oracle(forest), X, y, mse))
    assert_close_classes(w1.view(np.float32), want, RTOL, what=f"{name} D={D} mse={mse}, switch on")
    assert_close_classes(w0.view(np.float32), want, RTOL, what=f"{name} D={D} mse={mse}, switch off")
    assert all(h0.get(k, 0) == 0 for k in NEW), f"{name} D={D}: {h0} with the switch off"
    assert h1["skip"] == h0["skip"]
    if lean:
        assert h1["end_lean"] > 0 and h1["end"] == 0, f"{name} D={D}: END_LEAN {h1['end_lean']}, END {h1['end']}"
        assert h1["leaf_c"] + h1["leaf_v"] == one_leaf_words(forest), f"{name} D={D}: {h1['leaf_c']} + {h1['leaf_v']} leaf words, {one_leaf_words(forest)} such trees"
        assert h1["end_lean"] + h1["leaf_c"] + h1["leaf_v"] == h0["end"]
    else:
        assert all(h1.get(k, 0) == 0 for k in NEW), f"{name} D={D} mse={mse}: {h1} where END has to stay"
        assert h1 == h0
    return w1, h1, h0


# 512, 1024, 1536: one, two and three full tiles of the 8-row build, 3072: the six that fit LDS with ten variables (the leaf handlers' loop
# goes round twice more); 256: the 4-row build, 64: the 1-row build
@pytest.mark.parametrize("D", [512, 1024, 1536, 3072, 256, 64])
def test_full_tiles_take_the_lean_end(g, oracle, D):
    check(g, oracle, "arith+leaves", arith_and_leaves(oracle), D)


# 1000, 100: a ragged last tile (8-row and 4-row build); 8192: a dataset in pieces
@pytest.mark.parametrize("D", [1000, 100, 8192])
def test_ragged_tiles_and_pieces_keep_end(g, oracle, D):
    check(g, oracle, "arith+leaves", arith_and_leaves(oracle), D, lean=False)


def test_mean_absolute_error_keeps_end(g, oracle):
    check(g, oracle, "arith+leaves", arith_and_leaves(oracle), 1024, mse=False, lean=False)


def test_four_outputs_keep_end_mo(g, oracle):
    forest = cached("four", lambda: oracle.generate(500, 64, VARS, 4, 0.5, 0.5, [5, 5], depth2leaf(6), roulette_uniform(ARITH), CS3))
    _, h1, _ = check(g, oracle, "four outputs", forest, 1024, out_len=4, lean=False)
    assert h1["end_mo"] > 0


@pytest.mark.parametrize("D", [1024, 1536])   # two and three tiles: the window comes back once and twice per tree
def test_programs_of_two_blocks(g, oracle, D):
    forest = cached("unary", unary_forest)
    _, h1, h0 = check(g, oracle, "unary chains", forest, D)
    assert h1["next"] > 50 and h1["next"] == h0["next"], f"NEXT words: {h1['next']} on, {h0['next']} off"
    assert h1["end_lean"] == forest[0].shape[0] and h1["skip"] == 0


def test_a_call_is_the_concatenation_of_its_halves(g, oracle):
    forest = arith_and_leaves(oracle)
    X, y = dataset(1024)
    pop = forest[0].shape[0]
    whole = g.sr_fitness(*forest, X, y).view(np.uint32)
    for cut in (pop // 2, 8, pop - 3):
        halves = np.concatenate([g.sr_fitness(*(a[:cut] for a in forest), X, y), g.sr_fitness(*(a[cut:] for a in forest), X, y)]).view(np.uint32)
        assert np.array_equal(whole, halves), f"cut at {cut}: trees {np.nonzero(whole != halves)[0][:5]} differ"


def test_mode_is_checked(g):
    assert g.L.evogp_hip_debug_tc_end(2) != 0 and g.L.evogp_hip_debug_tc_end(-2) != 0
    assert g.L.evogp_hip_debug_tc_end(-1) == 0
