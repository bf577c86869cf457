"""GPU: the packed compiler's word table (evogp_amd/csrc/sr_tc.hip tc_table_entry; evogp_hip_debug_tc_table) changes no program word.

Program words.  A crafted forest -- every operator x operand kinds {variable, constant, function on the stack, function of two constants}
on either side, constants {0, -0, 1, -1, 2, 0.5, 2^-126, a denormal, inf, NaN}, each such node as a tree's root and as the left and the right
operand of another node, "no function" nodes (id 29) over every kind of operand, a row without a tree, divisions of the three in-place
forms at every stack height up to the interpreter's depth and beyond, blocks of trees sized so that one, two and three trees share a pass
and trees end on lane 63 -- is compiled with the table and with the selects, and the programs (evogp_hip_debug_tc_program, cut at the word
that ends them) must be identical word for word: under the twins on and off, EVOGP_TC_END 0 and 1, the fold levels 0, 1 and 2, the division
modes short and ieee (reciprocal columns on and off), batches of 8 and 32 trees, 64 and 512 rows.
Both are held against the one-tree-per-pass compiler (evogp_hip_debug_compile_batch(0)) as well.  That compiler writes neither END_LEAN / LEAF_*
nor NAN_TREE and hands "no function" trees on, so the programs are compared word for word where the vocabularies agree -- EVOGP_TC_END 0 and
fold level 0, trees without such a node -- and the FITNESS words in every setting and for every tree.

Fitness words, table against selects and both against the CPU oracle: 2000 trees of the headline's generator at 1024 and at 200 rows."""
import ctypes
import json
import os

import numpy as np
import pytest

from helpers import ARITH, assert_close_classes, depth2leaf, roulette_uniform

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_VAR, T_CONST, T_UFUNC, T_BFUNC = 0, 1, 2, 3
ADD, SUB, MUL, DIV = 1, 2, 3, 4
NOFN = 29
VARS = 6
MASK = sum(1 << f for f in ARITH)
CONSTS = [0.0, -0.0, 1.0, -1.0, 2.0, 0.5, float(np.float32(2.0) ** -126), 1e-40, float("inf"), float("nan")]
MAXW = 40


@pytest.fixture(scope="module")
def g():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import gpu_capi

    return gpu_capi


# ---- the crafted forest: expressions ('v', k) / ('c', x) / ('b', op, left, right) / ('u', id, operand) -> prefix rows ----
def V(k):
    return ("v", k % VARS)


def C(x):
    return ("c", x)


def Bn(op, a, b):
    return ("b", op, a, b)


def flat(e):
    if e[0] == "v":
        return [(T_VAR, float(e[1]), 1)]
    if e[0] == "c":
        return [(T_CONST, e[1], 1)]
    if e[0] == "u":
        a = flat(e[2])
        return [(T_UFUNC, float(e[1]), 1 + len(a))] + a
    a, b = flat(e[2]), flat(e[3])
    return [(T_BFUNC, float(e[1]), 1 + len(a) + len(b))] + a + b


def sized(n, r):
    """an expression of exactly n nodes (n odd) over + - * /, leaves variables and the constants"""
    if n == 1:
        return V(int(r.integers(VARS))) if r.random() < 0.6 else C(CONSTS[int(r.integers(len(CONSTS)))])
    left = 1 + 2 * int(r.integers((n - 1) // 2))
    return Bn(int(r.integers(ADD, DIV + 1)), sized(left, r), sized(n - 1 - left, r))


def operand(kind, i, c):
    return {"V": V(i), "C": C(c), "S": Bn(MUL, V(i + 1), V(i + 2)), "A": Bn(ADD, C(c), C(2.0))}[kind]


def crafted_forest():
    r = np.random.default_rng(2024)
    trees = []
    n = 0
    for op in (ADD, SUB, MUL, DIV):
        for lk in "VCSA":
            for rk in "VCSA":
                for ci, c in enumerate(CONSTS if "C" in (lk, rk) or "A" in (lk, rk) else [1.0]):
                    node = Bn(op, operand(lk, n, c), operand(rk, n + 3, CONSTS[(ci + 3) % len(CONSTS)] if lk in "CA" and rk in "CA" else c))
                    n += 1
                    trees += [node, Bn(ADD, node, V(n)), Bn(MUL, V(n), node), Bn(DIV, Bn(SUB, V(n), node), node)]
    # "no function" over a variable, a constant, a function on the stack, a function folded to a constant; as root and as an operand
    for i, a in enumerate([V(1), C(2.0), C(float("nan")), Bn(ADD, V(0), V(1)), Bn(MUL, C(2.0), C(0.5)), Bn(DIV, V(2), C(0.0))]):
        u = ("u", NOFN, a)
        trees += [u, Bn(ADD, u, V(i)), Bn(DIV, V(i), u), Bn(MUL, Bn(SUB, u, C(1.0)), u), ("u", NOFN, u)]
    # the in-place divisions S / S, S / c, c / S under h operands on the stack (the right operand of a node runs first and waits)
    s = lambda i: Bn(MUL, V(i), V(i + 1))   # noqa: E731
    for d in (lambda i: Bn(DIV, s(i), s(i + 2)), lambda i: Bn(DIV, s(i), C(3.0)), lambda i: Bn(DIV, C(3.0), s(i))):
        for h in range(0, 11):
            e = d(h)
            for k in range(h):
                e = Bn((ADD, SUB, MUL)[k % 3], e, s(k))
            if len(flat(e)) <= 64:
                trees.append(e)
    rows = [flat(e) for e in trees]
    rows.append(None)   # a row without a tree
    rows += [flat(sized(int(r.choice([3, 5, 7, 9, 11, 13, 15])), r)) for _ in range(-len(rows) % 32)]
    # whole batches of 32 (and so of 8): 61 nodes -- one tree per pass; 63 + 1 and 33 + 31 -- two, the second ends on lane 63;
    # 21 + 21 + 21 -- three; 43 + 11 + 9 + 1 -- four, the last ends on lane 63
    for sizes in ([61] * 32, [63, 1] * 16, [33, 31] * 16, [21] * 32, [43, 11, 9, 1] * 8):
        rows += [flat(sized(k, r)) for k in sizes]
    pop, L = len(rows), 64
    v = np.zeros((pop, L), np.float32); t = np.zeros((pop, L), np.int16); sz = np.zeros((pop, L), np.int16)
    for i, row in enumerate(rows):
        if row is None:
            continue
        assert len(row) <= L and row[0][2] == len(row)
        for j, (ty, val, s_) in enumerate(row):
            t[i, j], v[i, j], sz[i, j] = ty, val, s_
    nofn = ((t == T_UFUNC) & (np.arange(L)[None, :] < np.maximum(sz[:, :1], 1))).any(axis=1)
    return (v, t, sz), nofn


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def dataset(D, nvars):
    def make():
        r = np.random.default_rng(500 + D)
        return r.uniform(-5, 5, (D, nvars)).astype(np.float32), r.uniform(-5, 5, (D, 1)).astype(np.float32)
    return cached(("data", D, nvars), make)


def handler_table():
    return cached("handlers", lambda: {v["id"]: k for k, v in json.load(open(os.path.join(ROOT, "evogp_amd", "lib", "tc_handlers.json")))["K8_short"]["handlers"].items()})


def programs(g, pop):
    """[tuple of words] per tree of the last call, cut behind the word that ends the program"""
    names = handler_table()
    nh = g.L.evogp_hip_debug_tc_nhandlers()
    last = {"end", "skip", "end_lean", "leaf_c", "leaf_v", "nan_tree"}
    buf = (ctypes.c_uint * (2 * MAXW))()
    out = []
    for tree in range(pop):
        n = g.L.evogp_hip_debug_tc_program(tree, buf, MAXW)
        assert n > 0, tree
        w = buf[:2 * n]
        ids = [names[((w[2 * i] & 0xFFFF) >> 8) % nh] for i in range(n)]
        stop = next(i for i in range(n) if ids[i] in last)
        out.append((tuple(w[:2 * stop + 2]), tuple(ids[:stop + 1])))
    return out


def run(g, forest, X, y, table, batch):
    """(fitness words, programs) of one call"""
    try:
        assert g.L.evogp_hip_debug_tc_table(table) == 0 and g.L.evogp_hip_debug_compile_batch(batch) == 0
        w = g.sr_fitness(*forest, X, y, func_mask=MASK).view(np.uint32).copy()
        return w, programs(g, forest[0].shape[0])
    finally:
        assert g.L.evogp_hip_debug_tc_table(-1) == 0 and g.L.evogp_hip_debug_compile_batch(-1) == 0


def first_difference(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        if x[0] != y[0]:
            return f"tree {i}: {x[1]} {[hex(d) for d in x[0]]} against {y[1]} {[hex(d) for d in y[0]]}"
    return None


@pytest.mark.parametrize("batch", [8, 32])
@pytest.mark.parametrize("D", [64, 512])
@pytest.mark.parametrize("division", [2, 0], ids=["short", "ieee"])
def test_program_words(g, division, D, batch):
    forest, nofn = cached("crafted", crafted_forest)
    pop = forest[0].shape[0]
    X, y = dataset(D, VARS)
    seen = set()
    try:
        assert g.L.evogp_hip_set_sr_division(division) == 0
        for twins in (1, 0):
            for end in (1, 0):
                for fold in (2, 1, 0):
                    what = f"division {division} D {D} batch {batch} twins {twins} end {end} fold {fold}"
                    assert g.L.evogp_hip_debug_twins(twins) == 0 and g.L.evogp_hip_debug_tc_end(end) == 0 and g.L.evogp_hip_debug_tc_fold(fold) == 0
                    w1, p1 = run(g, forest, X, y, 1, batch)
                    w0, p0 = run(g, forest, X, y, 0, batch)
                    assert first_difference(p1, p0) is None, f"{what}, table against selects: {first_difference(p1, p0)}"
                    assert np.array_equal(w1, w0), f"{what}: fitness words of trees {np.nonzero(w1 != w0)[0][:5]} differ"
                    wr, pr = cached(("one tree per pass", division, D, twins, end, fold), lambda: run(g, forest, X, y, 0, 0))
                    bad = np.nonzero(w1 != wr)[0]
                    assert len(bad) == 0, f"{what}: fitness words of trees {bad[:5]} differ from the one-tree-per-pass compiler's"
                    if end == 0 and fold == 0:
                        keep = [i for i in range(pop) if not nofn[i]]
                        d = first_difference([p1[i] for i in keep], [pr[i] for i in keep])
                        assert d is None, f"{what}, table against one tree per pass (tree = position among the trees without 'no function'): {d}"
                    for prog in p1:
                        seen.update(prog[1])
    finally:
        assert g.L.evogp_hip_set_sr_division(2) == 0
        assert g.L.evogp_hip_debug_twins(-1) == 0 and g.L.evogp_hip_debug_tc_end(-1) == 0 and g.L.evogp_hip_debug_tc_fold(-1) == 0
    # the forest reaches what it is meant to reach
    need = {f"{o}_{f}" for o in ("add", "sub", "mul", "div") for f in ("SS", "SV", "VS", "SC", "CS", "VV", "VC", "CV")} - ({"div_SV", "div_VV", "div_CV"} if division else set())
    if D <= 64:   # (one row per lane: the stack is deep enough for every in-place division the forest holds)
        need -= {"div_SS", "div_SC", "div_CS"}
    need |= {"push_c", "gun_S", "skip", "nan_tree", "end", "end_lean", "leaf_c", "leaf_v", "divip_SS", "divip_SC", "divip_CS", "add_SS_np", "push_c_np", "divip_SS_np"}
    if division:
        need |= {"divr_SV", "divr_VV", "divr_CV", "divr_SV_np"}
    assert need <= seen, f"division {division} D {D}: no word with {sorted(need - seen)}"


def headline_forest(oracle):
    return cached("headline", lambda: oracle.generate(2000, 64, 10, 1, 0.5, 0.5, [42, 0], depth2leaf(6), roulette_uniform(ARITH), [-1.0, 0.0, 1.0]))


@pytest.mark.parametrize("D", [1024, 200])
def test_fitness_words(g, oracle, D):
    forest = headline_forest(oracle)
    X, y = dataset(D, 10)
    words = []
    try:
        for table in (1, 0):
            assert g.L.evogp_hip_debug_tc_table(table) == 0
            words.append(g.sr_fitness(*forest, X, y, func_mask=MASK).view(np.uint32).copy())
    finally:
        assert g.L.evogp_hip_debug_tc_table(-1) == 0
    diff = np.nonzero(words[0] != words[1])[0]
    assert len(diff) == 0, f"D={D}: {len(diff)} fitness words differ, first trees {diff[:5]}"
    want = cached(("want", D), lambda: oracle.sr_fitness(*forest, X, y, True))
    assert_close_classes(words[0].view(np.float32), want, 1e-5, what=f"D={D}, table")
    assert_close_classes(words[1].view(np.float32), want, 1e-5, what=f"D={D}, selects")
