"""GPU: settling NaN-proven trees at a batch's start (evogp_amd/csrc/gen/gen_tc_asm.py NANPEEK; sr_tc.hip TcParams::flags bit 15) changes no
fitness word and no program record.

Every case runs twice in one process: with the switch on (evogp_hip_debug_tc_nanpeek(1): a launch whose records may hold NAN_TREE words,
whatever its size, peeks at every record's first dword when a batch starts, gives the trees it finds there their NaN at once and walks the others) and off
(0: every tree is visited and NAN_TREE runs as a handler -- the loop of before).  The fitness WORDS must be identical, both must agree with
the CPU oracle (same NaN / inf classes, rtol 1e-5 on the finite values: helpers.assert_close_classes at the tolerance the other
test_gpu_tc_* files use for + - * /), and the handler histogram -- computed from the records -- must not move.

Small populations draw single trees by default, so a batch loop would never see two trees: the cases also run under the headline launch's
geometry (batches of 8, evogp_hip_debug_tc_batches(8, 0)) and under batches of 64, the widest mask.  The patterns repeat with the batch's
size; a workgroup's pool starts wherever the population's split puts it, so the NaN trees meet every position of a batch."""
import ctypes
import json
import os

import numpy as np
import pytest

from helpers import assert_close_classes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-5
T_VAR, T_CONST, T_UFUNC, T_BFUNC = 0, 1, 2, 3
ADD, SUB, MUL, DIV, SIN = 1, 2, 3, 4, 14
VARS = 10
POPS = (1, 2, 63, 64, 65, 130, 5000)
GEOMETRIES = ((0, -1), (8, 0), (64, 0))   # (trees per batch, shift of the drawn batches): the default, the headline's, the widest mask

V = lambda k: (T_VAR, float(k), 1)      # noqa: E731
C = lambda c: (T_CONST, float(c), 1)    # noqa: E731
B = lambda f, n: (T_BFUNC, float(f), n)  # noqa: E731
# proved NaN by the compiler: x0 / 0, x1 + (0 / 0) (a NaN constant after folding), x0 / (x1 - x1) (the Z rule: fold level 2)
NAN_TREES = [[B(DIV, 3), V(0), C(0.0)],
             [B(ADD, 5), V(1), B(DIV, 3), C(0.0), C(0.0)],
             [B(DIV, 5), V(0), B(SUB, 3), V(1), V(1)]]
# live: arithmetic trees of three and five nodes (a division among them), single leaves
LIVE_TREES = [[B(ADD, 3), V(0), V(1)],
              [B(SUB, 5), B(MUL, 3), V(2), V(3), V(4)],
              [V(5)],
              [B(DIV, 3), V(6), V(7)],
              [B(MUL, 3), V(8), C(0.5)],
              [C(1.25)],
              [B(ADD, 5), V(9), B(DIV, 3), C(2.0), V(3)],
              [B(SUB, 3), C(-1.0), V(2)]]


@pytest.fixture(scope="module")
def g():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import gpu_capi

    yield gpu_capi
    L = gpu_capi.L
    assert L.evogp_hip_debug_tc_nanpeek(-1) == 0 and L.evogp_hip_debug_tc_batches(0, -1) == 0


@pytest.fixture(autouse=True)
def defaults_afterwards(g):
    """the switches of this file are process-wide: whatever a test does, and however it ends, the next test starts from the defaults"""
    yield
    L = g.L
    L.evogp_hip_debug_tc_nanpeek(-1); L.evogp_hip_debug_tc_batches(0, -1); L.evogp_hip_debug_tc_fold(-1)
    L.evogp_hip_debug_twins(-1); L.evogp_hip_debug_tc_end(-1); L.evogp_hip_set_sr_division(2)


def rows_to_forest(trees, L=16):
    pop = len(trees)
    v = np.zeros((pop, L), np.float32); t = np.zeros((pop, L), np.int16); s = np.zeros((pop, L), np.int16)
    for i, tr in enumerate(trees):
        assert len(tr) <= L and tr[0][2] == len(tr), i
        for j, (ty, val, sz) in enumerate(tr):
            t[i, j], v[i, j], s[i, j] = ty, val, sz
    return v, t, s


def nan_mask(pattern, pop, nb):
    i = np.arange(pop)
    m = {"all": np.ones(pop, bool),
         "none": np.zeros(pop, bool),
         "alternating": i % 2 == 0,
         "first of a batch": i % nb == 0,
         "last of a batch": i % nb == nb - 1,
         "one live tree": i % nb != min(2, nb - 1),                 # a single live tree among NaN trees: the second-tree hook at the batch's end
         "two live trees": (i % nb != 0) & (i % nb != nb - 1),      # exactly two, at positions 0 and nb - 1
         "last tree": i == pop - 1}[pattern].copy()
    if pattern == "last tree":
        m[::7] = True   # (and a few more, so that the last one is not the only one its workgroup meets)
        m[pop - 1] = True
    return m


PATTERNS = ("all", "none", "alternating", "first of a batch", "last of a batch", "one live tree", "two live trees", "last tree")
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def forest_of(pattern, pop, nb=8, extra=()):
    def make():
        m = nan_mask(pattern, pop, nb)
        trees = [NAN_TREES[i % len(NAN_TREES)] if m[i] else LIVE_TREES[i % len(LIVE_TREES)] for i in range(pop)]
        for at, tree in extra:
            if at < pop:
                trees[at], m[at] = tree, False
        return rows_to_forest(trees), m
    return cached(("forest", pattern, pop, nb, len(extra)), make)


def dataset(D):
    def make():
        r = np.random.default_rng(2000 + D)
        return r.uniform(-5, 5, (D, VARS)).astype(np.float32), r.uniform(-5, 5, (D, 1)).astype(np.float32)
    return cached(("data", D), make)


def histogram(g, pop):
    import torch

    nh = g.L.evogp_hip_debug_tc_nhandlers()
    hist = torch.zeros(2 * nh, dtype=torch.int64, device=g.DEV)
    rc = g.L.evogp_hip_debug_tc_histogram(pop, ctypes.c_void_p(hist.data_ptr()), 2 * nh, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, g.L.evogp_hip_error_string(rc)
    return hist.cpu().numpy()


def nan_tree_words(g, hist):
    nh = g.L.evogp_hip_debug_tc_nhandlers()
    i = json.load(open(os.path.join(ROOT, "evogp_amd", "lib", "tc_handlers.json")))["K8_short"]["handlers"]["nan_tree"]["id"]
    return int(hist[i] + hist[nh + i])


def on_and_off(g, call, pop):
    """[(words, histogram, flag raised)] with the switch on, then off"""
    out = []
    try:
        for mode in (1, 0):
            assert g.L.evogp_hip_debug_tc_nanpeek(mode) == 0
            w = np.asarray(call()).view(np.uint32).copy()
            out.append((w, histogram(g, pop), g.L.evogp_hip_debug_tc_nanpeek_raised()))
    finally:
        assert g.L.evogp_hip_debug_tc_nanpeek(-1) == 0
    return out


def check(g, oracle, pattern, pop, D, mse=True, geometry=(8, 0), fold=2, forest=None, skip_values=()):
    (forest, m) = forest or forest_of(pattern, pop, geometry[0] or 8)
    X, y = dataset(D)
    what = f"{pattern} pop={pop} D={D} mse={mse} batches={geometry} fold={fold}"
    try:
        assert g.L.evogp_hip_debug_tc_batches(*geometry) == 0
        (w1, h1, f1), (w0, h0, f0) = on_and_off(g, lambda: g.sr_fitness(*forest, X, y, mse), pop)
    finally:
        assert g.L.evogp_hip_debug_tc_batches(0, -1) == 0
    diff = np.nonzero(w1 != w0)[0]
    assert len(diff) == 0, f"{what}: {len(diff)} fitness words differ, first trees {diff[:5]}: {w1[diff[:5]]} against {w0[diff[:5]]}"
    assert np.array_equal(h1, h0), f"{what}: the handler histogram moved"
    assert f0 == 0, f"{what}: the flag is up with the switch off"
    assert f1 == (1 if fold >= 1 else 0), f"{what}: flag {f1}"
    if fold == 0:
        assert nan_tree_words(g, h1) == 0, f"{what}: NAN_TREE words at fold level 0"
    elif fold == 2 and not skip_values:
        assert nan_tree_words(g, h1) == int(m.sum()), f"{what}: {nan_tree_words(g, h1)} NAN_TREE words, {int(m.sum())} such trees"
    want = cached(("want", pattern, pop, D, mse, geometry[0] or 8, len(skip_values)), lambda: oracle.sr_fitness(*forest, X, y, mse))
    keep = np.ones(pop, bool)
    keep[[i for i in skip_values if i < pop]] = False
    for w, name in ((w1, "on"), (w0, "off")):
        got = w.view(np.float32)
        assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}, switch {name}: NaN sets differ from the oracle's"
        assert_close_classes(got[keep], want[keep], RTOL, what=f"{what}, switch {name}")
    assert np.isnan(w1.view(np.float32)[m]).all(), f"{what}: a NaN-proven tree is not NaN"
    return w1


# 64: the 1-row build, 256: the 4-row build, 512 / 1024: one and two tiles of the 8-row build (END_LEAN), 1000: a ragged tile (END)
@pytest.mark.parametrize("D", [64, 256, 512, 1024, 1000])
def test_populations_and_patterns(g, oracle, D):
    for geometry in GEOMETRIES:
        for pop in POPS:
            for pattern in PATTERNS:
                check(g, oracle, pattern, pop, D, geometry=geometry)


@pytest.mark.parametrize("D", [256, 1024, 1000])
def test_mean_absolute_error(g, oracle, D):
    for pop in (65, 5000):
        for pattern in PATTERNS:
            check(g, oracle, pattern, pop, D, mse=False)


@pytest.mark.parametrize("division", [0, 1, 2])   # ieee, fast, short
@pytest.mark.parametrize("twins", [0, 1])
@pytest.mark.parametrize("end", [0, 1])            # the early record fetch lives in END, or in END_LEAN and the leaf handlers
def test_divisions_twins_and_ends(g, oracle, division, twins, end):
    L = g.L
    try:
        assert L.evogp_hip_set_sr_division(division) == 0 and L.evogp_hip_debug_twins(twins) == 0 and L.evogp_hip_debug_tc_end(end) == 0
        for D in (64, 256, 1024):
            for pop in (65, 5000):
                for pattern in ("alternating", "one live tree", "two live trees", "first of a batch", "last tree"):
                    check(g, oracle, pattern, pop, D)
    finally:
        assert L.evogp_hip_set_sr_division(2) == 0 and L.evogp_hip_debug_twins(-1) == 0 and L.evogp_hip_debug_tc_end(-1) == 0


@pytest.mark.parametrize("fold", [0, 1, 2])
def test_fold_levels(g, oracle, fold):
    """level 0: no NAN_TREE word exists and the flag stays down; 1: x0 / (x1 - x1) is a live tree that is NaN in every row; 2: the default"""
    try:
        assert g.L.evogp_hip_debug_tc_fold(fold) == 0
        for D in (256, 1024):
            for pop in (65, 5000):
                for pattern in ("all", "alternating", "one live tree", "two live trees"):
                    check(g, oracle, pattern, pop, D, fold=fold)
    finally:
        assert g.L.evogp_hip_debug_tc_fold(-1) == 0


def test_a_dataset_in_pieces(g, oracle):
    """8192 rows of ten variables run in pieces (flags bits 2 / 3): a NaN must survive the add into the stored word, and the word of a tree
    that bails out at run time (sin of an operand beyond 2^17) must keep its sentinel through the later pieces -- the register kernels then
    evaluate it; their sin of such an operand is not the oracle's to the last digit, so those trees are held to on == off and the NaN sets"""
    bail = [B(ADD, 6), (T_UFUNC, float(SIN), 4), B(MUL, 3), V(0), C(1e6), V(1)]   # sin(x0 * 1e6) + x1
    at = (3, 8, 77, 4001)
    for pop in (65, 5000):
        for pattern in ("alternating", "one live tree", "two live trees", "all"):
            forest = forest_of(pattern, pop, 8, extra=tuple((i, bail) for i in at))
            check(g, oracle, pattern, pop, 8192, forest=forest, skip_values=at)
            check(g, oracle, pattern, pop, 8192, mse=False, forest=forest, skip_values=at)


def test_a_call_is_the_concatenation_of_its_halves(g, oracle):
    """whole against halves with the peek on and with it off, and on against off; the cuts leave ragged last batches"""
    X, y = dataset(1024)
    try:
        assert g.L.evogp_hip_debug_tc_batches(8, 0) == 0
        for pop in (130, 5000):
            for pattern in ("alternating", "one live tree", "last tree"):
                forest, _ = forest_of(pattern, pop)
                words = {}
                for mode in (1, 0):
                    assert g.L.evogp_hip_debug_tc_nanpeek(mode) == 0
                    whole = g.sr_fitness(*forest, X, y).view(np.uint32)
                    assert g.L.evogp_hip_debug_tc_nanpeek_raised() == mode, f"{pattern} pop={pop}: flag with the switch at {mode}"
                    for n in (pop // 2, 3, pop - 11):
                        first = g.sr_fitness(*(a[:n] for a in forest), X, y)
                        assert g.L.evogp_hip_debug_tc_nanpeek_raised() == mode
                        second = g.sr_fitness(*(a[n:] for a in forest), X, y)
                        assert g.L.evogp_hip_debug_tc_nanpeek_raised() == mode
                        halves = np.concatenate([first, second]).view(np.uint32)
                        assert np.array_equal(whole, halves), f"{pattern} pop={pop} cut at {n}, switch {mode}: trees {np.nonzero(whole != halves)[0][:5]} differ from the halves'"
                    words[mode] = whole
                assert np.array_equal(words[1], words[0]), f"{pattern} pop={pop}: trees {np.nonzero(words[1] != words[0])[0][:5]} differ on against off"
    finally:
        assert g.L.evogp_hip_debug_tc_nanpeek(-1) == 0 and g.L.evogp_hip_debug_tc_batches(0, -1) == 0


def test_a_second_stream_beside_the_first(g, oracle):
    """two forests on two streams at once, twice over, with the peek on and with it off: each call's words are those of the call alone,
    and the words with the peek on are those with it off"""
    import torch

    X, y = dataset(1024)
    side = torch.cuda.Stream()

    def launch(dev_args, fit, pop):
        rc = g.L.evogp_hip_sr_fitness(pop, 1024, 16, VARS, 1, 1, *[x.data_ptr() for x in dev_args], fit.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, g.L.evogp_hip_error_string(rc)

    try:
        assert g.L.evogp_hip_debug_tc_batches(8, 0) == 0
        for pattern, other in (("alternating", "one live tree"), ("two live trees", "all")):
            pop = 5000
            (fa, _), (fb, _) = forest_of(pattern, pop), forest_of(other, pop)
            da, db = ([g.dev(f[0], np.float32), g.dev(f[1], np.int16), g.dev(f[2], np.int16), g.dev(X, np.float32), g.dev(y, np.float32)] for f in (fa, fb))
            words = {}
            for mode in (1, 0):
                assert g.L.evogp_hip_debug_tc_nanpeek(mode) == 0
                alone = [g.sr_fitness(*f, X, y).view(np.uint32) for f in (fa, fb)]
                assert g.L.evogp_hip_debug_tc_nanpeek_raised() == mode
                out = [torch.full((pop,), 12345.0, dtype=torch.float32, device=g.DEV) for _ in range(4)]
                torch.cuda.synchronize()
                side.wait_stream(torch.cuda.current_stream())
                for rep in range(2):
                    with torch.cuda.stream(side):
                        launch(db, out[2 * rep + 1], pop)
                        assert g.L.evogp_hip_debug_tc_nanpeek_raised() == mode
                    launch(da, out[2 * rep], pop)
                    assert g.L.evogp_hip_debug_tc_nanpeek_raised() == mode
                torch.cuda.synchronize()
                for rep in range(2):
                    for k in range(2):
                        got = out[2 * rep + k].cpu().numpy().view(np.uint32)
                        assert np.array_equal(got, alone[k]), f"{(pattern, other)[k]}, call {rep} beside another stream, switch {mode}: trees {np.nonzero(got != alone[k])[0][:5]} differ"
                words[mode] = alone
            for k in range(2):
                assert np.array_equal(words[1][k], words[0][k]), f"{(pattern, other)[k]}: trees differ on against off"
    finally:
        assert g.L.evogp_hip_debug_tc_nanpeek(-1) == 0 and g.L.evogp_hip_debug_tc_batches(0, -1) == 0


def test_small_launches_do_not_peek_by_default(g, oracle):
    """left to itself (-1) a launch raises the flag from 900 trees per CU on: below that its batches are of one or two trees"""
    (forest, m), (X, y) = forest_of("alternating", 5000), dataset(1024)
    assert g.L.evogp_hip_debug_tc_nanpeek(-1) == 0
    w = g.sr_fitness(*forest, X, y)
    assert g.L.evogp_hip_debug_tc_nanpeek_raised() == int(os.environ.get("EVOGP_TC_NANPEEK", "1") == "2")
    assert np.array_equal(np.isnan(w), m)


def test_modes_are_checked(g):
    L = g.L
    assert L.evogp_hip_debug_tc_nanpeek(2) != 0 and L.evogp_hip_debug_tc_nanpeek(-2) != 0 and L.evogp_hip_debug_tc_nanpeek(-1) == 0
    assert L.evogp_hip_debug_tc_batches(65, 0) != 0 and L.evogp_hip_debug_tc_batches(8, 4) != 0 and L.evogp_hip_debug_tc_batches(0, -1) == 0
