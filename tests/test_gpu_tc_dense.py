"""GPU: the dense arithmetic compiler (evogp_amd/csrc/sr_tc.hip tc_compile_dense_kernel; evogp_hip_debug_tc_dense) changes no record.

tc_compile_dense_kernel gives a lane to every FUNCTION node only and reads leaves from the row; tc_compile_packed_kernel<B, 0, false, true>
gives a lane to every node and is the truth here.  Everything is compared bit for bit between the two (evogp_hip_debug_tc_dense 1 / 0):

Program words (evogp_hip_debug_tc_program, cut at the word that ends the program): the crafted forest of test_gpu_tc_table.py (batches of 8
and 32 trees in every setting, of 16 and 64 in two), and the first
1, 2, 31, 32, 33, 64, 65 and 5000 trees of oracle-generated forests with max_layer_cnt 1 .. 6 (batches of 32, the headline's), each under
twins on / off x EVOGP_TC_END 1 / 0 x the fold levels 0 / 1 / 2 x the three division modes x 64 and 512 rows.

Edge shapes: forests of one-leaf trees only, of none, alternating; a full 63-node tree alone and beside one-leaf trees; a left and a right
comb of 63 nodes over leaves and over products (the left comb over products needs 16 stack entries, more than the interpreter has at 512
rows: handed on, the packed compiler's sentinel); trees whose right child is the
row's last node (rows exactly as long as the tree); the three in-place divisions under every stack height.

Rows the dense line must hand on: sizes that do not describe the tree (too large, zero, negative, past the row, a leaf that is not 1, a root
that is even or above the row), a row without a tree, the generator's "no function" node, a unary function under a mask that promised none,
and tests/forest_invariance.py's arithmetic case with its bad rows and with stale words behind every tree.  The engine has no read-out of the
compiler's marks; what they cause is checked instead: the program is SKIP in both and the call's fitness word -- which the kernels behind the
marks write, and which stays the sentinel 0x7FC0FEED where a mark is missing -- is the same, and every other tree of the forest keeps the
program it has in the forest without the bad row.

Fitness words: dense against packed and both against the CPU oracle on 2000 trees of the headline's generator at 1024 and 1000 rows, and a
call against the calls on its halves."""
import numpy as np
import pytest

import test_gpu_tc_table as T
from helpers import ARITH, assert_close_classes, depth2leaf, roulette_uniform

pytestmark = pytest.mark.gpu
MASK = T.MASK
V, C, Bn, flat = T.V, T.C, T.Bn, T.flat
ADD, SUB, MUL, DIV = T.ADD, T.SUB, T.MUL, T.DIV
SENTINEL_HEAVY = 0x7FC0FEED


@pytest.fixture(scope="module")
def g():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import gpu_capi

    return gpu_capi


def run(g, forest, X, y, dense, batch=32, mask=MASK):
    """(fitness words, programs) of one call with the word table on"""
    try:
        assert g.L.evogp_hip_debug_tc_dense(dense) == 0 and g.L.evogp_hip_debug_tc_table(1) == 0 and g.L.evogp_hip_debug_compile_batch(batch) == 0
        w = g.sr_fitness(*forest, X, y, func_mask=mask).view(np.uint32).copy()
        return w, T.programs(g, forest[0].shape[0])
    finally:
        assert g.L.evogp_hip_debug_tc_dense(-1) == 0 and g.L.evogp_hip_debug_tc_table(-1) == 0 and g.L.evogp_hip_debug_compile_batch(-1) == 0


def same(g, forest, X, y, what, batch=32, mask=MASK):
    """dense == packed, programs and fitness words; -> (words, programs)"""
    w1, p1 = run(g, forest, X, y, 1, batch, mask)
    w0, p0 = run(g, forest, X, y, 0, batch, mask)
    d = T.first_difference(p1, p0)
    assert d is None, f"{what}, dense against packed: {d}"
    assert np.array_equal(w1, w0), f"{what}: fitness words of trees {np.nonzero(w1 != w0)[0][:5]} differ"
    return w1, p1


class settings:
    """every twins x EVOGP_TC_END x fold level under one division mode"""

    def __init__(self, g, division):
        self.g, self.division = g, division

    def __iter__(self):
        g = self.g
        try:
            assert g.L.evogp_hip_set_sr_division(self.division) == 0
            for twins in (1, 0):
                for end in (1, 0):
                    for fold in (2, 1, 0):
                        assert g.L.evogp_hip_debug_twins(twins) == 0 and g.L.evogp_hip_debug_tc_end(end) == 0 and g.L.evogp_hip_debug_tc_fold(fold) == 0
                        yield f"division {self.division} twins {twins} end {end} fold {fold}"
        finally:
            assert g.L.evogp_hip_set_sr_division(2) == 0
            assert g.L.evogp_hip_debug_twins(-1) == 0 and g.L.evogp_hip_debug_tc_end(-1) == 0 and g.L.evogp_hip_debug_tc_fold(-1) == 0


def rows_to_forest(rows, L=64):
    pop = len(rows)
    v = np.zeros((pop, L), np.float32); t = np.zeros((pop, L), np.int16); s = np.zeros((pop, L), np.int16)
    for i, row in enumerate(rows):
        assert len(row) <= L
        for j, (ty, val, sz) in enumerate(row):
            t[i, j], v[i, j], s[i, j] = ty, val, sz
    return v, t, s


# ---- 1. program words ----
@pytest.mark.parametrize("division,D,batch", [(v, D, b) for v in (2, 1, 0) for D in (64, 512) for b in (8, 32)] + [(2, 512, 16), (2, 512, 64), (0, 64, 16), (0, 64, 64)])
def test_program_words_crafted(g, division, D, batch):
    forest, _ = T.cached("crafted", T.crafted_forest)
    X, y = T.dataset(D, T.VARS)
    seen = set()
    for what in settings(g, division):
        _, p = same(g, forest, X, y, f"{what} D {D} batch {batch}", batch)
        for prog in p:
            seen.update(prog[1])
    # the forest reaches the words the dense line has to choose among
    need = {"push_c", "skip", "nan_tree", "end", "end_lean", "leaf_c", "leaf_v", "divip_SS", "divip_SC", "divip_CS", "add_SS_np", "push_c_np", "add_VV", "mul_SC", "sub_CS"}
    assert need <= seen, f"division {division} D {D}: no word with {sorted(need - seen)}"


SIZES = [1, 2, 31, 32, 33, 64, 65, 5000]


def generated(oracle, layers):
    return T.cached(("generated", layers), lambda: oracle.generate(5000, 64, 10, 1, 0.5, 0.5, [42 + layers, 0], depth2leaf(layers), roulette_uniform(ARITH), [-1.0, 0.0, 1.0]))


@pytest.mark.parametrize("layers", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("D", [64, 512])
@pytest.mark.parametrize("division", [2, 1, 0])
def test_program_words_generated(g, oracle, division, D, layers):
    full = generated(oracle, layers)
    X, y = T.dataset(D, 10)
    for what in settings(g, division):
        for n in SIZES:
            same(g, tuple(a[:n].copy() for a in full), X, y, f"{what} D {D} max_layer_cnt {layers}, {n} trees")


# ---- 2. edge shapes ----
def comb(n_ops, left, products=False):
    """a comb of n_ops functions over variables (2 n_ops + 1 nodes), or of n_ops functions over products of two variables (4 n_ops + 3
    nodes).  A leaf is fused into its parent's word, so a comb over leaves needs one stack entry; over products the LEFT comb keeps one
    product waiting per level (a node's right operand runs first): n_ops + 1 entries, the right comb two."""
    arm = (lambda k: Bn(MUL, V(k), V(k + 1))) if products else V
    e = arm(0)
    for k in range(n_ops):
        e = Bn((ADD, SUB, MUL)[k % 3], e, arm(k + 1)) if left else Bn((ADD, SUB, MUL)[k % 3], arm(k + 1), e)
    return e


def edge_forests():
    r = np.random.default_rng(77)
    leaves = [flat(V(i)) if i % 3 else flat(C(T.CONSTS[i % len(T.CONSTS)])) for i in range(70)]
    trees = [flat(T.sized(int(r.choice([3, 5, 9, 13, 21, 31])), r)) for _ in range(70)]
    full = flat(T.sized(63, r))
    s = lambda i: Bn(MUL, V(i), V(i + 1))   # noqa: E731
    inplace = []
    for d in (lambda i: Bn(DIV, s(i), s(i + 2)), lambda i: Bn(DIV, s(i), C(3.0)), lambda i: Bn(DIV, C(3.0), s(i))):
        for h in range(0, 13):
            e = d(h)
            for k in range(h):
                e = Bn((ADD, SUB, MUL)[k % 3], e, s(k))
            if len(flat(e)) <= 64:
                inplace.append(flat(e))
    out = {
        "one leaf each": rows_to_forest(leaves),
        "no one-leaf tree": rows_to_forest(trees),
        "alternating": rows_to_forest([x for pair in zip(leaves, trees) for x in pair]),
        "a 63-node tree alone": rows_to_forest([full]),
        "a 63-node tree beside leaves": rows_to_forest([leaves[0], full] + leaves[1:40] + [full, full]),
        "left comb of 63": rows_to_forest([flat(V(1)), flat(comb(31, True)), trees[0], trees[1]]),
        "right comb of 63": rows_to_forest([trees[0], flat(comb(31, False)), flat(V(1)), trees[1]]),
        "left comb of 63 over products": rows_to_forest([flat(V(1)), flat(comb(15, True, True)), trees[0], trees[1]] + trees[2:40]),
        "right comb of 63 over products": rows_to_forest([trees[0], flat(comb(15, False, True)), flat(V(1)), trees[1]]),
        "in-place divisions": rows_to_forest(inplace),
    }
    # the right child is the row's last node: rows exactly as long as their trees (31 nodes), the root's right operand a leaf or a subtree
    # that ends there
    last = [flat(Bn(int(r.integers(ADD, DIV + 1)), T.sized(29, r), V(i))) for i in range(20)] + [flat(T.sized(31, r)) for _ in range(20)]
    out["right child at the row's end"] = rows_to_forest(last, L=31)
    return out


@pytest.mark.parametrize("D", [64, 512])
def test_edge_shapes(g, D):
    X, y = T.dataset(D, T.VARS)
    forests = T.cached("edges", edge_forests)
    for division in (2, 0):
        for what in settings(g, division):
            for name, forest in forests.items():
                for batch in (8, 32):
                    w, p = same(g, forest, X, y, f"{name}, {what} D {D} batch {batch}", batch)
                    if name == "left comb of 63 over products" and D == 512:   # 16 stack entries against the interpreter's 9 at eight
                        # rows per lane: handed on -- SKIP, and the kernels behind the mark have replaced the sentinel
                        assert p[1][1] == ("skip",) and w[1] != SENTINEL_HEAVY, name


# ---- 3. rows the dense line hands on ----
def bad_rows():
    """name -> row (value, type, size words) that the arithmetic line does not take, each a change to one 15-node tree"""
    base = flat(Bn(ADD, Bn(MUL, Bn(SUB, V(0), C(2.0)), Bn(DIV, V(1), V(2))), Bn(SUB, Bn(ADD, V(3), C(0.5)), Bn(MUL, V(4), V(5)))))
    assert len(base) == 15

    def with_size(i, s):
        row = list(base)
        row[i] = (row[i][0], row[i][1], s)
        return row

    def with_node(i, ty, val):
        row = list(base)
        row[i] = (ty, val, row[i][2])
        return row

    sub = Bn(MUL, Bn(SUB, V(0), C(2.0)), Bn(DIV, V(1), V(2)))
    out = {
        "inner size too large": with_size(1, 9), "inner size too small": with_size(1, 5), "inner size zero": with_size(8, 0),
        "inner size negative": with_size(8, -3), "left size past the row": with_size(1, 69), "left size past the tree": with_size(9, 13),
        "leaf of size 3": with_size(3, 3), "leaf of size 0": with_size(14, 0), "last leaf of size 40": with_size(14, 40),
        "root even": with_size(0, 16), "root too large": with_size(0, 17), "root above the row": with_size(0, 65),
        "no tree (0)": with_size(0, 0), "no tree (-2)": with_size(0, -2),
        "leaf where the root should be": with_node(0, T.T_VAR, 1.0),
        # well-formed trees with a node that is not the arithmetic line's
        "no function": flat(Bn(ADD, ("u", T.NOFN, sub), V(3))), "no function at the root": flat(("u", T.NOFN, sub)),
        "no function of a leaf": flat(Bn(ADD, sub, ("u", T.NOFN, V(3)))),
        "unary function": flat(Bn(ADD, ("u", 14, sub), V(3))), "unary function at the root": flat(("u", 25, Bn(ADD, V(0), V(1)))),
        "binary function not + - * /": flat(Bn(8, sub, V(3))),
    }
    return out


def test_handed_on_rows(g):
    X, y = T.dataset(64, T.VARS)
    r = np.random.default_rng(9)
    clean_rows = [flat(T.sized(int(r.choice([1, 3, 5, 9, 13])), r)) for _ in range(70)]
    clean = rows_to_forest(clean_rows)
    _, p_clean = same(g, clean, X, y, "the clean forest")
    for at in (0, 5, 31, 32, 69):
        for name, row in bad_rows().items():
            rows = list(clean_rows)
            rows[at] = row
            forest = rows_to_forest(rows)
            w, p = same(g, forest, X, y, f"'{name}' in row {at}")
            if name.startswith("no function"):   # (the packed passes compile the node themselves, gun_S / push_c: the batch is theirs)
                assert "skip" not in p[at][1], f"'{name}' in row {at}: compiled to {p[at][1]}"
            else:
                assert p[at][1] == ("skip",), f"'{name}' in row {at}: compiled to {p[at][1]}"
            assert w[at] != SENTINEL_HEAVY, f"'{name}' in row {at}: nobody evaluated the tree"
            others = [i for i in range(len(rows)) if i != at]
            d = T.first_difference([p[i] for i in others], [p_clean[i] for i in others])
            assert d is None, f"'{name}' in row {at} changed another tree's program (position among the other trees): {d}"


@pytest.mark.parametrize("which", ["forest", "stale"])
def test_invariance_case_rows(g, which):
    import forest_invariance as FI

    c = FI.build_case("arith_L64")
    forest = getattr(c, which)
    w, _ = same(g, forest, c.shared["X"], c.shared["y"], f"forest_invariance arith_L64 {which}", mask=c.func_mask)
    assert not (w == SENTINEL_HEAVY).any()
    wz, _ = same(g, c.forest, c.shared["X"], c.shared["y"], "forest_invariance arith_L64 forest", mask=c.func_mask)
    assert np.array_equal(w, wz), "words behind the trees changed a fitness word"


# ---- 4. fitness words ----
@pytest.mark.parametrize("D", [1024, 1000])
def test_fitness_words(g, oracle, D):
    forest = T.headline_forest(oracle)
    X, y = T.dataset(D, 10)
    words = []
    try:
        for dense in (1, 0):
            assert g.L.evogp_hip_debug_tc_dense(dense) == 0
            words.append(g.sr_fitness(*forest, X, y, func_mask=MASK).view(np.uint32).copy())
        assert g.L.evogp_hip_debug_tc_dense(1) == 0
        half = forest[0].shape[0] // 2
        halves = np.concatenate([g.sr_fitness(*(a[:half].copy() for a in forest), X, y, func_mask=MASK).view(np.uint32),
                                 g.sr_fitness(*(a[half:].copy() for a in forest), X, y, func_mask=MASK).view(np.uint32)])
    finally:
        assert g.L.evogp_hip_debug_tc_dense(-1) == 0
    diff = np.nonzero(words[0] != words[1])[0]
    assert len(diff) == 0, f"D={D}: {len(diff)} fitness words differ, first trees {diff[:5]}"
    diff = np.nonzero(words[0] != halves)[0]
    assert len(diff) == 0, f"D={D}: {len(diff)} fitness words of the call differ from its halves', first trees {diff[:5]}"
    want = T.cached(("want", D), lambda: oracle.sr_fitness(*forest, X, y, True))
    assert_close_classes(words[0].view(np.float32), want, 1e-5, what=f"D={D}, dense")
    assert_close_classes(words[1].view(np.float32), want, 1e-5, what=f"D={D}, packed")
