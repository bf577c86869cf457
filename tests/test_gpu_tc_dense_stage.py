"""GPU: the dense compiler's staged node stage (evogp_amd/csrc/sr_tc.hip tc_compile_dense_kernel) changes no record.

The node stage reads the rows of `type` and `size` eight bytes per lane -- four nodes per lane, four trees per wave step --, ranks the function
nodes inside their tree's 16 lanes and leaves one meta byte per node (size - 1, class) in LDS, from which the dense passes take the types and
sizes of a lane's node and of both its children.  tc_compile_packed_kernel<B, 0, false, true> (evogp_hip_debug_tc_dense 0) is the truth:
every case compares program words, sentinels (the fitness words) and what the marks cause bit for bit between the two, and every case asserts
evogp_hip_debug_tc_dense_fallbacks() -- the batches the dense kernel handed to the packed passes, -1 where the launch was not the dense
kernel's -- so that no comparison passes because everything fell back.

1. every tree shape the four-trees-per-step stage can get wrong: left combs, right combs and balanced trees of every odd length 1 .. 63, each
   at every position of its load group of four; function nodes at every node index a 63-node row can hold one at (0 .. 60: a function node's
   two children follow it); a 63-node tree among three one-leaf trees.  Clean forests: no fallback.
2. ragged batches: 1 .. 129 trees under batches of 8, 16 and 32 -- last groups of 1 .. 3 trees, short last batches.
3. dead words: forest_invariance's stale tails, and a binary function with a large size as the first dead node (always in the 8-byte group of
   the last live one: lengths are odd): same words as the clean forest, no fallback.
4. rows handed on (first-node sizes, inner sizes that lie, types the line does not take, the "no function" node), one per batch and at every
   position of a load group: packed's records, and as many fallbacks as there are batches with such a row.
5. row lengths and alignment: gp_len a multiple of four runs the dense kernel, any other the packed one (-1); a view that starts at an odd tree
   is aligned with gp_len 4 and not with gp_len 6.
6. fitness words of 2000 generated trees against packed, the CPU oracle and the calls on the halves, at 64 and 1000 rows, in the three
   division modes (variables in [-5, 5) and the constants -1, 0, 1 over at most six levels: no quotient leaves FAST's documented range)."""
import numpy as np
import pytest

import test_gpu_tc_dense as D
import test_gpu_tc_table as T
from helpers import assert_close_classes

pytestmark = pytest.mark.gpu
MASK = T.MASK
V, C, Bn, flat = T.V, T.C, T.Bn, T.flat
ADD, SUB, MUL, DIV = T.ADD, T.SUB, T.MUL, T.DIV
g = D.g


def fallbacks(g):
    return g.L.evogp_hip_debug_tc_dense_fallbacks()


def same(g, forest, X, y, what, batch=32, mask=MASK, want_fallbacks=0):
    """dense == packed, programs and fitness words, and the dense launch's fallbacks; -> (words, programs)"""
    w1, p1 = D.run(g, forest, X, y, 1, batch, mask)
    fb = fallbacks(g)
    w0, p0 = D.run(g, forest, X, y, 0, batch, mask)
    assert fallbacks(g) == -1, f"{what}: the packed launch reports fallbacks"
    d = T.first_difference(p1, p0)
    assert d is None, f"{what}, dense against packed: {d}"
    assert np.array_equal(w1, w0), f"{what}: fitness words of trees {np.nonzero(w1 != w0)[0][:5]} differ"
    if want_fallbacks is not None:
        assert fb == want_fallbacks, f"{what}: {fb} batches handed on, expected {want_fallbacks}"
    return w1, p1


# ---- 1. tree shapes ----
def balanced(n, k=0):
    if n == 1:
        return V(k)
    left = ((n - 1) // 2) | 1
    return Bn((ADD, SUB, MUL, DIV)[(n // 2) % 4], balanced(left, k + 1), balanced(n - 1 - left, k + 2))


def zigzag(n_ops):
    """a comb that turns at every level: function nodes at even and odd indices"""
    e = V(0)
    for k in range(n_ops):
        e = Bn((ADD, SUB, MUL)[k % 3], e, V(k + 1)) if k % 2 else Bn((ADD, SUB, MUL)[k % 3], V(k + 1), e)
    return e


def shape_rows():
    r = np.random.default_rng(404)
    fill = [flat(V(1)), flat(Bn(ADD, V(0), C(2.0))), flat(Bn(MUL, Bn(SUB, V(2), V(3)), V(4)))]
    rows = []
    for n_ops in range(0, 32):
        shapes = [D.comb(n_ops, True), D.comb(n_ops, False), balanced(2 * n_ops + 1), zigzag(n_ops), T.sized(2 * n_ops + 1, r)]
        for e in shapes:
            for pos in range(4):
                group = [fill[(n_ops + k) % 3] for k in range(4)]
                group[pos] = flat(e)
                rows += group
    big = flat(T.sized(63, r))
    for pos in range(4):   # a full tree among one-leaf trees
        group = [flat(V(k)) if k % 2 else flat(C(0.5)) for k in range(4)]
        group[pos] = big
        rows += group
    return rows


def test_tree_shapes(g):
    rows = T.cached("stage shapes", shape_rows)
    at = {i for row in rows for i, (ty, _, _) in enumerate(row) if ty == T.T_BFUNC}
    assert at == set(range(61)), f"no function node at indices {sorted(set(range(61)) - at)}"
    assert {len(row) for row in rows} == set(range(1, 64, 2))
    forest = D.rows_to_forest(rows)
    X, y = T.dataset(64, T.VARS)
    for batch in (8, 32):
        _, p = same(g, forest, X, y, f"tree shapes, batch {batch}", batch)
    assert not any(prog[1] == ("skip",) for prog in p)


# ---- 2. ragged batches ----
def mixed_rows(n, seed=11):
    r = np.random.default_rng(seed)
    return [flat(T.sized(int(r.choice([1, 1, 3, 5, 7, 9, 13, 21, 31, 43, 63])), r)) for _ in range(n)]


@pytest.mark.parametrize("batch", [8, 16, 32])
def test_ragged_batches(g, batch):
    rows = T.cached("stage mixed", lambda: mixed_rows(129))
    X, y = T.dataset(64, T.VARS)
    for pop in (1, 2, 3, 4, 5, 31, 32, 33, 63, 65, 127, 129):
        same(g, D.rows_to_forest(rows[-pop:]), X, y, f"{pop} trees, batch {batch}", batch)


# ---- 3. dead words ----
def test_dead_words(g):
    import forest_invariance as FI

    rows = T.cached("stage shapes", shape_rows)[:1200]
    clean = D.rows_to_forest(rows)
    X, y = T.dataset(64, T.VARS)
    _, p_clean = same(g, clean, X, y, "the clean forest")
    sv, st, ss, planted = FI.stale_tails(np.random.default_rng(5), *clean, 1)
    assert planted, "no pattern planted"
    _, p = same(g, (sv, st, ss), X, y, "stale tails")
    d = T.first_difference(p, p_clean)
    assert d is None, f"stale tails changed a program: {d}"
    # the first dead node a binary function with a large size; the other dead words stale as well
    for size in (30000, 64, -1):
        v, t, s = sv.copy(), st.copy(), ss.copy()
        n = s[:, 0].astype(np.int64)
        has = np.nonzero(n < s.shape[1])[0]
        assert len(has) > 1000 and (n[has] % 4 != 0).all()   # (the dead node shares its 8-byte group with the last live one)
        v[has, n[has]], t[has, n[has]], s[has, n[has]] = float(ADD), T.T_BFUNC, size
        _, p = same(g, (v, t, s), X, y, f"a dead binary function of size {size}")
        d = T.first_difference(p, p_clean)
        assert d is None, f"a dead binary function of size {size} changed a program: {d}"


# ---- 4. rows handed on ----
def handed_on_rows():
    base = flat(Bn(ADD, Bn(MUL, Bn(SUB, V(0), C(2.0)), Bn(DIV, V(1), V(2))), Bn(SUB, Bn(ADD, V(3), C(0.5)), Bn(MUL, V(4), V(5)))))
    assert len(base) == 15 and base[1][0] == T.T_BFUNC and base[3][0] != T.T_BFUNC

    def with_size(i, s):
        row = list(base)
        row[i] = (row[i][0], row[i][1], s)
        return row

    def with_type(i, ty):
        row = list(base)
        row[i] = (ty, row[i][1], row[i][2])
        return row

    out = dict(D.bad_rows())
    out.update({
        "first size 0": with_size(0, 0), "first size -1": with_size(0, -1), "first size 14": with_size(0, 14), "first size 65": with_size(0, 65),
        "first size 1000": with_size(0, 1000),
        "function of size 0": with_size(1, 0), "function of size 1": with_size(1, 1), "leaf of size 3 (left)": with_size(3, 3),
        "leaf of size 3 (right)": with_size(4, 3), "function of size 64": with_size(8, 64), "left child of size 64": with_size(9, 64),
        "right child behind the row": with_size(2, 62),
        "type 2": with_type(5, 2), "type 4": with_type(8, 4), "type 0x7F": with_type(3, 0x7F), "type 0x80 | 3": with_type(1, 0x80 | 3),
        "type -1": with_type(14, -1), "type -32768 + 3": with_type(8, -32768 + 3),
    })
    return out


@pytest.mark.parametrize("rot", [0, 1, 2, 3])
def test_rows_handed_on(g, rot):
    X, y = T.dataset(64, T.VARS)
    bad = handed_on_rows()
    batch = 8
    clean_rows = mixed_rows(batch * len(bad), seed=3)
    _, p_clean = same(g, D.rows_to_forest(clean_rows), X, y, "the clean forest", batch)
    rows, at = list(clean_rows), {}
    for i, (name, row) in enumerate(bad.items()):   # one per batch, at every position of a load group and in either group of the batch
        at[name] = batch * i + 4 * ((i >> 2) & 1) + (i + rot) % 4
        rows[at[name]] = row
    w, p = same(g, D.rows_to_forest(rows), X, y, f"one row handed on per batch, rotation {rot}", batch, want_fallbacks=len(bad))
    for name, t in at.items():
        if not name.startswith("no function"):   # (the packed passes compile that node themselves)
            assert p[t][1] == ("skip",), f"'{name}' in row {t}: compiled to {p[t][1]}"
        assert w[t] != D.SENTINEL_HEAVY, f"'{name}' in row {t}: nobody evaluated the tree"
    others = [i for i in range(len(rows)) if i not in at.values()]
    d = T.first_difference([p[i] for i in others], [p_clean[i] for i in others])
    assert d is None, f"a row handed on changed another tree's program (position among the other trees): {d}"
    # a single bad row: one batch
    rows = list(clean_rows)
    rows[batch * 3 + rot] = bad["type 2"]
    same(g, D.rows_to_forest(rows), X, y, "one row handed on", batch, want_fallbacks=1)


# ---- 5. row lengths and alignment ----
def short_rows(L, n=70, seed=21):
    r = np.random.default_rng(seed + L)
    sizes = [k for k in (1, 3, 5, 7, 9, 11, 31, 59, 63) if k <= L]
    return [flat(T.sized(int(r.choice(sizes)), r)) for _ in range(n)]


@pytest.mark.parametrize("L", [4, 8, 12, 32, 60, 64, 3, 5, 6, 7, 10, 63])
def test_row_lengths(g, L):
    X, y = T.dataset(64, T.VARS)
    forest = D.rows_to_forest(short_rows(L), L)
    for batch in (8, 32):
        same(g, forest, X, y, f"gp_len {L}, batch {batch}", batch, want_fallbacks=0 if L % 4 == 0 else -1)


def view_call(g, forest, X, y, start):
    """sr_fitness on the rows from `start` on of the forest's device arrays, in place (no copy: the pointers are the view's)"""
    import torch

    a = [g.dev(forest[0], np.float32), g.dev(forest[1], np.int16), g.dev(forest[2], np.int16), g.dev(X, np.float32), g.dev(y, np.float32)]
    pop, L = forest[0].shape
    fit = torch.full((pop - start,), 12345.0, dtype=torch.float32, device=g.DEV)
    ptr = [x[start:].data_ptr() for x in a[:3]] + [a[3].data_ptr(), a[4].data_ptr()]
    assert ptr[1] == a[1].data_ptr() + 2 * L * start
    rc = g.L.evogp_hip_sr_fitness_hinted(pop - start, X.shape[0], L, X.shape[1], 1, 1, *ptr, fit.data_ptr(), 0, MASK, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, g.L.evogp_hip_error_string(rc)
    torch.cuda.synchronize()
    return fit.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("L,aligned", [(4, True), (6, False)])
def test_views(g, L, aligned):
    X, y = T.dataset(64, T.VARS)
    forest = D.rows_to_forest(short_rows(L), L)
    tail = tuple(a[1:].copy() for a in forest)
    try:
        assert g.L.evogp_hip_debug_tc_dense(0) == 0 and g.L.evogp_hip_debug_tc_table(1) == 0
        w0 = g.sr_fitness(*tail, X, y, func_mask=MASK).view(np.uint32).copy()
        p0 = T.programs(g, tail[0].shape[0])
        assert g.L.evogp_hip_debug_tc_dense(1) == 0
        w1 = view_call(g, forest, X, y, 1)
        fb = fallbacks(g)
        p1 = T.programs(g, tail[0].shape[0])
    finally:
        assert g.L.evogp_hip_debug_tc_dense(-1) == 0 and g.L.evogp_hip_debug_tc_table(-1) == 0
    assert fb == (0 if aligned else -1), f"gp_len {L}, a view from tree 1 on: fallbacks {fb}"
    d = T.first_difference(p1, p0)
    assert d is None, f"gp_len {L}, a view from tree 1 on: {d}"
    assert np.array_equal(w1, w0)


# ---- 6. fitness words ----
def generated_2000(oracle):
    def make():
        parts = [D.generated(oracle, layers) for layers in range(1, 7)]
        return tuple(np.concatenate([p[k][:334] for p in parts])[:2000].copy() for k in range(3))
    return T.cached("stage generated", make)


@pytest.mark.parametrize("rows", [64, 1000])
def test_fitness_words(g, oracle, rows):
    forest = generated_2000(oracle)
    assert forest[0].shape[0] == 2000
    X, y = T.dataset(rows, 10)
    want = T.cached(("stage want", rows), lambda: oracle.sr_fitness(*forest, X, y, True))
    half = 1000
    got = {}
    try:
        for division in (0, 2, 1):
            assert g.L.evogp_hip_set_sr_division(division) == 0
            words = []
            for dense in (1, 0):
                assert g.L.evogp_hip_debug_tc_dense(dense) == 0
                words.append(g.sr_fitness(*forest, X, y, func_mask=MASK).view(np.uint32).copy())
                fb = fallbacks(g)
                assert fb == (0 if dense else -1), f"division {division} rows {rows} dense {dense}: fallbacks {fb}"
            assert g.L.evogp_hip_debug_tc_dense(1) == 0
            halves = np.concatenate([g.sr_fitness(*(a[:half].copy() for a in forest), X, y, func_mask=MASK).view(np.uint32),
                                     g.sr_fitness(*(a[half:].copy() for a in forest), X, y, func_mask=MASK).view(np.uint32)])
            assert fallbacks(g) == 0
            diff = np.nonzero(words[0] != words[1])[0]
            assert len(diff) == 0, f"division {division} rows {rows}: {len(diff)} fitness words differ, first trees {diff[:5]}"
            diff = np.nonzero(words[0] != halves)[0]
            assert len(diff) == 0, f"division {division} rows {rows}: {len(diff)} fitness words of the call differ from its halves', first trees {diff[:5]}"
            got[division] = words[0].view(np.float32)
    finally:
        assert g.L.evogp_hip_set_sr_division(2) == 0 and g.L.evogp_hip_debug_tc_dense(-1) == 0
    for division in (0, 2, 1):
        assert_close_classes(got[division], want, 1e-5, what=f"division {division} rows {rows}, dense")
