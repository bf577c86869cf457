"""CPU: the numpy restatement of multi-gene SR fitness (tests/gene_ref.py) against numpy.linalg.lstsq and hand cases.

The lstsq runs on centred, unit-variance columns with rcond = 2^-15 = sqrt(TAU): it cuts singular directions, the restatement drops
genes, and on a tree without a borderline pivot the two leave out the same float32-noise directions up to their weight in the loss,
which the 1e-6 Syy/D margin covers (the issue measured 1.1e-7 Syy/D at worst over 3347 trees)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gene_ref as GR  # noqa: E402
import sr_grad_ref as R  # noqa: E402
from grad_trees import ALL_FUNCS, ARITH, out_word, random_forest  # noqa: E402
from subtree_ref import live_len, well_formed  # noqa: E402

B, U, V, C, OUT = R.T_BFUNC, R.T_UFUNC, R.T_VAR, R.T_CONST, 0x80


def _outputs(oracle, value, type_, size, X, G):
    bad = np.array([not well_formed(type_[r] & 0x7F if G > 1 else type_[r], live_len(size[r], value.shape[1])) for r in range(value.shape[0])])
    v, t, s = value.copy(), type_.copy(), size.copy()
    v[bad, 0], t[bad, 0], s[bad, 0] = 0.0, C, 1
    P = oracle.batch_evaluate(v, t, s, X, G).copy()
    P[bad] = np.nan
    return P


def _lstsq_loss(g, y):
    """mean squared residual of the truncated least-squares fit of the centred labels on the centred, unit-variance genes"""
    g = g.astype(np.float64)
    D = g.shape[0]
    v = y - y.mean()
    gc = g - g.mean(0)
    sd = np.sqrt((gc * gc).mean(0))
    keep = (g.min(0) != g.max(0)) & (sd > 0) & (D > 1)
    if not keep.any():
        return float((v * v).mean())
    Z = gc[:, keep] / sd[keep]
    w = np.linalg.lstsq(Z, v, rcond=2.0 ** -15)[0]
    r = v - Z @ w
    return float((r * r).mean())


@pytest.mark.parametrize("D", [300, 1100])
@pytest.mark.parametrize("G", [2, 4, 8])
@pytest.mark.parametrize("funcs", ["arith", "all"])
def test_restatement_matches_truncated_lstsq(rng, oracle, funcs, G, D):
    pop = 120
    value, type_, size = random_forest(rng, pop, 64, ARITH if funcs == "arith" else ALL_FUNCS, 3, G, max_depth=5)
    size[5, 0] = 0   # a malformed row
    X = rng.uniform(0.5, 1.5, (D, 3)).astype(np.float32)
    y = (1.5 * X[:, 0] ** 2 - X[:, 2] + 0.3 * X[:, 1]).astype(np.float32)
    Gv = _outputs(oracle, value, type_, size, X, G)
    ref = GR.fit(Gv, y)
    finite_in = np.isfinite(Gv).all(axis=(1, 2))
    assert np.array_equal(np.isnan(ref["loss"]), ~finite_in) and np.isnan(ref["loss"][5])   # (no float32 overflow of a weight in these forests)
    assert np.array_equal(np.isnan(ref["coef"]).any(1), ~finite_in)
    border = GR.borderline(ref["ratio"])
    finite = np.flatnonzero(finite_in)
    assert len(finite) >= pop // 3
    share = border[finite].sum() / len(finite)
    worst = 0.0
    y64 = y.astype(np.float64)
    for t in finite:
        if border[t]:
            continue
        gap = abs(ref["loss"][t] - _lstsq_loss(Gv[t], y64))
        worst = max(worst, gap / ref["syy_D"])
        assert gap <= 1e-6 * ref["syy_D"], (t, ref["loss"][t], gap / ref["syy_D"], ref["ratio"][t])
    print(f"{funcs} G{G} D{D}: {len(finite)} finite trees, {share:.1%} borderline, worst |loss - lstsq| / (Syy/D) {worst:.3g}")
    assert share <= 0.02


# ---- hand cases ---------------------------------------------------------------------------------------------------------------------
def _genes(*cols):
    return np.stack([np.asarray(c, np.float32) for c in cols], axis=1)[None]   # (1, D, G)


@pytest.fixture
def cols(rng):
    D = 200
    return rng.uniform(-1, 1, D).astype(np.float32), rng.uniform(-1, 1, D).astype(np.float32)


def test_exact_linear_model(cols):
    g0, g1 = cols
    y = 2.0 * g0.astype(np.float64) - 3.0 * g1.astype(np.float64) + 1.0
    ref = GR.fit(_genes(g0, g1), y)
    assert np.allclose(ref["coef"][0], [1.0, 2.0, -3.0], rtol=1e-12, atol=1e-12) and ref["loss"][0] <= 1e-24 * ref["syy_D"] + 1e-28
    assert ref["kept"][0].all()


def test_identical_and_doubled_genes_are_dropped(cols):
    g0, _ = cols
    y = np.sin(3 * g0.astype(np.float64)) + 0.2
    one = GR.fit(_genes(g0), y)
    for second in (g0, g0 + g0):   # bit-identical, and exactly twice (the sum is exact in float32)
        two = GR.fit(_genes(g0, second), y)
        assert two["coef"][0, 2] == 0.0 and not two["kept"][0, 1] and two["kept"][0, 0]
        # (numpy sums a (D, 1) and a (D, 2) block in different orders: equal up to the float64 order of summation, D 2^-53)
        for got, want in ((two["loss"][0], one["loss"][0]), (two["coef"][0, 1], one["coef"][0, 1]), (two["coef"][0, 0], one["coef"][0, 0])):
            assert abs(got - want) <= 200 * 2.0 ** -53 * max(abs(want), one["syy_D"]), (got, want)


def test_constant_gene_no_gene_and_one_row(cols):
    g0, g1 = cols
    y = (g0 * 0.5 - 0.1).astype(np.float64)
    ref = GR.fit(_genes(np.full_like(g0, 3.25), g0), y)
    assert ref["coef"][0, 1] == 0.0 and ref["kept"][0].tolist() == [False, True] and np.isnan(ref["ratio"][0, 0])
    # no gene at all (a tree without an OUT node evaluates to zeros): the mean model
    none = GR.fit(_genes(np.zeros_like(g0), np.zeros_like(g0)), y)
    assert none["coef"][0].tolist() == [none["ybar"], 0.0, 0.0] and none["loss"][0] == none["syy_D"]
    # D == 1: every gene is flat, the loss is Syy/D = 0
    single = GR.fit(_genes(g0[:1], g1[:1]), y[:1])
    assert single["coef"][0].tolist() == [y[0], 0.0, 0.0] and single["loss"][0] == 0.0


def test_nan_gene_poisons_the_tree(cols):
    g0, g1 = cols
    g1 = g1.copy()
    g1[17] = np.nan
    ref = GR.fit(_genes(g0, g1), g0.astype(np.float64))
    assert np.isnan(ref["loss"][0]) and np.isnan(ref["coef"][0]).all()
    g1[17] = np.inf
    assert np.isnan(GR.fit(_genes(g0, g1), g0.astype(np.float64))["loss"][0])


def test_trees_without_out_nodes_and_with_an_index_past_G(rng, oracle):
    """through the evaluator: a tree with no OUT node has all-zero genes, and an OUT index >= G is ignored"""
    G, L, D = 2, 16, 50
    value, type_, size = np.zeros((3, L), np.float32), np.zeros((3, L), np.int16), np.zeros((3, L), np.int16)

    def plant(t, nodes):
        for i, (v, ty, s) in enumerate(nodes):
            value[t, i], type_[t, i], size[t, i] = v, ty, s

    plant(0, [(R.F_ADD, B, 3), (0, V, 1), (1, V, 1)])                                   # no OUT node
    plant(1, [(out_word(R.F_ADD, 5), B | OUT, 3), (0, V, 1), (1, V, 1)])                # OUT index 5 >= G: ignored
    plant(2, [(out_word(R.F_MUL, 1), B | OUT, 3), (0, V, 1), (1, V, 1)])                # gene 1 = x0 * x1
    X = rng.uniform(0.5, 1.5, (D, 2)).astype(np.float32)
    y = (X[:, 0] * X[:, 1]).astype(np.float32)
    Gv = _outputs(oracle, value, type_, size, X, G)
    assert not Gv[0].any() and not Gv[1].any() and np.array_equal(Gv[2, :, 1], X[:, 0] * X[:, 1]) and not Gv[2, :, 0].any()
    ref = GR.fit(Gv, y)
    for t in (0, 1):
        assert ref["coef"][t].tolist() == [ref["ybar"], 0.0, 0.0] and ref["loss"][t] == ref["syy_D"]
    assert ref["coef"][2, 1] == 0.0 and abs(ref["coef"][2, 2] - 1.0) <= 1e-12 and ref["loss"][2] <= 1e-20


def test_pack_and_from_packed_round_trip(cols):
    g0, g1 = cols
    y = g0.astype(np.float64) - g1
    mom = GR.moments(_genes(g0, g1, g0 * g1), y)
    packed = GR.pack(mom["mean"], mom["C"], mom["c"])
    assert packed.shape == (1, GR.n_moments(3))
    back = GR.from_packed(packed, 3, mom["mn"], mom["mx"], mom["bad"], mom["ybar"], mom["syy_D"], mom["D"])
    for k in ("mean", "C", "c"):
        assert np.array_equal(back[k], mom[k])
    assert np.array_equal(GR.solve(back)["coef"], GR.solve(mom)["coef"])
