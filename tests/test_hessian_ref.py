"""CPU: the hyper-dual restatement (tests/hessian_ref.py) against a central difference of the first-order restatement, and the floors
of the forests the GPU tests (tests/test_gpu_hessian.py) compare on.

  * on a table of hand-built trees -- one per function family, IF, max / min, a nested pow, a variable that occurs twice -- the float64
    second derivative agrees with the central difference in x_b of input_grad_ref.forest_xgrad's d / dx_a, step 1e-5 max(1, |x|), within
    1e-6 (1 + |value|): the truncation error of the difference, far above float64 rounding;
  * ``gpu_case``: the two forests of forest_invariance (the arithmetic one with two more data columns no tree reads, so that eight distinct
    pairs exist over its three variables) and their float64 / float32 references, computed once at 130 rows; a test on fewer rows takes
    the first D.  The floors are asserted here, on the reference alone: "comparable" = finite in the float64 and the float32 run."""
import functools

import numpy as np
import pytest

import forest_invariance as FI
import hessian_ref as H
import input_grad_ref as XR
import sr_grad_ref as R
from interval_cases import B, C, IF, U, V, rows

x0, x1, x2 = V(0), V(1), V(2)
x01 = B(R.F_MUL, x0, x1)
TABLE = {
    "arith": B(R.F_SUB, B(R.F_ADD, x01, B(R.F_DIV, x0, x1)), B(R.F_MUL, x0, x0)),
    "twice": B(R.F_ADD, B(R.F_MUL, x0, B(R.F_MUL, x0, x0)), x01),
    "trig": B(R.F_ADD, U(R.F_SIN, x01), B(R.F_MUL, U(R.F_COS, x0), U(R.F_TAN, B(R.F_MUL, C(0.5), x1)))),
    "hyperbolic": B(R.F_ADD, U(R.F_TANH, x01), B(R.F_MUL, U(R.F_SINH, x0), U(R.F_COSH, x1))),
    "log_exp": B(R.F_MUL, U(R.F_LOG, B(R.F_ADD, x01, C(1.0))), U(R.F_EXP, B(R.F_SUB, x0, x1))),
    "inv_sqrt": B(R.F_ADD, U(R.F_INV, B(R.F_ADD, B(R.F_MUL, x0, x0), x1)), U(R.F_SQRT, x01)),
    "loose": B(R.F_ADD, B(R.F_LOOSE_DIV, U(R.F_LOOSE_SQRT, x01), U(R.F_LOOSE_LOG, B(R.F_ADD, x0, C(2.0)))), U(R.F_LOOSE_INV, B(R.F_SUB, x01, C(3.0)))),
    "abs_neg": U(R.F_ABS, U(R.F_NEG, B(R.F_MUL, x01, x0))),
    "if": IF(B(R.F_SUB, x2, C(1.0)), B(R.F_MUL, x01, x0), B(R.F_MUL, x01, x1)),
    "max_min": B(R.F_MIN, B(R.F_MAX, B(R.F_MUL, x01, x0), C(-5.0)), B(R.F_ADD, C(50.0), x01)),
    "nested_pow": B(R.F_POW, B(R.F_POW, x0, x1), B(R.F_ADD, x0, C(0.5))),
    "loose_pow": B(R.F_LOOSE_POW, B(R.F_SUB, x01, C(3.0)), x1),
}
PAIRS3 = [(0, 0), (0, 1), (1, 1)]


@pytest.mark.parametrize("name", sorted(TABLE))
def test_restatement_agrees_with_a_central_difference(name):
    forest = rows([TABLE[name]], 32)
    X = np.random.default_rng(7).uniform(0.5, 1.5, (40, 3))
    _, h = H.forest_hessian(*forest, X, PAIRS3)
    _, h32 = H.forest_hessian(*forest, X.astype(np.float32), PAIRS3, np.float32)
    assert np.isfinite(h).all() and np.isfinite(h32).all(), f"{name}: an entry of the table is not comparable"
    for k, (a, b) in enumerate(PAIRS3):
        step = 1e-5 * np.maximum(1.0, np.abs(X[:, b]))
        up, down = X.copy(), X.copy()
        up[:, b] += step
        down[:, b] -= step
        fd = (XR.forest_xgrad(*forest, up, [a])[1][0, 0] - XR.forest_xgrad(*forest, down, [a])[1][0, 0]) / (up[:, b] - down[:, b])
        err = np.abs(h[k, 0] - fd)
        assert (err <= 1e-6 * (1 + np.abs(fd))).all(), f"{name} pair {(a, b)}: {h[k, 0][err.argmax()]!r} against the difference {fd[err.argmax()]!r}"


GPU_CASES = {
    # name: (forest_invariance case, trees, pairs of eight, the floor of its comparable share)
    "arith": ("arith_L64", 48, [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2), (0, 4), (3, 3)], 0.5),
    "all": ("all_L1024_v40", 24, [(0, 0), (0, 1), (1, 1), (2, 39), (39, 39), (5, 17), (3, 3), (0, 39)], 0.2),
}
GPU_ROWS = 130


@functools.lru_cache(maxsize=None)
def gpu_case(name):
    """``(forest, X (130, var_len) float32, y, pairs, ref64 (pred, h), ref32 (pred, h), comparable (8, pop, 130))``"""
    case_name, pop, pairs, _ = GPU_CASES[name]
    c = FI.build_case(case_name, pop, GPU_ROWS)
    X, y = c.shared["X"], c.shared["y"]
    if name == "arith":   # two columns no tree reads: pairs that every tree lacks, and room for eight distinct pairs
        X = np.concatenate([X, np.random.default_rng(5).uniform(0.5, 1.5, (GPU_ROWS, 2)).astype(np.float32)], 1)
    ref64 = H.forest_hessian(*c.forest, X, pairs)
    ref32 = H.forest_hessian(*c.forest, X, pairs, np.float32)
    ok = np.isfinite(ref64[1]) & np.isfinite(ref32[1]) & np.isfinite(ref64[0])[None] & np.isfinite(ref32[0])[None]
    return c.forest, np.ascontiguousarray(X), y, pairs, ref64, ref32, ok


@pytest.mark.parametrize("name", sorted(GPU_CASES))
def test_the_gpu_forests_meet_their_floor(name):
    ok = gpu_case(name)[6]
    share = ok.mean()
    print(f"{name}: {share:.3f} of the {ok.size} (pair, tree, row) entries are comparable")
    assert share >= GPU_CASES[name][3]
