"""TEST-ONLY: the cases of the normal-equation comparison (tests/test_gpu_sr_lm.py) and their exclusion rule, in one place so that the
CPU suite can check that the float64 reference alone leaves enough comparable trees for the chosen seeds (tests/test_sr_lm_ref.py)."""
import zlib

import numpy as np

import sr_grad_ref as R
import sr_lm_ref as LM
from grad_trees import ALL_FUNCS, ARITH, random_forest
from helpers import per_tree_tolerance

# (funcs, gp_len, D): 128 is the smallest row on the global tape; 1 / 63 / 65 / 300 rows: one partial tile, one tile short of full,
# two tiles, and more tiles than waves
CASES = [(f, L, D) for f in ("arith", "all") for L in (64, 128) for D in (1, 63, 65, 300)]
FILL_CASE = ("all", 64, 65)   # run at a population that fills the chip: the one-wave-per-tree path
POP = 24                      # below 16 x the CU count: up to 4 waves share a tree
FILL_DISTINCT = 128           # distinct trees of the chip-filling population (tiled to its size)


def make_case(funcs, gp_len, D, pop=POP, var_len=3):
    rng = np.random.default_rng([20261017, zlib.crc32(f"{funcs}-{gp_len}-{D}-{pop}".encode())])
    value, type_, size = random_forest(rng, pop, gp_len, ARITH if funcs == "arith" else ALL_FUNCS, var_len, 1, max_depth=5)
    X = rng.uniform(0.5, 1.5, (D, var_len)).astype(np.float32)
    y = rng.uniform(-1, 1, (D, 1)).astype(np.float32)
    return value, type_, size, X, y


def comparable(oracle, value, type_, size, X, y):
    """-> (want_loss, want, nabs, stable): the float64 normal equations and the trees that are compared.  The exclusion rule of the
    gradient test: a tree is compared when its float64 loss is finite, its fp32 loss is ulp-stable -- a 3-ulp nudge of every library
    result (the oracle's sensitivity probe) moves it by at most 1e-4 relative -- and its float64 normal equations are well
    conditioned at fp32 resolution: nudging every constant and input by a relative 2^-22 (two draws of random signs) moves no entry
    by more than 1e-4 of its scale."""
    with np.errstate(all="ignore"):
        want_loss, want, nabs = LM.forest_normal_eq(value, type_, size, X, y)
        _, tol, unstable = per_tree_tolerance(oracle, (value, type_, size), X, y, use_mse=True)
        stable = np.isfinite(want_loss) & ~unstable & (tol <= 1e-4 * np.abs(want_loss) + 1e-6)
        is_c = type_.astype(np.int32) == R.T_CONST
        for k in range(2):
            jr = np.random.default_rng(k)
            vj = np.where(is_c, value * (1 + 2.0 ** -22 * jr.choice([-1, 1], value.shape)), value).astype(np.float32)
            Xj = X.astype(np.float64) * (1 + 2.0 ** -22 * jr.choice([-1, 1], X.shape))
            _, nj, _ = LM.forest_normal_eq(vj, type_, size, Xj, y)
            moved = np.abs(nj - want) > 1e-4 * nabs + 1e-9
            stable &= ~np.any(np.where(np.isfinite(want) & np.isfinite(nabs), moved | ~np.isfinite(nj), False), axis=1)
    return want_loss, want, nabs, stable
