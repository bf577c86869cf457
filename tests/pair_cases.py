"""TEST-ONLY: forests, datasets and events for the tests of the pairwise semantic moments (tests/test_pair_ref.py, test_pair_host.py,
test_gpu_pairs.py).

``pair_forest``: random trees over the chosen function set with constants in [-1.5, 1.5], and, from 63 rows on, planted rows:
    2   n = 0 (malformed)                5   ADD with one operand (malformed)        7   T + 0 * S, S a sum that needs 20 operands (deep)
    9   T                                11  x1 + HUGE: -inf on the LAST row only    13  x0 / 0: NaN on every row
    15  a structural copy of row 9       17  sin(T) (FULL build)                     19  sin(T + 0 * S) (FULL build first, then deep)
    21  (gp_len > 64) a comb of 79 nodes: deeper than the register stack             23, 30, 37, ...  x_k / (x_j - x_j) + a random tree: NaN
and garbage behind every live prefix.  Row 0 is always x0 * x1 (finite), so a population of one tree has a usable pair.
``dataset``: tests/semantic_cases.py's, rows in [-2, 2] and x0 = -7 on the last one; labels x0 x1 - x2 / 1.5 + noise.
``events``: first (E,) and candidates (E, M) uniform over the forest, with every 17th index replaced by one outside it."""
import functools
import zlib

import numpy as np

import sr_grad_ref as R
from dedup_cases import comb, garbage_tails
from grad_trees import ALL_FUNCS, ARITH, random_forest, random_tree
from semantic_cases import HUGE, T, X0, X1, dataset, left_sum, nodes_of, plant

MALFORMED = (2, 5)
DEEP_ROW, T_ROW, INF_LAST_ROW, NAN_ROW, COPY_ROW, HEAVY_ROW, HEAVY_DEEP_ROW, COMB_ROW = 7, 9, 11, 13, 15, 17, 19, 21
OUTSIDE = (-1, None, 2 ** 31 - 1, -2 ** 31)   # None: the population size


def _set(value, type_, size, t, words):
    assert len(words) <= value.shape[1]
    value[t], type_[t], size[t] = 0, 0, 0
    for i, (v, ty, s) in enumerate(words):
        value[t, i], type_[t, i], size[t, i] = v, ty, s


@functools.lru_cache(maxsize=None)
def pair_forest(funcs, gp_len, pop, var_len=3, seed=0):
    """(value, type, size), read-only"""
    rng = np.random.default_rng([20261021, zlib.crc32(funcs.encode()), gp_len, pop, var_len, seed])
    fs = ARITH if funcs == "arith" else ALL_FUNCS
    value, type_, size = random_forest(rng, pop, gp_len, fs, var_len, 1, max_depth=5 if funcs == "arith" else 4, const_range=(-1.5, 1.5))
    plant(value, type_, size, 0, ("mul", X0, X1))
    if pop >= 63:
        zero = ("c", np.float32(0.0))
        deep = ("add", T, ("mul", zero, left_sum(20, rng)))
        for t, e in ((DEEP_ROW, deep), (T_ROW, T), (INF_LAST_ROW, ("add", X1, HUGE)), (NAN_ROW, ("div", X0, zero)), (COPY_ROW, T),
                     (HEAVY_ROW, ("sin", T)), (HEAVY_DEEP_ROW, ("sin", deep)), (5, ("add", X0))):
            plant(value, type_, size, t, e)
        size[5, 0] = 2
        size[2, 0] = 0
        if gp_len > 64:
            value[COMB_ROW], type_[COMB_ROW], size[COMB_ROW] = comb(40, gp_len, rng)
        for t in range(23, pop, 7):
            k, j = int(rng.integers(var_len)), int(rng.integers(var_len))
            tail = random_tree(rng, fs, var_len, 1, 3, const_range=(-1.5, 1.5))
            nan = nodes_of(("div", ("x", k), ("sub", ("x", j), ("x", j))))
            words = [(float(R.F_ADD), R.T_BFUNC, 1 + len(nan) + len(tail))] + nan + [tuple(w) for w in tail]
            _set(value, type_, size, t, words)
    garbage_tails(rng, value, type_, size)
    for a in (value, type_, size):
        a.setflags(write=False)
    return value, type_, size


@functools.lru_cache(maxsize=None)
def pair_data(D, var_len=3, seed=0):
    """(X (D, var_len), y (D,)) float32, read-only"""
    rng = np.random.default_rng([77, D, var_len, seed])
    X = dataset(rng, D, var_len)
    y = (X[:, 0] * X[:, 1] - X[:, 2] / np.float32(1.5) + rng.normal(0.0, 0.1, D)).astype(np.float32)
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y


def events(rng, E, M, pop_a, pop_b=None):
    """first (E,) int32 into a forest of pop_a rows, candidates (E, M) int32 into one of pop_b rows; every 17th index lies outside"""
    pop_b = pop_a if pop_b is None else pop_b
    first = rng.integers(0, pop_a, E).astype(np.int64)
    cand = rng.integers(0, pop_b, (E, M)).astype(np.int64)
    out = [o for o in OUTSIDE]
    flat = cand.reshape(-1)
    for k, i in enumerate(range(5, flat.size, 17)):
        o = out[k % len(out)]
        flat[i] = pop_b if o is None else o
    for k, i in enumerate(range(11, E, 17)):
        o = out[k % len(out)]
        first[i] = pop_a if o is None else o
    return first.astype(np.int32), cand.astype(np.int32)


# (funcs, gp_len, pop, E, M, D, var_len, labels): every value of the issue's shape list at least once -- pop 1 / 63 / 200, E 1 / 65 / 300,
# M 1 / 3 / 16, gp_len 64 / 1024, D 1 / 63 / 64 / 65 / 257 / 1100 (ragged tiles; five tiles for four waves), var_len 40 (the scratch-stack
# kernel alone), var_len 13 (the 32-wide register tuple), both function sets, with and without labels
SHAPES = [
    ("arith", 64, 1, 1, 1, 1, 3, True),
    ("arith", 64, 1, 65, 3, 257, 3, True),
    ("arith", 64, 63, 65, 3, 63, 3, True),
    ("all", 64, 63, 1, 16, 64, 3, False),
    ("all", 64, 200, 300, 16, 65, 3, True),
    ("arith", 1024, 200, 65, 16, 257, 3, True),
    ("all", 1024, 63, 300, 3, 1100, 3, True),
    ("arith", 64, 200, 300, 1, 1100, 3, False),
    ("all", 64, 200, 65, 3, 1100, 13, True),
    ("all", 64, 63, 65, 3, 65, 40, True),
    ("all", 1024, 200, 65, 16, 1, 3, True),
]


def shape_id(s):
    return "{}-L{}-pop{}-E{}-M{}-D{}-v{}{}".format(*s[:7], "" if s[7] else "-nolabels")


def case_events(shape):
    funcs, gp_len, pop, E, M, D, var_len, _ = shape
    return events(np.random.default_rng([5, zlib.crc32(shape_id(shape).encode())]), E, M, pop)


def check_condition(shape, mom):
    """the condition on the inputs: at least a quarter of the pairs finite and at least a tenth NaN (restatement's words).  One event of
    one pair cannot show both: there the forest's tree 0 is finite by construction and the pair is whatever its two indices make it"""
    nan = np.isnan(mom[..., 0])
    if nan.size < 10:
        return
    assert (~nan).mean() >= 0.25 and nan.mean() >= 0.10, (shape_id(shape), float((~nan).mean()), float(nan.mean()))
