"""TEST-ONLY: single-output forests with planted semantic duplicates and near-duplicates, and the dataset that goes with them, for the
tests of csrc/sr_semantic.hip (tests/test_semantic_ref.py, tests/test_semantic_host.py, tests/test_gpu_semantics.py)."""
import numpy as np

import sr_grad_ref as R
from dedup_cases import comb, garbage_tails
from grad_trees import ALL_FUNCS, ARITH, random_forest

_BINARY = {"add": R.F_ADD, "sub": R.F_SUB, "mul": R.F_MUL, "div": R.F_DIV, "pow": R.F_POW, "max": R.F_MAX, "min": R.F_MIN}
_UNARY = {"neg": R.F_NEG, "sin": R.F_SIN, "exp": R.F_EXP}


def nodes_of(expr):
    """prefix-order (value, type, size) words of a nested tuple: ("x", k), ("c", v), (unary, a), (binary, a, b)"""
    op = expr[0]
    if op == "x":
        return [(float(expr[1]), R.T_VAR, 1)]
    if op == "c":
        return [(expr[1], R.T_CONST, 1)]
    kids = [nodes_of(e) for e in expr[1:]]
    n = 1 + sum(len(k) for k in kids)
    head = (float(_UNARY[op]), R.T_UFUNC, n) if op in _UNARY else (float(_BINARY[op]), R.T_BFUNC, n)
    return [head] + [w for k in kids for w in k]


def plant(value, type_, size, t, expr):
    words = nodes_of(expr)
    assert len(words) <= value.shape[1]
    value[t], type_[t], size[t] = 0, 0, 0
    for i, (v, ty, s) in enumerate(words):
        value[t, i], type_[t, i], size[t, i] = v, ty, s


def left_sum(n, rng):
    """((c + c) + c) + ... of n constants in [0.5, 1.5]: executed in reverse prefix order it holds n operands at once"""
    e = ("c", np.float32(rng.uniform(0.5, 1.5)))
    for _ in range(n - 1):
        e = ("add", e, ("c", np.float32(rng.uniform(0.5, 1.5))))
    return e


X0, X1, X2 = ("x", 0), ("x", 1), ("x", 2)
A = X0
B = ("mul", X1, ("c", np.float32(1.25)))
T = ("sub", ("mul", X0, X1), ("div", X2, ("c", np.float32(1.5))))
Z = ("min", ("add", X0, ("c", np.float32(5.0))), ("c", np.float32(0.0)))   # 0 on every row but the last, where x0 = -7: -2
HUGE = ("mul", Z, ("c", np.float32(3e38)))                                  # 0 / -inf

# rows that must share a class, as tuples of row indices (from 63 rows on)
SAME = [(3, 4), (5, 6), (7, 8), (9, 10, 11, 12), (13, 14), (15, 16), (17, 18), (20, 21), (22, 23), (24, 25), (30, 31), (38, 39)]
# pairs that must not
DIFFERENT = [(26, 27), (28, 29), (32, 33)]
MALFORMED = [34, 35, 36, 37]
DEEP_ROW, FULL_ROW, COPY_ROW, COPY_OF = 18, 24, 19, 0


def dataset(rng, D, var_len=3):
    """(D, var_len) float32 in [-2, 2]; the LAST row has x0 = -7, the only row on which max(x0, -5) is not x0"""
    X = rng.uniform(-2, 2, (D, var_len)).astype(np.float32)
    X[D - 1, 0] = -7.0
    return X


def planted_forest(rng, pop, gp_len, var_len=3):
    """(value, type, size): half the rows arithmetic trees, half trees over all 29 functions, garbage tails everywhere.  From 63 rows on
    (SAME, DIFFERENT and MALFORMED list them):
      3 / 4     a + b, b + a                  5 / 6     a * b, b * a                   7 / 8     a - b, a + neg(b)
      9 .. 12   T, T * 1, T + 0, neg(neg(T))  13 / 14   x + x, x * 2                   15 / 16   two different trees, NaN on every row
      17 / 18   T, ADD(T, MUL(0, S)) with S a finite sum that needs an operand stack of 20 (register stack: 16)
      19        a literal copy of row 0; row pop - 1 a copy of row 9
      20 / 21   sin(x0) + exp(x1), commuted   22 / 23   pow(x0, 2) * x1, commuted      24 / 25   sin(c + (c + ...)) of gp_len nodes, its two innermost constants swapped
      26 / 27   (a + b) + c, a + (b + c): different        28 / 29   x0, max(x0, -5): differ on the last row only
      30 / 31   differ by -0.0 against +0.0 on the last row only: SAME class
      32 / 33   differ by -inf against NaN on the last row only: different
      38 / 39   sin(T), sin(ADD(T, MUL(0, S))): marked for the FULL build first and only then found too deep
      34, 37    empty rows (n = 0)   35   n = gp_len + 1 over a tree cut off by the end of the row   36   ADD with one operand
    gp_len > 64: rows 41 / 44 a comb of 79 nodes and the same with its two innermost constants swapped (same class)."""
    half = pop // 2
    a = random_forest(rng, pop - half, gp_len, ARITH, var_len, 1, max_depth=4)
    if half:
        b = random_forest(rng, half, gp_len, ALL_FUNCS, var_len, 1, max_depth=4)
        value, type_, size = (np.concatenate([x, y]) for x, y in zip(a, b))
        order = rng.permutation(pop)
        value, type_, size = value[order], type_[order], size[order]
    else:
        value, type_, size = a
    if pop >= 63:
        one, zero, two = ("c", np.float32(1.0)), ("c", np.float32(0.0)), ("c", np.float32(2.0))
        for t, e in ((3, ("add", A, B)), (4, ("add", B, A)), (5, ("mul", A, B)), (6, ("mul", B, A)),
                     (7, ("sub", A, B)), (8, ("add", A, ("neg", B))),
                     (9, T), (10, ("mul", T, one)), (11, ("add", T, zero)), (12, ("neg", ("neg", T))),
                     (13, ("add", X1, X1)), (14, ("mul", X1, two)),
                     (15, ("div", X0, zero)), (16, ("add", ("div", X1, zero), X2)),
                     (17, T), (18, ("add", T, ("mul", zero, left_sum(20, rng)))),
                     (20, ("add", ("sin", X0), ("exp", X1))), (21, ("add", ("exp", X1), ("sin", X0))),
                     (22, ("mul", ("pow", X0, two), X1)), (23, ("mul", X1, ("pow", X0, two))),
                     (26, ("add", ("add", X0, X1), X2)), (27, ("add", X0, ("add", X1, X2))),
                     (28, X0), (29, ("max", X0, ("c", np.float32(-5.0)))),
                     (30, ("mul", Z, zero)), (31, zero),
                     (32, ("add", X1, HUGE)), (33, ("add", X1, ("mul", HUGE, zero))),
                     (36, ("add", X0)),
                     (38, ("sin", T)), (39, ("sin", ("add", T, ("mul", zero, left_sum(20, rng)))))):
            plant(value, type_, size, t, e)
        size[36, 0] = 2
        value[19], type_[19], size[19] = value[COPY_OF], type_[COPY_OF], size[COPY_OF]
        value[24], type_[24], size[24] = comb(gp_len // 2, gp_len, rng, unary_root=True)   # n == gp_len
        value[25], type_[25], size[25] = value[24], type_[24], size[24]
        value[25, gp_len - 2], value[25, gp_len - 1] = value[24, gp_len - 1], value[24, gp_len - 2]
        for t in (34, 37):
            size[t, 0] = 0
        value[35], type_[35], size[35] = 0, 0, 0   # ADD x0 ADD x0 ... ADD x0: the last ADD has lost an operand to the end of the row
        value[35, 0::2], type_[35, 0::2] = R.F_ADD, R.T_BFUNC
        type_[35, 1::2] = R.T_VAR
        size[35, 0::2], size[35, 1::2] = np.arange(gp_len + 1, 1, -2)[:gp_len // 2], 1
        if gp_len > 64:
            value[41], type_[41], size[41] = comb(40, gp_len, rng)
            value[44], type_[44], size[44] = value[41], type_[41], size[41]
            value[44, 77], value[44, 78] = value[41, 78], value[41, 77]
    garbage_tails(rng, value, type_, size)
    if pop >= 63:
        n = int(size[9, 0])
        value[pop - 1, :n], type_[pop - 1, :n], size[pop - 1, :n] = value[9, :n], type_[9, :n], size[9, :n]
    return value, type_, size
