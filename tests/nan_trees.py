"""The arithmetic line's NaN-poisoned trees, restated on the host (evogp_amd/csrc/sr_tc.hip, compile_pack_arith).

A tree of + - * / over variables and constants whose value is a NaN CONSTANT somewhere -- a NaN constant leaf, a function of two
constant leaves that folds to NaN (0 / 0, inf - inf, c / 0), a function whose operands become constants through that first fold
and which folds to NaN itself, or a division whose right operand is (or folds to) a zero constant -- is NaN in every row: each of
+ - * / hands a NaN operand on (x / NaN included), and the row errors are summed.  The compiler gives such a tree the one-word
program NAN_TREE.  `poisoned` finds the trees the compiler finds, with the compiler's two folding rounds and nothing more."""
import numpy as np

T_VAR, T_CONST, T_BFUNC = 0, 1, 3
ADD, SUB, MUL, DIV = 1, 2, 3, 4


def _fold(op, x, y):
    """the interpreter's arithmetic on constants (forward.cu:177-187): float32, x / 0 is NaN"""
    with np.errstate(all="ignore"):
        q = np.where(y == 0, np.float32(np.nan), x / np.where(y == 0, np.float32(1), y))
        return np.select([op == ADD, op == SUB, op == MUL], [x + y, x - y, x * y], q).astype(np.float32)


def poisoned(value, type_, size):
    """bool per tree: the compiler proves the tree NaN in every row (trees of at most 64 nodes over + - * / only)"""
    v = np.ascontiguousarray(value, np.float32)
    t = np.asarray(type_).astype(np.int32)
    s = np.asarray(size).astype(np.int32)
    pop, L = v.shape
    n = s[:, 0]
    idx = np.arange(L)[None, :]
    inside = idx < n[:, None]
    op = np.where(t == T_BFUNC, v, 0).astype(np.int32)
    isC = inside & (t == T_CONST)
    isB = inside & (t == T_BFUNC) & (op >= ADD) & (op <= DIV)
    line = (inside & ~((t == T_VAR) | (t == T_CONST) | isB)).sum(1) == 0
    li = np.minimum(idx + 1, L - 1).repeat(pop, 0)
    ri = np.minimum(idx + 1 + np.take_along_axis(s, li, 1), L - 1)
    g = lambda a, i: np.take_along_axis(a, i, 1)
    # first round: functions of two constant leaves
    absorbed = isB & g(isC, li) & g(isC, ri)
    folded = _fold(op, g(v, li), g(v, ri))
    ec = isC | absorbed
    ev = np.where(absorbed, folded, v)
    # second round: functions whose operands became constants
    cc = isB & ~absorbed & g(ec, li) & g(ec, ri)
    folded2 = _fold(op, g(ev, li), g(ev, ri))
    dz = isB & (op == DIV) & g(ec, ri) & (g(ev, ri) == 0)
    nanc = (isC & np.isnan(v)) | (absorbed & np.isnan(folded)) | (cc & np.isnan(folded2)) | dz
    return line & (n >= 1) & (n <= 64) & nanc.any(1)


def crafted_forest():
    """trees that put NaN, +-inf, +-0 and x / 0 in every operand position, nested, with a control tree of each shape that is not NaN"""
    V, C, B = T_VAR, T_CONST, T_BFUNC
    nan, inf = float("nan"), float("inf")
    trees = []
    for o in (ADD, SUB, MUL, DIV):
        for c in (nan, inf, -inf, 0.0, -0.0, 1.0, -1.0):
            trees.append([(B, o, 3), (V, 0, 1), (C, c, 1)])                                 # x o c
            trees.append([(B, o, 3), (C, c, 1), (V, 1, 1)])                                 # c o x
            trees.append([(B, ADD, 5), (B, o, 3), (V, 0, 1), (C, c, 1), (V, 2, 1)])         # (x o c) + z
            trees.append([(B, MUL, 5), (V, 2, 1), (B, o, 3), (C, c, 1), (V, 1, 1)])         # z * (c o x)
            for c2 in (0.0, -0.0, 1.0, inf):
                trees.append([(B, DIV, 5), (V, 0, 1), (B, o, 3), (C, c, 1), (C, c2, 1)])    # x / (c o c2): a divisor that folds
                trees.append([(B, SUB, 7), (V, 3, 1), (B, DIV, 5), (V, 0, 1), (B, o, 3), (C, c, 1), (C, c2, 1)])
                # (c o c2) o (c2 o c): folded in the second round
                trees.append([(B, o, 7), (B, o, 3), (C, c, 1), (C, c2, 1), (B, ADD, 3), (C, c2, 1), (C, c, 1)])
                trees.append([(B, DIV, 9), (V, 1, 1), (B, o, 7), (B, SUB, 3), (C, c, 1), (C, c2, 1), (B, MUL, 3), (C, c2, 1), (C, c, 1)])
    trees.append([(C, nan, 1)])
    trees.append([(C, 0.0, 1)])
    trees.append([(V, 4, 1)])
    trees.append([(B, DIV, 3), (C, 0.0, 1), (C, 0.0, 1)])
    # a deep chain with the x / 0 at the bottom
    chain = [(B, DIV, 3), (V, 5, 1), (C, 0.0, 1)]
    for k in range(20):
        chain = [(B, (ADD, SUB, MUL, DIV)[k % 4], len(chain) + 2), (V, k % 6, 1)] + chain
    trees.append(chain)
    L = 64
    pop = len(trees)
    v = np.zeros((pop, L), np.float32); t = np.zeros((pop, L), np.int16); s = np.zeros((pop, L), np.int16)
    for i, tr in enumerate(trees):
        for j, (ty, val, sz) in enumerate(tr):
            t[i, j], v[i, j], s[i, j] = ty, val, sz
    # the sizes must describe the trees
    for i, tr in enumerate(trees):
        assert s[i, 0] == len(tr), i
    return v, t, s


def special_dataset(D, var_len, seed):
    """columns of finite values with -0, +-inf and NaN planted in some of them"""
    r = np.random.default_rng(seed)
    X = r.uniform(-3, 3, (D, var_len)).astype(np.float32)
    y = r.uniform(-3, 3, (D, 1)).astype(np.float32)
    X[::7, 0] = -0.0
    X[::5, 1] = 0.0
    if D > 3:
        X[1, 2] = np.inf; X[2, 3] = -np.inf; X[3, 4] = np.nan
    y[::11, 0] = -0.0
    return X, y
