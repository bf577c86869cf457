"""The arithmetic line's Z rule, restated on the host (evogp_amd/csrc/sr_tc.hip, compile_pack_arith, TcCompileParams::nan_trees = 2).

On top of tests/nan_trees.py (a NaN constant, or a division by a zero CONSTANT, makes a tree NaN in every row): a division is NaN in
every row as well when its divisor is +-0 or NaN in every row, whatever the data.  Z = "this node's value is +-0 or NaN in every row":

  * a constant -- a leaf, or a function folded in the compiler's first or second folding round -- that is +-0 or NaN;
  * v - v, both operands leaves of the same variable (0 where v is finite, NaN where it is not);
  * a * b with a or b in Z (0 * finite = 0, 0 * inf = NaN, NaN stays);
  * a + b, a - b with a and b in Z;
  * a / b with a in Z (0 / b is 0, or NaN where b is 0 or NaN).

Z goes up one level per round (a node looks at its two children), ROUNDS rounds; the headline forest of six layers reaches its fixed
point after four (which marks another 0.12 % of its trees), a deeper tree may keep a division whose divisor only more rounds would prove.  A tree is proved NaN when it holds a NaN constant or a
division whose right operand is in Z.  (The compiler compares variable leaves by the column they read -- the index truncated and clamped to the
dataset's width; this file compares the leaves' values, the same for every forest whose variable indices are in range.)"""
import numpy as np

from nan_trees import ADD, DIV, MUL, SUB, T_BFUNC, T_CONST, T_VAR, _fold

ROUNDS = 3   # sr_tc.hip kZeroRounds


def proved_nan(value, type_, size, rounds=ROUNDS):
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
    isV = inside & (t == T_VAR)
    isB = inside & (t == T_BFUNC) & (op >= ADD) & (op <= DIV)
    line = (inside & ~(isV | isC | isB)).sum(1) == 0
    li = np.minimum(idx + 1, L - 1).repeat(pop, 0)
    g = lambda a, i: np.take_along_axis(a, i, 1)
    ri = np.minimum(idx + 1 + g(s, li), L - 1)
    # the two folding rounds (nan_trees.poisoned)
    absorbed = isB & g(isC, li) & g(isC, ri)
    folded = _fold(op, g(v, li), g(v, ri))
    ec = isC | absorbed
    ev = np.where(absorbed, folded, v)
    cc = isB & ~absorbed & g(ec, li) & g(ec, ri)
    folded2 = _fold(op, g(ev, li), g(ev, ri))
    ec2 = ec | cc
    ev2 = np.where(cc, folded2, ev)
    # Z: constants, v - v, then upwards
    same = isB & (op == SUB) & g(isV, li) & g(isV, ri) & (g(v, li) == g(v, ri))
    Z = (ec2 & ((ev2 == 0) | np.isnan(ev2))) | same
    for _ in range(rounds):
        Zl, Zr = g(Z, li), g(Z, ri)
        Z = Z | (isB & (((op == MUL) & (Zl | Zr)) | (((op == ADD) | (op == SUB)) & Zl & Zr) | ((op == DIV) & Zl)))
    nanc = (ec2 & np.isnan(ev2)) | (isB & (op == DIV) & g(Z, ri))
    return line & (n >= 1) & (n <= 64) & nanc.any(1)
