"""TEST-ONLY: a numpy restatement of the per-subtree pass and of the rewrite that uses it (csrc/sr_subtree.hip, single-output trees).

``forest_subtree_errors(value, type, size, X, y, use_mse, value_dtype)`` -> ``(node_err, node_const)``, both (pop, L):
    node_err[t][i]    (1/D) sum_d err(y[d] - v_i(X[d])) in float64, v_i the value of the subtree rooted at node i (evaluated in
                      ``value_dtype``: float64, or float32 as the engine does -- then a folded tree keeps its errors exactly)
    node_const[t][i]  float32: the value of v_i when it has one bit pattern on every row and is not a NaN, else NaN.  Constancy is a
                      statement about float32 bit patterns, so v_i is evaluated in float32 for it: exact for + - * / (every step is
                      correctly rounded on both sides), a library function may differ from the device's by an ulp
Tail entries and malformed trees are NaN.

``prune_rows(value, type, size, node_err, node_const, hoist, fold)`` -> ``(value, type, size, root_pos, loss)`` is the rule of
include/evogp_hip.h evogp_hip_prune_rows in integer and float32 comparisons: the kernel must reproduce it bit for bit."""
import numpy as np

from sr_grad_ref import ARITY, T_CONST, T_VAR, binary, decode, unary


def live_len(size_row, L):
    return min(max(int(size_row[0]), 0), L)


def well_formed(type_row, n):
    """the stack discipline classify_tree checks (single-output mode: the raw type decides the arity)"""
    if n <= 0:
        return False
    h = 0
    for i in reversed(range(n)):
        t = int(type_row[i])
        h += 1 - (0 if t in (T_VAR, T_CONST) else 1 if t == 2 else 2 if t == 3 else 3)
        if h < 1:
            return False
    return h == 1


def node_values(value, type_, size, X, dtype=np.float64):
    """one tree: the list of v_i (each an array over the rows of X) for i < len, or None for a malformed tree"""
    L = len(value)
    D, var_len = X.shape
    n = live_len(size, L)
    if not well_formed(type_, n):
        return None
    nodes = [decode(type_[i], value[i], False, var_len, 1) for i in range(n)]
    X = X.astype(dtype)
    val = [None] * n
    stack = []
    for i in reversed(range(n)):
        kind, f, _ = nodes[i]
        if kind == "C":
            val[i] = np.full(D, f, dtype=dtype)
        elif kind == "V":
            val[i] = X[:, f]
        else:
            ops = [val[stack.pop()] for _ in range(ARITY[kind])]   # top of stack first: a, b, c
            with np.errstate(all="ignore"):
                if kind == "U":
                    r = unary(f, ops[0])
                elif kind == "B":
                    r = binary(f, ops[0], ops[1])
                else:
                    r = np.where(ops[0] > 0, ops[1], ops[2])
            val[i] = np.asarray(r, dtype=dtype)
        stack.append(i)
    return val


def tree_subtree_errors(value, type_, size, X, y, use_mse=True, value_dtype=np.float64):
    L = len(value)
    err = np.full(L, np.nan)
    const = np.full(L, np.nan, np.float32)
    v64 = node_values(value, type_, size, X, value_dtype)
    if v64 is None:
        return err, const
    v32 = node_values(value, type_, size, X, np.float32)
    yy = np.asarray(y, np.float64).reshape(-1)
    for i in range(len(v64)):
        with np.errstate(all="ignore"):
            diff = yy - v64[i].astype(np.float64)
            err[i] = np.mean(diff * diff if use_mse else np.abs(diff))
        b = np.ascontiguousarray(v32[i], np.float32).view(np.uint32)
        if np.all(b == b[0]) and not np.isnan(v32[i][0]):
            const[i] = v32[i][0]
    return err, const


def forest_subtree_errors(value, type_, size, X, y, use_mse=True, value_dtype=np.float64):
    value, type_, size = np.asarray(value), np.asarray(type_), np.asarray(size)
    pop, L = value.shape
    err = np.full((pop, L), np.nan)
    const = np.full((pop, L), np.nan, np.float32)
    for t in range(pop):
        err[t], const[t] = tree_subtree_errors(value[t], type_[t], size[t], np.asarray(X), np.asarray(y), use_mse, value_dtype)
    return err, const


def extract_subtrees(value, type_, size, t):
    """every subtree of (well-formed) tree t as a row of its own: row i holds nodes [i, i + size[t][i]) from position 0"""
    L = value.shape[1]
    n = live_len(size[t], L)
    v = np.zeros((n, L), np.float32)
    ty = np.zeros((n, L), np.int16)
    s = np.zeros((n, L), np.int16)
    for i in range(n):
        k = int(size[t, i])
        v[i, :k], ty[i, :k], s[i, :k] = value[t, i:i + k], type_[t, i:i + k], size[t, i:i + k]
    return v, ty, s


# ---- the rewrite rule ---------------------------------------------------------------------------------------------------------------
def prune_row(value, type_, size, err, const, hoist, fold):
    L = len(value)
    n = live_len(size, L)
    if not well_formed(type_, n):   # malformed: the row as it is
        return value.copy(), type_.copy(), size.copy(), 0, np.float32(np.nan)
    err = np.asarray(err, np.float32)
    const = np.asarray(const, np.float32)

    def span(j):
        return min(max(int(size[j]), 1), n - j)

    r = 0
    if hoist:
        cand = [i for i in range(n) if np.isfinite(err[i])]
        if cand:
            r = min(cand, key=lambda i: (float(err[i]), span(i), i))   # (floats compare as floats: -0.0 ties with 0.0)
    r1 = r + span(r)
    folds = [bool(fold) and int(type_[j]) not in (T_VAR, T_CONST) and bool(np.isfinite(const[j])) for j in range(r, r1)]
    keep, cover = [], 0
    for j in range(r, r1):
        keep.append(cover <= j)                      # not strictly inside the span of a folding node in front of it
        if folds[j - r]:
            cover = max(cover, j + span(j))
    before = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)   # kept nodes in front of node r + k
    ov, ot, os_ = np.zeros(L, np.float32), np.zeros(L, np.int16), np.zeros(L, np.int16)
    for j in range(r, r1):
        if not keep[j - r]:
            continue
        at = before[j - r]
        if folds[j - r]:
            ov[at], ot[at], os_[at] = const[j], T_CONST, 1
        else:
            ov[at], ot[at], os_[at] = value[j], type_[j], before[min(j + span(j), r1) - r] - at
    return ov, ot, os_, r, err[r]


def prune_rows(value, type_, size, node_err, node_const, hoist=True, fold=True):
    value, type_, size = np.asarray(value, np.float32), np.asarray(type_, np.int16), np.asarray(size, np.int16)
    pop, L = value.shape
    ov, ot, os_ = np.zeros_like(value), np.zeros_like(type_), np.zeros_like(size)
    root = np.zeros(pop, np.int32)
    loss = np.zeros(pop, np.float32)
    for t in range(pop):
        ov[t], ot[t], os_[t], root[t], loss[t] = prune_row(value[t], type_[t], size[t], node_err[t], node_const[t], hoist, fold)
    return ov, ot, os_, root, loss


def check_prefix_tree(type_row, size_row):
    """is the live prefix a well-formed prefix tree whose every size is the size of its subtree (and the tail zero)?"""
    L = len(type_row)
    n = live_len(size_row, L)
    if not well_formed(type_row, n):
        return False

    def walk(i):
        t = int(type_row[i])
        k = 0 if t in (T_VAR, T_CONST) else 1 if t == 2 else 2 if t == 3 else 3
        j = i + 1
        for _ in range(k):
            j = walk(j)
            if j < 0:
                return -1
        return j if int(size_row[i]) == j - i else -1

    return walk(0) == n and not np.any(type_row[n:]) and not np.any(size_row[n:])
