"""TEST-ONLY: trees, boxes and sample points shared by the interval tests (tests/test_interval_ref.py, tests/test_gpu_intervals.py)."""
import numpy as np

import sr_grad_ref as R
from subtree_ref import extract_subtrees

ARITH = [R.F_ADD, R.F_SUB, R.F_MUL, R.F_DIV]
LOGIC = ARITH + [R.F_LT, R.F_GT, R.F_LE, R.F_GE, R.F_IF]
ALL = list(range(29))
# the functions whose endpoints are exact float32 operations on the operands' endpoints (rule 1), by arity
EXACT_UNARY = [R.F_NEG, R.F_ABS, R.F_SQRT, R.F_LOOSE_SQRT]
EXACT_BINARY = [R.F_ADD, R.F_SUB, R.F_MUL, R.F_MAX, R.F_MIN]
# every function whose kernel result must equal the restatement bit for bit (rules 1-3 and 7: no library call)
EXACT_TIER = (ARITH + [R.F_LOOSE_DIV, R.F_MAX, R.F_MIN, R.F_LT, R.F_GT, R.F_LE, R.F_GE, R.F_IF, R.F_INV, R.F_LOOSE_INV, R.F_NEG, R.F_ABS,
                       R.F_SQRT, R.F_LOOSE_SQRT])

BOXES = [
    (np.array([-1, -1, -1], np.float32), np.array([1, 1, 1], np.float32)),
    (np.array([0, -1e-3, 5], np.float32), np.array([0, 1e-3, 7], np.float32)),
    (np.array([-1e20, -1e20, -1e20], np.float32), np.array([1e20, 1e20, 1e20], np.float32)),
]


def V(i):
    return ("V", i)


def C(c):
    return ("C", c)


def U(f, a):
    return ("U", f, a)


def B(f, a, b):
    return ("B", f, a, b)


def IF(a, b, c, fid=R.F_IF):
    return ("T", fid, a, b, c)


def flatten(expr):
    """prefix-order list of [value, type, size]"""
    out = []

    def go(e):
        at = len(out)
        if e[0] == "V":
            out.append([np.float32(e[1]), R.T_VAR, 1])
        elif e[0] == "C":
            out.append([np.float32(e[1]), R.T_CONST, 1])
        else:
            out.append([np.float32(e[1]), {"U": 2, "B": 3, "T": 4}[e[0]], 0])
            for k in e[2:]:
                go(k)
            out[at][2] = len(out) - at
    go(expr)
    return out


def rows(exprs, L):
    value, type_, size = np.zeros((len(exprs), L), np.float32), np.zeros((len(exprs), L), np.int16), np.zeros((len(exprs), L), np.int16)
    for t, e in enumerate(exprs):
        nodes = e if isinstance(e, list) else flatten(e)
        assert len(nodes) <= L
        for i, (v, ty, s) in enumerate(nodes):
            value[t, i], type_[t, i], size[t, i] = v, ty, s
    return value, type_, size


def single_op(f, var_len=3):
    """f applied to the first variables: the smallest tree that uses function id f"""
    if f == R.F_IF:
        return IF(V(0), V(1 % var_len), V(2 % var_len))
    if f >= R.F_SIN:
        return U(f, V(0))
    return B(f, V(0), V(1 % var_len))


def chain(f, depth, left=True, leaf=None):
    """a chain of ``depth`` binary nodes f leaning left or right, as a node list (built without recursion)"""
    leaf = leaf or (lambda k: [np.float32(k % 3), R.T_VAR, 1] if k % 2 else [np.float32(0.5 + (k % 5) * 0.25), R.T_CONST, 1])
    n = 2 * depth + 1
    nodes = []
    if left:     # f(f(f(.., l), l), l): the functions first, then the leaves
        for k in range(depth):
            nodes.append([np.float32(f), 3, n - 2 * k])
        nodes += [leaf(k) for k in range(depth + 1)]
    else:        # f(l, f(l, f(l, ..)))
        for k in range(depth):
            nodes.append([np.float32(f), 3, n - 2 * k])
            nodes.append(leaf(k))
        nodes.append(leaf(depth))
    return nodes


def random_exact_forest(rng, pop, L, var_len, full_rows=0, nan_share=0.1):
    """random trees over the exact tier, with NaN / +-inf constants planted in a share of them; the first ``full_rows`` rows have exactly
    L live nodes (a random tree padded on top by unary NEG nodes)"""
    from grad_trees import random_tree

    exprs = []
    for t in range(pop):
        depth = int(rng.integers(2, 7))
        while True:
            nodes = random_tree(rng, EXACT_TIER, var_len, 1, depth, const_range=(-2.0, 2.0))
            if len(nodes) <= L:
                break
        if t < full_rows:
            pad = L - len(nodes)
            nodes = [[np.float32(R.F_NEG), 2, L - k] for k in range(pad)] + nodes
        consts = [i for i, nd in enumerate(nodes) if nd[1] == R.T_CONST]
        if consts and rng.random() < nan_share:
            nodes[int(rng.choice(consts))][0] = np.float32(rng.choice([np.nan, np.inf, -np.inf]))
        exprs.append(nodes)
    return rows(exprs, L)


def oracle_forest(oracle, rng, pop, funcs, var_len=3, gp_len=64, plant=0.1, key=0):
    """``pop`` trees from the oracle's tree_generate over the function ids ``funcs``; NaN / +-inf planted into a CONST of a share"""
    from oracle.pyoracle import depth2leaf, roulette_uniform

    v, t, s = oracle.generate(pop, gp_len, var_len, 1, 0.0, 0.4, [20261018 + key, len(funcs)], depth2leaf(5), roulette_uniform(funcs),
                              [-2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0, 3.0])
    for r in range(pop):
        consts = np.nonzero(t[r, :int(s[r, 0])] == R.T_CONST)[0]
        if len(consts) and rng.random() < plant:
            v[r, int(rng.choice(consts))] = np.float32(rng.choice([np.nan, np.inf, -np.inf]))
    return v, t, s


def sample_points(rng, lower, upper, n=256):
    """n float32 points of the box: every corner first, then each coordinate drawn independently from lower, upper, the midpoint, 0
    (where the box holds it) or a uniform draw"""
    lower, upper = np.asarray(lower, np.float32), np.asarray(upper, np.float32)
    d = len(lower)
    pts = []
    if 2 ** d <= n:
        for m in range(2 ** d):
            pts.append([upper[k] if (m >> k) & 1 else lower[k] for k in range(d)])
    while len(pts) < n:
        p = []
        for k in range(d):
            lo, hi = lower[k], upper[k]
            mid = np.float32(0.5) * lo + np.float32(0.5) * hi
            pick = [lo, hi, mid, np.float32(rng.uniform(float(lo), float(hi)))]
            if lo <= 0 <= hi:
                pick.append(np.float32(0.0))
            p.append(pick[int(rng.integers(len(pick)))])
        pts.append(p)
    X = np.array(pts, np.float32)
    return np.minimum(np.maximum(X, lower[None, :]), upper[None, :])


def all_subtree_rows(value, type_, size):
    """every subtree of every (well-formed) tree as a row of its own, and (tree, node) of every row"""
    vs, ts, ss, where = [], [], [], []
    for t in range(value.shape[0]):
        v, ty, s = extract_subtrees(value, type_, size, t)
        vs.append(v); ts.append(ty); ss.append(s)
        where += [(t, i) for i in range(v.shape[0])]
    return np.concatenate(vs), np.concatenate(ts), np.concatenate(ss), np.array(where)


def ulp_key(x):
    """the position of float32 x on the line of floats (-0.0 and +0.0 share one)"""
    s = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
    return np.where(s >= 0, s, -(s & 0x7FFFFFFF))
