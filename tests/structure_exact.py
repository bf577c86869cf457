"""TEST-ONLY: an independent checker of the structural pass (tests/structure_ref.py, csrc/sr_structure.hip).  It shares nothing with the
walk: the prefix row is parsed recursively into nested tuples ``(symbol, index, children)`` and every quantity is computed from its
textbook statement --
  depth        the number of edges from the root down to the node, by recursion
  height       the number of nodes on the longest path from the node down to a leaf
  complexity   the sum of the costs over the node set of the subtree
  below_r      the maximum, over every path from the node down to a leaf, of the number of inner symbols strictly below the node
and the flags from those.  ``parse`` returns None for a row that is not exactly one tree with true size words."""
import sys

import numpy as np

VAR, CONST, UNKNOWN = 29, 30, 31


def _symbol(t, v):
    """(symbol, arity) from the raw words: type 0 a variable, 1 a constant, 2 unary, 3 binary, anything else ternary"""
    t = int(t)
    if t == 0:
        return VAR, 0
    if t == 1:
        return CONST, 0
    if t not in (2, 3):
        return 0, 3
    f = int(np.float32(v))
    lo, hi = (14, 28) if t == 2 else (1, 13)
    return (f if lo <= f <= hi else UNKNOWN), (1 if t == 2 else 2)


def parse(value, type_, size):
    """the nested tuples of the live prefix, or None"""
    L = len(value)
    n = min(max(int(size[0]), 0), L)
    if n == 0:
        return None
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 4 * L + 200))

    def go(at):
        if at >= n:
            raise ValueError
        s, arity = _symbol(type_[at], value[at])
        kids, nxt = [], at + 1
        for _ in range(arity):
            kid, nxt = go(nxt)
            kids.append(kid)
        if int(size[at]) != nxt - at:
            raise ValueError
        return (s, at, kids), nxt

    try:
        tree, end = go(0)
    except ValueError:
        return None
    return tree if end == n else None


def nodes_of(tree):
    out = [tree]
    for k in tree[2]:
        out += nodes_of(k)
    return out


def node_height(tree):
    return 1 + max([node_height(k) for k in tree[2]], default=0)


def paths_down(tree):
    """every path from the node to a leaf, as lists of symbols, the node's own first"""
    if not tree[2]:
        return [[tree[0]]]
    return [[tree[0]] + p for k in tree[2] for p in paths_down(k)]


def inner_below(tree, inner):
    """the largest number of inner symbols strictly below the node on one path down.  (Paths are enumerated only for small trees; the
    recursion below is the same maximum, path by path.)"""
    return max([((inner >> k[0]) & 1) + inner_below(k, inner) for k in tree[2]], default=0)


def check_row(value, type_, size, cost, operand_limit, rules, max_depth, max_complexity):
    """-> dict of per-node arrays and the count, or None for a malformed row"""
    tree = parse(value, type_, size)
    if tree is None:
        return None
    L, R = len(value), len(rules)
    out = dict(complexity=np.zeros(L, np.int64), height=np.zeros(L, np.int64), depth=np.zeros(L, np.int64), nest=np.zeros((L, R), np.int64),
               flags=np.zeros(L, np.int64))

    def descend(node, d):
        out["depth"][node[1]] = d
        for k in node[2]:
            descend(k, d + 1)

    descend(tree, 0)
    count = 0
    for node in nodes_of(tree):
        s, i, kids = node
        out["complexity"][i] = sum(int(cost[m[0]]) for m in nodes_of(node))
        out["height"][i] = node_height(node)
        f = 0
        for r, (outer, inner, limit) in enumerate(rules):
            below = inner_below(node, inner)
            out["nest"][i, r] = min(255, below + ((inner >> s) & 1))
            if (outer >> s) & 1 and below > limit:
                f |= 1
        for k, kid in enumerate(kids):
            lim = int(operand_limit[s][k])
            if lim >= 0 and sum(int(cost[m[0]]) for m in nodes_of(kid)) > lim:
                f |= 2
        out["flags"][i] = f
        count += f != 0
    if max_depth >= 0 and node_height(tree) > max_depth:
        out["flags"][0] |= 8
        count += 1
    if max_complexity >= 0 and out["complexity"][0] > max_complexity:
        out["flags"][0] |= 16
        count += 1
    out["violations"] = int(count)
    return out
