"""TEST-ONLY: the integer restatement of the structural pass over SR trees (csrc/sr_structure.hip) -- and its DEFINITION: the kernel
follows this file rule by rule, and since all arithmetic is integer it must give the same words.

``forest_structure(value, type, size, cost, operand_limit, rule_outer, rule_inner, rule_limit, max_depth, max_complexity)`` ->
``(complexity (pop, L) int32, height (pop, L) int16, depth (pop, L) int16, nest (pop, L, R) uint8, flags (pop, L) uint8,
violations (pop,) int32)``.

SYMBOLS.  Every live node has a symbol s in [0, 32), taken from ``decode(type, value, False, var_len, 1)``: the function ids 0 .. 28; a
ternary-typed node is IF (0) whatever its id, as the interpreters treat it; VAR is 29, CONST 30; a unary or binary node whose id is no
function of its class is UNKNOWN, 31.

PARAMETERS.  ``cost[32]`` int32, each in [0, 65535].  ``operand_limit[32][3]`` int32, -1 for none, else >= 0.  R rules, 0 <= R <= 8,
each (outer_mask, inner_mask, limit): the masks are 32-bit sets of symbols (bit s = symbol s; held as int32 words), limit in [0, 254].
``max_depth`` and ``max_complexity``: -1 for none.

PASS UP, from the last live node to node 0 (a sum or a max over no children is 0).  Operand order is interp.hpp's: the first child of
node i is node i + 1, the second follows the first's subtree, the third the second's.
  complexity[i] = cost[s_i] + sum of complexity[child]                  (int32; cannot overflow: 65535 * 1024 < 2^31)
  height[i]     = 1 + max height[child]                                 (a leaf has height 1)
  for rule r:     below_r = max nest_r[child];  nest_r[i] = min(255, below_r + [s_i in inner_r])
  NEST          when s_i in outer_r and below_r > limit_r for some r
  OPERAND       when for some operand k operand_limit[s_i][k] >= 0 and complexity[child_k] > operand_limit[s_i][k]
THE ROOT.  max_depth >= 0 and height[0] > max_depth sets DEPTH on node 0; max_complexity >= 0 and complexity[0] > max_complexity sets
COMPLEXITY on node 0.
PASS DOWN, from node 0 to the last live node: depth[0] = 0, depth[child] = depth[i] + 1.

FLAGS per node: NEST 1, OPERAND 2, MALFORMED 4, DEPTH 8, COMPLEXITY 16.  ``violations`` = (the nodes with NEST or OPERAND, each counted
once) + [DEPTH] + [COMPLEXITY].

MALFORMED ROWS are judged by interval_ref.tree_intervals' rule (stack discipline plus verified size words), as dimension_ref does:
MALFORMED on every live word (on word 0 when the row has none), 0 in every other output, violations = -1.  Words past the live prefix
are 0.  With every cost 1, complexity equals subtree_size on every live node of a well-formed row."""
import numpy as np

from sr_grad_ref import decode
from subtree_ref import live_len, well_formed

N_SYMBOLS = 32
VAR, CONST, UNKNOWN = 29, 30, 31
NEST, OPERAND, MALFORMED, DEPTH, COMPLEXITY = 1, 2, 4, 8, 16
MAX_RULES = 8
ARITY = {"C": 0, "V": 0, "U": 1, "B": 2, "T": 3}


def symbol(type_word, value_word):
    """(symbol, arity) of one node"""
    kind, pay, _ = decode(type_word, value_word, False, 1, 1)
    if kind == "C":
        return CONST, 0
    if kind == "V":
        return VAR, 0
    if kind == "T":
        return 0, 3
    return (UNKNOWN if pay is None else int(pay)), ARITY[kind]


def tree_structure(value, type_, size, cost, operand_limit, rules, max_depth, max_complexity):
    """one row -> (complexity (L,), height (L,), depth (L,), nest (L, R), flags (L,), violations); rules: [(outer, inner, limit)] with
    the masks as non-negative ints"""
    L, R = len(value), len(rules)
    cx, ht, dp = np.zeros(L, np.int32), np.zeros(L, np.int16), np.zeros(L, np.int16)
    nest, flags = np.zeros((L, R), np.uint8), np.zeros(L, np.uint8)
    n = live_len(size, L)
    ok = well_formed(type_, n)
    count = 0
    kids = [None] * n
    if ok:
        for i in reversed(range(n)):
            s, arity = symbol(type_[i], value[i])
            ks = []
            c = i + 1
            for _ in range(arity):
                ks.append(c)
                c += int(size[c])
            if int(size[i]) != c - i:
                ok = False
                break
            kids[i] = ks
            cx[i] = int(cost[s]) + sum(int(cx[k]) for k in ks)
            ht[i] = 1 + max([int(ht[k]) for k in ks], default=0)
            f = 0
            for r, (outer, inner, limit) in enumerate(rules):
                below = max([int(nest[k, r]) for k in ks], default=0)
                nest[i, r] = min(255, below + ((inner >> s) & 1))
                if (outer >> s) & 1 and below > limit:
                    f |= NEST
            for k, kid in enumerate(ks):
                lim = int(operand_limit[s][k])
                if lim >= 0 and int(cx[kid]) > lim:
                    f |= OPERAND
            flags[i] = f
            count += 1 if f else 0
    if not ok:
        cx[:], ht[:], dp[:], nest[:], flags[:] = 0, 0, 0, 0, 0
        flags[:max(n, 1)] = MALFORMED
        return cx, ht, dp, nest, flags, -1
    if max_depth >= 0 and int(ht[0]) > max_depth:
        flags[0] |= DEPTH
        count += 1
    if max_complexity >= 0 and int(cx[0]) > max_complexity:
        flags[0] |= COMPLEXITY
        count += 1
    for i in range(n):
        for k in kids[i]:
            dp[k] = dp[i] + 1
    return cx, ht, dp, nest, flags, count


def as_tables(cost, operand_limit, rule_outer, rule_inner, rule_limit):
    """the op's tensors as (cost (32,), operand_limit (32, 3), [(outer, inner, limit)]): the mask words taken as unsigned"""
    cost = np.asarray(cost, np.int64).reshape(N_SYMBOLS)
    operand_limit = np.asarray(operand_limit, np.int64).reshape(N_SYMBOLS, 3)
    outer, inner, limit = (np.asarray(a, np.int64).reshape(-1) for a in (rule_outer, rule_inner, rule_limit))
    assert len(outer) == len(inner) == len(limit) <= MAX_RULES
    assert ((cost >= 0) & (cost <= 65535)).all() and (operand_limit >= -1).all() and ((limit >= 0) & (limit <= 254)).all()
    rules = [(int(o) & 0xFFFFFFFF, int(i) & 0xFFFFFFFF, int(l)) for o, i, l in zip(outer, inner, limit)]
    return cost, operand_limit, rules


def forest_structure(value, type_, size, cost, operand_limit, rule_outer=(), rule_inner=(), rule_limit=(), max_depth=-1, max_complexity=-1):
    value, type_, size = np.asarray(value, np.float32), np.asarray(type_, np.int16), np.asarray(size, np.int16)
    cost, operand_limit, rules = as_tables(cost, operand_limit, rule_outer, rule_inner, rule_limit)
    pop, L = value.shape
    R = len(rules)
    cx, ht, dp = np.zeros((pop, L), np.int32), np.zeros((pop, L), np.int16), np.zeros((pop, L), np.int16)
    nest, flags, viol = np.zeros((pop, L, R), np.uint8), np.zeros((pop, L), np.uint8), np.zeros(pop, np.int32)
    for t in range(pop):
        cx[t], ht[t], dp[t], nest[t], flags[t], viol[t] = tree_structure(value[t], type_[t], size[t], cost, operand_limit, rules,
                                                                         int(max_depth), int(max_complexity))
    return cx, ht, dp, nest, flags, viol


def unit_cost():
    return np.ones(N_SYMBOLS, np.int32)


def no_operand_limit():
    return np.full((N_SYMBOLS, 3), -1, np.int32)


def mask_word(symbols):
    """a set of symbols as the int32 word the op takes (bit 31 gives a negative word)"""
    m = 0
    for s in symbols:
        m |= 1 << int(s)
    return int(np.uint32(m).view(np.int32))
