"""TEST-ONLY: the hand table, the random trees and the random parameters shared by the structure tests (tests/test_structure_ref.py,
tests/test_gpu_structure.py).  Every expected figure of the table is worked out by hand from the definition (tests/structure_ref.py)."""
import numpy as np

import sr_grad_ref as R
import structure_ref as SR
from interval_cases import B, C, IF, U, V, rows

VAR, CONST, UNKNOWN = SR.VAR, SR.CONST, SR.UNKNOWN
SIN, COS, POW, ADD, MUL, NEG = R.F_SIN, R.F_COS, R.F_POW, R.F_ADD, R.F_MUL, R.F_NEG


def params(cost=None, oplim=None, rules=(), max_depth=-1, max_complexity=-1):
    """cost {symbol: cost} over unit costs; oplim {symbol: limits}; rules [(outer symbols, inner symbols, limit)] -> the op's arguments
    (cost, operand_limit, rule_outer, rule_inner, rule_limit, max_depth, max_complexity)"""
    c, o = SR.unit_cost(), SR.no_operand_limit()
    for s, x in (cost or {}).items():
        c[s] = x
    for s, lims in (oplim or {}).items():
        for k, x in enumerate(lims):
            o[s, k] = x
    outer = np.array([SR.mask_word(r[0]) for r in rules], np.int32)
    inner = np.array([SR.mask_word(r[1]) for r in rules], np.int32)
    limit = np.array([r[2] for r in rules], np.int32)
    return c, o, outer, inner, limit, int(max_depth), int(max_complexity)


def case(name, expr, viol, flags=None, cx=None, height=None, nest=None, **kw):
    """viol: the expected count; flags: {node: flag byte} (every other live node: 0); cx / height: of the root; nest: {node: [R
    counters]}"""
    return dict(name=name, expr=expr, viol=viol, flags=flags or {}, cx=cx, height=height, nest=nest or {}, params=params(**kw))


X, Y = V(0), V(1)
SQ = lambda e: B(POW, e, C(2.0))   # noqa: E731
NO_TRIG_IN_SIN = [([SIN], [SIN], 0), ([SIN], [COS], 0)]
POW_ONCE = [([POW], [POW], 1)]

TABLE = [
    # ---- no constraint at all ----
    case("a leaf", X, 0, cx=1, height=1),
    case("unit costs give the size", B(ADD, U(SIN, X), B(MUL, X, C(2.0))), 0, cx=6, height=3),
    # ---- DEPTH alone ----
    case("height 3 under max_depth 2", B(ADD, X, B(MUL, X, Y)), 1, {0: 8}, height=3, max_depth=2),
    case("height 3 under max_depth 3", B(ADD, X, B(MUL, X, Y)), 0, height=3, max_depth=3),
    case("a leaf under max_depth 0", C(1.0), 1, {0: 8}, height=1, max_depth=0),
    case("the deepest path is the third operand", IF(X, Y, U(NEG, U(NEG, X))), 1, {0: 8}, height=4, max_depth=3),
    # ---- COMPLEXITY alone ----
    case("sin costs 3: 6 > 5", B(ADD, U(SIN, X), X), 1, {0: 16}, cx=6, cost={SIN: 3}, max_complexity=5),
    case("sin costs 3: 6 <= 6", B(ADD, U(SIN, X), X), 0, cx=6, cost={SIN: 3}, max_complexity=6),
    case("variables 2, constants 3, + free", B(ADD, X, C(1.0)), 0, cx=5, cost={VAR: 2, CONST: 3, ADD: 0}, max_complexity=5),
    case("max_complexity 0", X, 1, {0: 16}, cx=1, max_complexity=0),
    case("the largest cost", U(SIN, U(SIN, X)), 0, cx=131071, cost={SIN: 65535}),
    # ---- OPERAND alone ----
    case("pow(x, 2) under (-1, 1)", SQ(X), 0, oplim={POW: (-1, 1)}),
    case("pow(x, c + c) under (-1, 1)", B(POW, X, B(ADD, C(1.0), C(1.0))), 1, {0: 2}, oplim={POW: (-1, 1)}),
    case("pow(x + x, 2) under (1, -1): the first operand", B(POW, B(ADD, X, X), C(2.0)), 1, {0: 2}, oplim={POW: (1, -1)}),
    case("pow(x + x, 2) under (3, 1)", B(POW, B(ADD, X, X), C(2.0)), 0, oplim={POW: (3, 1)}),
    case("sin(x + x) under 2", U(SIN, B(ADD, X, X)), 1, {0: 2}, oplim={SIN: (2,)}),
    case("sin(neg x) under 2", U(SIN, U(NEG, X)), 0, oplim={SIN: (2,)}),
    case("the third operand of if", IF(X, Y, U(NEG, X)), 1, {0: 2}, oplim={R.F_IF: (-1, -1, 1)}),
    case("the second operand of if", IF(X, U(NEG, Y), X), 1, {0: 2}, oplim={R.F_IF: (-1, 1, -1)}),
    case("a limit of 0 under free leaves", B(POW, X, Y), 0, oplim={POW: (0, 0)}, cost={VAR: 0}),
    case("the limit is on the weighted complexity", B(POW, X, C(2.0)), 1, {0: 2}, oplim={POW: (-1, 1)}, cost={CONST: 2}),
    case("an inner node, not the root", U(NEG, B(POW, X, B(ADD, X, X))), 1, {1: 2}, oplim={POW: (-1, 1)}),
    case("two nodes", B(POW, B(POW, X, U(NEG, X)), U(NEG, X)), 2, {0: 2, 1: 2}, oplim={POW: (-1, 1)}),
    # ---- NEST alone ----
    case("sin(sin x)", U(SIN, U(SIN, X)), 1, {0: 1}, nest={0: [2, 0], 1: [1, 0], 2: [0, 0]}, rules=NO_TRIG_IN_SIN),
    case("sin(cos x)", U(SIN, U(COS, X)), 1, {0: 1}, nest={0: [1, 1], 1: [0, 1]}, rules=NO_TRIG_IN_SIN),
    case("cos(sin x)", U(COS, U(SIN, X)), 0, nest={0: [1, 1], 1: [1, 0]}, rules=NO_TRIG_IN_SIN),
    case("sin x + sin x", B(ADD, U(SIN, X), U(SIN, X)), 0, nest={0: [1, 0]}, rules=NO_TRIG_IN_SIN),
    case("sin(x + neg(cos x)): the path through the second operand", U(SIN, B(ADD, X, U(NEG, U(COS, X)))), 1, {0: 1},
         nest={0: [1, 1], 1: [0, 1]}, rules=NO_TRIG_IN_SIN),
    case("a tower: every sine but the innermost", U(SIN, U(SIN, U(SIN, X))), 2, {0: 1, 1: 1}, rules=NO_TRIG_IN_SIN),
    case("the path through the third operand", IF(X, Y, U(SIN, U(SIN, X))), 1, {0: 1}, nest={0: [2]}, rules=[([R.F_IF], [SIN], 1)]),
    case("the third operand, within the limit", IF(X, Y, U(SIN, U(SIN, X))), 0, nest={0: [2]}, rules=[([R.F_IF], [SIN], 2)]),
    case("only the second rule fires", U(SIN, U(COS, X)), 1, {0: 1}, rules=[([SIN], [SIN], 0), ([SIN], [COS], 0)]),
    case("a set of inner symbols counts them together", U(SIN, U(COS, U(SIN, X))), 1, {0: 1}, nest={0: [3], 1: [2]},
         rules=[([SIN], [SIN, COS], 1)]),
    case("a set of outer symbols", U(COS, U(NEG, U(SIN, X))), 1, {0: 1}, rules=[([SIN, COS], [SIN], 0)]),
    case("leaves as inner symbols", B(ADD, X, C(1.0)), 1, {0: 1}, nest={0: [1], 1: [1], 2: [0]}, rules=[([ADD], [VAR], 0)]),
    # ---- outer == inner at limits 0 and 1 ----
    case("pow in pow, limit 1", SQ(SQ(X)), 0, nest={0: [2], 1: [1]}, rules=POW_ONCE),
    case("pow in pow in pow, limit 1: the outermost only", SQ(SQ(SQ(X))), 1, {0: 1}, nest={0: [3], 1: [2], 2: [1], 3: [0]}, rules=POW_ONCE),
    case("pow in pow, limit 0", SQ(SQ(X)), 1, {0: 1}, rules=[([POW], [POW], 0)]),
    case("pow in pow in pow, limit 0: the outer two", SQ(SQ(SQ(X))), 2, {0: 1, 1: 1}, rules=[([POW], [POW], 0)]),
    case("a single pow, limit 0", SQ(X), 0, nest={0: [1]}, rules=[([POW], [POW], 0)]),
    case("pow in the exponent", B(POW, X, SQ(Y)), 1, {0: 1}, rules=[([POW], [POW], 0)]),
    # ---- more than one cause ----
    case("NEST and OPERAND on one node count once", B(POW, SQ(X), B(ADD, X, X)), 1, {0: 3}, rules=[([POW], [POW], 0)], oplim={POW: (-1, 1)}),
    case("every flag at the root", B(POW, SQ(X), B(ADD, X, X)), 3, {0: 27}, cx=7, height=3, rules=[([POW], [POW], 0)],
         oplim={POW: (-1, 1)}, max_depth=2, max_complexity=6),
    case("DEPTH and COMPLEXITY, NEST below", U(NEG, U(SIN, U(SIN, X))), 3, {0: 24, 1: 1}, rules=NO_TRIG_IN_SIN, max_depth=3, max_complexity=3),
    # ---- the symbols ----
    case("a ternary node with another id is IF", IF(X, Y, X, fid=7), 1, {0: 3}, cx=13, cost={R.F_IF: 10, R.F_LOOSE_POW: 100},
         rules=[([R.F_IF], [VAR], 0)], oplim={R.F_IF: (0, -1, -1)}),
    case("a unary node with a binary id is UNKNOWN", U(5, X), 1, {0: 16}, cx=8, cost={UNKNOWN: 7, R.F_LOOSE_DIV: 100}, max_complexity=7),
    case("a binary node with a unary id is UNKNOWN", B(20, X, U(SIN, Y)), 1, {0: 1}, nest={0: [1, 1]},
         rules=[([UNKNOWN], [SIN], 0), ([SIN], [UNKNOWN], 0)]),
    case("UNKNOWN as an inner symbol", U(SIN, U(77, X)), 1, {0: 1}, rules=[([SIN], [UNKNOWN], 0)]),
    case("UNKNOWN's operands", B(40, X, U(NEG, Y)), 1, {0: 2}, oplim={UNKNOWN: (-1, 1)}),
]


def table_rows(L=16):
    """one call per case: [(case, value, type, size)]"""
    return [(c,) + rows([c["expr"]], L) for c in TABLE]


# ---- random trees and parameters ----
def random_forest(rng, pop, L, max_depth=5, funcs=None):
    """random trees over all 29 functions, unknown ids among them"""
    from grad_trees import ALL_FUNCS, random_tree

    exprs = []
    for t in range(pop):
        while True:
            nodes = random_tree(rng, funcs or ALL_FUNCS, 3, 1, int(rng.integers(1, max_depth + 1)))
            if len(nodes) <= L:
                break
        for nd in nodes:
            if nd[1] >= 2 and rng.random() < 0.03:
                nd[0] = np.float32(rng.choice([0.0, 5.0, 20.0, 40.0, 77.0]))     # an id that is unknown for most arities
        exprs.append(nodes)
    return rows(exprs, L)


def random_params(rng, R_=None, tight=False):
    """random costs, 0 .. 8 random rules and random limits; ``tight``: limits near what trees of depth <= 5 reach, so that a forest
    holds passing and violating trees alike"""
    n_rules = int(rng.integers(0, 9)) if R_ is None else R_
    cost = rng.integers(0, 4, 32) if rng.random() < 0.7 else rng.integers(0, 65536, 32)
    if rng.random() < 0.3:
        cost[rng.integers(0, 32, 4)] = 65535
    oplim = np.full((32, 3), -1, np.int64)
    pick = rng.random((32, 3)) < (0.1 if tight else 0.3)
    typical = int(np.median(cost)) + 1
    oplim[pick] = rng.integers(0, (12 if tight else 6) * typical, int(pick.sum()))
    outer = rng.integers(0, 1 << 32, n_rules, dtype=np.uint64) & rng.integers(0, 1 << 32, n_rules, dtype=np.uint64)
    inner = rng.integers(0, 1 << 32, n_rules, dtype=np.uint64) & rng.integers(0, 1 << 32, n_rules, dtype=np.uint64)
    if tight:
        outer &= rng.integers(0, 1 << 32, n_rules, dtype=np.uint64)
    limit = np.where(rng.random(n_rules) < 0.9, rng.integers(0, 3, n_rules) + (2 if tight else 0), rng.integers(0, 255, n_rules))
    total = float(np.mean(cost)) * 12
    max_depth = -1 if rng.random() < 0.3 else int(rng.integers(5, 7) if tight else rng.integers(0, 7))
    max_complexity = -1 if rng.random() < 0.3 else int(rng.integers(int(total) + 1, 4 * int(total) + 2) if tight else rng.integers(0, 2 * int(total) + 2))
    return (cost.astype(np.int32), oplim.astype(np.int32), outer.astype(np.uint32).view(np.int32), inner.astype(np.uint32).view(np.int32),
            limit.astype(np.int32), max_depth, max_complexity)


def unary_chain(n, f=SIN):
    """f(f(.. f(x) ..)) of n nodes as a node list (built without recursion)"""
    return [[np.float32(f), 2, n - k] for k in range(n - 1)] + [[np.float32(0), R.T_VAR, 1]]


def right_comb(depth, f=ADD, inner=SIN):
    """f(l, f(l, .. f(l, l))) with every other leaf wrapped in ``inner``: children 2 at far offsets"""
    nodes = []
    leaf = lambda k: [[np.float32(inner), 2, 2], [np.float32(k % 3), R.T_VAR, 1]] if k % 2 else [[np.float32(k % 3), R.T_VAR, 1]]   # noqa: E731
    leaves = [leaf(k) for k in range(depth + 1)]
    n = depth + sum(len(l) for l in leaves)
    used = 0
    for k in range(depth):
        nodes.append([np.float32(f), 3, n - used])
        nodes += leaves[k]
        used += 1 + len(leaves[k])
    return nodes + leaves[depth]
