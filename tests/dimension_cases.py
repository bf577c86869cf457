"""TEST-ONLY: the hand table and the random trees shared by the dimension tests (tests/test_dimension_ref.py,
tests/test_gpu_dimensions.py).  K = 2 base dimensions (m, s) unless a case brings its own variables."""
import numpy as np

import sr_grad_ref as R
from interval_cases import B, C, IF, U, V, rows

DEN = 25200
LIM = 1 << 24
M, S, MPS, ONE = (DEN, 0), (0, DEN), (DEN, -DEN), (0, 0)
VARS = [M, S, MPS, ONE]                      # x0 metres, x1 seconds, x2 metres per second, x3 a pure number
LABELS = [None, M, (DEN, -2 * DEN), ONE]     # none (check_root off), m, m / s^2, 1
HALF_M = (DEN // 2, 0)
NAN, INF = float("nan"), float("inf")

TRANSCENDENTAL = list(range(R.F_SIN, R.F_EXP + 1))


def nest(f, depth, leaf, second=None):
    """f(f(.. f(leaf) ..)); a binary f takes ``second`` as its other operand"""
    e = leaf
    for _ in range(depth):
        e = U(f, e) if second is None else B(f, e, second)
    return e


def case(name, expr, label, viol, root=None, consts=None, var_units=VARS, flags=None):
    """expr: an expression or a node list; label None: check_root off; viol: the expected count; root: the expected unit of node 0;
    consts: {node index: expected unit}; flags: {node index: expected flag byte}"""
    return dict(name=name, expr=expr, label=label, viol=viol, root=root, consts=consts or {}, var_units=var_units, flags=flags or {})


BIG = [(1 << 23, 0), (LIM, -LIM), (1, 0)]     # variables at the edge of the range, and one with an odd numerator

TABLE = [
    # ---- leaves, the root ----
    case("a variable alone", V(0), M, 0, root=M),
    case("a variable against another label", V(0), S, 1, root=M, flags={0: 8}),
    case("check_root off", V(0), None, 0, root=M),
    case("a constant takes the label", C(1.0), (DEN, -2 * DEN), 0, root=(DEN, -2 * DEN), consts={0: (DEN, -2 * DEN)}, flags={0: 1}),
    case("a free root without a label is dimensionless", C(1.0), None, 0, root=ONE),
    case("clamped variable indices", B(R.F_ADD, B(R.F_ADD, V(-3), V(0)), B(R.F_MUL, V(99), V(0))), M, 0, root=M),
    case("a clamped index that differs", B(R.F_ADD, V(99), V(0)), None, 1),
    # ---- + - max min, if ----
    case("m + m", B(R.F_ADD, V(0), V(0)), M, 0, root=M),
    case("m + s", B(R.F_ADD, V(0), V(1)), None, 1, flags={0: 2}),
    case("m - c", B(R.F_SUB, V(0), C(2.0)), M, 0, consts={2: M}),
    case("c - s", B(R.F_SUB, C(2.0), V(1)), None, 0, root=S, consts={1: S}),
    case("c - c under a label", B(R.F_SUB, C(2.0), C(1.0)), S, 0, consts={1: S, 2: S}, flags={0: 1}),
    case("max(m, s)", B(R.F_MAX, V(0), V(1)), None, 1),
    case("min(s, c)", B(R.F_MIN, V(1), C(0.0)), S, 0, consts={2: S}),
    case("if: any condition, equal branches", IF(V(1), V(0), V(0)), M, 0, root=M),
    case("if: branches differ", IF(C(1.0), V(0), V(1)), None, 1),
    case("if: a free condition is a number", IF(C(1.0), C(2.0), V(0)), M, 0, consts={1: ONE, 2: M}),
    case("if: all free", IF(C(1.0), C(2.0), C(3.0)), S, 0, consts={1: ONE, 2: S, 3: S}),
    case("a ternary node with another id", IF(V(3), V(2), V(2), fid=7), MPS, 0, root=MPS),
    # ---- comparisons ----
    case("m < s", B(R.F_LT, V(0), V(1)), None, 1, root=ONE),
    case("m > c", B(R.F_GT, V(0), C(1.0)), ONE, 0, root=ONE, consts={2: M}),
    case("c <= m/s", B(R.F_LE, C(1.0), V(2)), ONE, 0, consts={1: MPS}),
    case("c >= c", B(R.F_GE, C(1.0), C(2.0)), ONE, 0, consts={1: ONE, 2: ONE}),
    case("a comparison is a number", B(R.F_LT, V(0), V(0)), M, 1, root=ONE, flags={0: 8}),
    # ---- * / loose_div ----
    case("m * s", B(R.F_MUL, V(0), V(1)), (DEN, DEN), 0, root=(DEN, DEN)),
    case("m / s", B(R.F_DIV, V(0), V(1)), MPS, 0, root=MPS),
    case("m / s is no length", B(R.F_DIV, V(0), V(1)), M, 1, flags={0: 8}),
    case("loose_div(m, m/s)", B(R.F_LOOSE_DIV, V(0), V(2)), S, 0, root=S),
    case("c * s = m", B(R.F_MUL, C(3.0), V(1)), M, 0, consts={1: MPS}),
    case("s * c = m", B(R.F_MUL, V(1), C(3.0)), M, 0, consts={2: MPS}),
    case("c / s = m", B(R.F_DIV, C(3.0), V(1)), M, 0, consts={1: (DEN, DEN)}),
    case("m / c = s", B(R.F_DIV, V(0), C(3.0)), S, 0, consts={2: MPS}),
    case("c * c", B(R.F_MUL, C(3.0), C(2.0)), M, 0, consts={1: M, 2: ONE}),
    case("loose_div(c, c)", B(R.F_LOOSE_DIV, C(3.0), C(2.0)), M, 0, consts={1: M, 2: ONE}),
    case("m + c * s", B(R.F_ADD, V(0), B(R.F_MUL, C(2.0), V(1))), M, 0, consts={3: MPS}),
    case("a product at the edge of the range", B(R.F_MUL, V(0), V(0)), None, 0, root=(LIM, 0), var_units=BIG),
    case("a product past the range", B(R.F_MUL, B(R.F_MUL, V(0), V(0)), V(0)), None, 1, root=ONE, var_units=BIG, flags={0: 2}),
    case("a quotient past the range", B(R.F_DIV, V(1), U(R.F_INV, V(1))), None, 1, root=ONE, var_units=BIG),
    case("a demand past the range", B(R.F_MUL, C(1.0), V(1)), (-LIM, LIM), 1, consts={1: ONE}, var_units=BIG, flags={0: 1, 1: 3}),
    # ---- neg abs inv sqrt ----
    case("neg abs", U(R.F_NEG, U(R.F_ABS, V(2))), MPS, 0, root=MPS),
    case("neg of a constant", U(R.F_NEG, C(1.0)), M, 0, consts={1: M}),
    case("1 / s", U(R.F_INV, V(1)), (0, -DEN), 0, root=(0, -DEN)),
    case("loose_inv(c) = s", U(R.F_LOOSE_INV, C(1.0)), S, 0, consts={1: (0, -DEN)}),
    case("sqrt(m * m)", U(R.F_SQRT, B(R.F_MUL, V(0), V(0))), M, 0, root=M),
    case("sqrt(m)", U(R.F_LOOSE_SQRT, V(0)), HALF_M, 0, root=HALF_M),
    case("sqrt(c) = m", U(R.F_SQRT, C(1.0)), M, 0, consts={1: (2 * DEN, 0)}),
    case("an odd numerator under sqrt", U(R.F_SQRT, V(2)), None, 1, root=ONE, var_units=BIG, flags={0: 2}),
    case("four nested square roots of m stay exact", nest(R.F_SQRT, 4, V(0)), None, 0, root=(DEN // 16, 0)),
    case("the fifth does not", nest(R.F_SQRT, 5, V(0)), None, 1, root=ONE),
    case("nested sqrt overflows the demand in pass 2", nest(R.F_SQRT, 10, C(1.0)), M, 1, flags={9: 1, 10: 3}),
    case("nine nested sqrt do not", nest(R.F_SQRT, 9, C(1.0)), M, 0, consts={9: (DEN << 9, 0)}),
    # ---- the transcendentals ----
    case("sin of a number", U(R.F_SIN, V(3)), ONE, 0, root=ONE),
    case("sin of a length", U(R.F_SIN, V(0)), None, 1, root=ONE),
    case("exp(m / m)", U(R.F_EXP, B(R.F_DIV, V(0), V(0))), ONE, 0),
    case("log(c * s)", U(R.F_LOG, B(R.F_MUL, C(2.0), V(1))), ONE, 0, consts={2: (0, -DEN)}),
    case("cosh(c)", U(R.F_COSH, C(2.0)), ONE, 0, consts={1: ONE}),
    case("a transcendental is a number", U(R.F_TANH, V(3)), M, 1, flags={0: 8}),
    # ---- pow loose_pow ----
    case("pow(m, 2)", B(R.F_POW, V(0), C(2.0)), (2 * DEN, 0), 0, root=(2 * DEN, 0), consts={2: ONE}),
    case("pow(m, 0.5)", B(R.F_POW, V(0), C(0.5)), HALF_M, 0, root=HALF_M),
    case("pow(m, 0.3)", B(R.F_POW, V(0), C(0.3)), None, 1, root=ONE, flags={0: 2}),
    case("loose_pow(m/s, -1.5)", B(R.F_LOOSE_POW, V(2), C(-1.5)), None, 0, root=(-3 * DEN // 2, 3 * DEN // 2)),
    case("a NaN exponent", B(R.F_POW, V(0), C(NAN)), None, 1, root=ONE),
    case("an infinite exponent", B(R.F_POW, V(0), C(INF)), None, 1, root=ONE),
    case("pow(m, 0) is a number", B(R.F_POW, V(0), C(0.0)), ONE, 0, root=ONE),
    case("pow(m, x)", B(R.F_POW, V(0), V(3)), None, 1),
    case("pow(m, c + c)", B(R.F_POW, V(0), B(R.F_ADD, C(1.0), C(1.0))), None, 1),
    case("pow(1, s)", B(R.F_POW, V(3), V(1)), None, 1),
    case("pow(1, 1)", B(R.F_LOOSE_POW, V(3), V(3)), ONE, 0),
    case("pow(c, c)", B(R.F_POW, C(2.0), C(3.0)), ONE, 0, consts={1: ONE, 2: ONE}),
    case("pow(m, s): one node, one violation", B(R.F_POW, V(0), V(1)), None, 1),
    case("repeated squaring leaves the range in pass 1", nest(R.F_POW, 10, V(0), C(2.0)), None, 1, root=ONE, flags={0: 2, 1: 0}),
    case("nine squarings do not", nest(R.F_POW, 9, V(0), C(2.0)), None, 0, root=(DEN << 9, 0)),
    case("the gap: pow over a free base", B(R.F_POW, B(R.F_MUL, C(1.0), V(0)), C(2.0)), (2 * DEN, 0), 1, flags={0: 8}),
    # ---- unknown function ids ----
    case("a unary node with a binary id", U(5, V(0)), ONE, 0, root=ONE),
    case("a binary node with a unary id", B(20, V(0), V(1)), ONE, 0, root=ONE),
    case("an unknown id over constants", B(77, C(1.0), U(40, C(2.0))), ONE, 0, consts={1: ONE, 3: ONE}),
    case("an unknown id is a number", U(R.F_NEG, U(40, V(0))), M, 1, flags={0: 8}),
]


def table_rows(L=32):
    """one call per case (the label and the variables' units belong to the call):
    [(case, value, type, size, var_units int32, label int32, check_root)]"""
    out = []
    for c in TABLE:
        value, type_, size = rows([c["expr"]], L)
        label = np.array(c["label"] if c["label"] is not None else (0, 0), np.int32)
        out.append((c, value, type_, size, np.array(c["var_units"], np.int32), label, c["label"] is not None))
    return out


def malformed_rows(L=8):
    """five rows: a good one, a bad size word, a stack underflow, an empty row, a length beyond the row; then a full row (n == L)"""
    good = B(R.F_ADD, B(R.F_MUL, V(0), C(2.0)), V(0))
    value, type_, size = rows([good] * 5 + [nest(R.F_NEG, L - 1, V(0))], L)
    size[1, 1] = 2            # the size word of the product is not its subtree's size
    type_[2, 4] = 3           # the last leaf becomes a binary node: underflow
    size[3, 0] = 0            # empty
    size[4, 0] = L + 5        # clamped to L: the zero words past the tree are VAR 0 leaves, so the prefix is no single tree
    return value, type_, size


# ---- random trees for the soundness / completeness runs ----
CONSTS = [0.5, 2.0, 3.0, -1.0, 1.5, 0.3]
_CLASSES = [
    ("same", [R.F_ADD, R.F_SUB, R.F_MAX, R.F_MIN], 3.0),
    ("product", [R.F_MUL, R.F_DIV, R.F_LOOSE_DIV], 5.0),
    ("compare", [R.F_LT, R.F_GT, R.F_LE, R.F_GE], 1.0),
    ("pow", [R.F_POW, R.F_LOOSE_POW], 1.0),
    ("if", [R.F_IF], 1.0),
    ("sign", [R.F_NEG, R.F_ABS], 1.0),
    ("inv", [R.F_INV, R.F_LOOSE_INV], 1.0),
    ("sqrt", [R.F_SQRT, R.F_LOOSE_SQRT], 1.0),
    ("transcendental", TRANSCENDENTAL, 1.0),
]
_WEIGHTS = np.array([w for _, _, w in _CLASSES]) / sum(w for _, _, w in _CLASSES)


def random_expr(rng, max_depth=3, const_prob=0.35, depth=0):
    """a random tree of depth <= max_depth over every operator class"""
    if depth >= max_depth or (depth > 0 and rng.random() < 0.3):
        return C(CONSTS[int(rng.integers(len(CONSTS)))]) if rng.random() < const_prob else V(int(rng.integers(len(VARS))))
    _, fs, _ = _CLASSES[int(rng.choice(len(_CLASSES), p=_WEIGHTS))]
    f = int(fs[int(rng.integers(len(fs)))])
    kid = lambda: random_expr(rng, max_depth, const_prob, depth + 1)   # noqa: E731
    if f == R.F_IF:
        return IF(kid(), kid(), kid())
    if f >= R.F_SIN:
        return U(f, kid())
    return B(f, kid(), kid())


def random_dim_forest(rng, pop, L, var_len, funcs=None, max_depth=5):
    """random trees over all 29 functions (plus a few unknown ids) for the word-for-word runs: constants from CONSTS, NaN and inf among them"""
    from grad_trees import ALL_FUNCS, random_tree

    exprs = []
    for t in range(pop):
        while True:
            nodes = random_tree(rng, funcs or ALL_FUNCS, var_len, 1, int(rng.integers(1, max_depth + 1)))
            if len(nodes) <= L:
                break
        for nd in nodes:
            if nd[1] == R.T_CONST:
                nd[0] = np.float32(rng.choice(CONSTS + [1.0, 4.0, NAN, INF]))
            elif nd[1] >= 2 and rng.random() < 0.02:
                nd[0] = np.float32(rng.choice([0.0, 40.0, 77.0]))     # an id that is unknown for most arities
        exprs.append(nodes)
    return rows(exprs, L)


def random_units(rng, var_len, K):
    """(var_len, K) int32 numerators: multiples of DEN / 2 mostly, a few odd or large ones"""
    u = rng.integers(-2, 3, (var_len, K)) * (DEN // 2)
    odd = rng.random((var_len, K)) < 0.05
    u = np.where(odd, rng.integers(-LIM, LIM + 1, (var_len, K)), u)
    return u.astype(np.int32)

