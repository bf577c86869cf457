"""TEST-ONLY: the adjoint battery -- probe trees that read ONE rule of DESIGN.md's "Constant gradients" table directly off a gradient
word, their float64 truth, the planted edge cells of the table with their exact expectations, the per-function operand draws, and
the derived error unit of every rule.  No GPU import: tests/test_adjoint_battery.py checks all of it against the references on the
CPU, tests/test_gpu_sr_adjoint.py runs it on the device.

Probe trees.  D = 1, MAE, every operand of the probed function f a CONST node:
    direct    f(c) / f(c0, c1) / IF(c0, c1, c2)                         a = node 1 (the first popped), b = node 2, c = node 3
    stacked   f(ADD(c, x0)) / f(ADD(c0, x0), ADD(c1, x0)) / ... with x0 = 0: the rule's output is STORED in the ADD's adjoint slot and a
              second rule (ADD) carries it to the CONST accumulator.  ADD(c, 0) turns -0 into +0: `effective_operands` gives the truth
              the same operands.  Multi-output: a function node without the OUT flag hands its LAST operand on unchanged, so the
              stacked form is f(ADD(x0, c)) there and -0 stays -0.
The label of a launch is shared by all its trees, so it is the least value of  pred_ref - max(1, 2 |pred_ref|)  over the trees whose
float64 prediction is finite in fp32 (0 when there is none): pred - y > 0 on every one of them and the output adjoint is exactly 1.0f;
a tree whose prediction is +inf / -inf / NaN has the output adjoint +1 / -1 / NaN, which `out_adjoint` restates.  The gradient word at a
CONST operand is then the fp32 value of the rule itself, nothing summed or scaled (a -0 comes out as +0: the accumulator adds it to +0).

Truth.  sr_grad_ref's `unary` / `binary` / `unary_adjoint` / `binary_adjoint` and the IF rule, vectorised in float64 on the fp32 operands.

Error unit of a point (section "units"):   u = ulp32(truth) + sum over the library results x the rule reads |d rule / d x| BOUND[x] ulp32(x)
with BOUND from tests/ulp_bounds.py (the forward result r from the tape, and the rule's own cosf / sinf / coshf / sinhf / logf / powf
calls), plus, for the two powers, the rounding of the exponent b - 1 carried through powf.  CEILING is the a-priori bound in those
units: 0.5 per rounding fp32 operation of the rule as written (negation, sign, fabs and selects do not round; a contraction of
a * b + c into an fma removes a rounding, never adds one) plus 1 for the propagated terms."""
import zlib

import numpy as np

import sr_grad_ref as R
import sr_lm_ref as LM
from grad_trees import out_word
from ulp_bounds import BINARY as _ULP_BINARY, UNARY as _ULP_UNARY

C, V, U, B, T = R.T_CONST, R.T_VAR, R.T_UFUNC, R.T_BFUNC, 4
F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
DELTA = F32(1e-9)
DELTA_UP, DELTA_DN = np.nextafter(DELTA, F32(1)), np.nextafter(DELTA, F32(0))
DEN = F32(2.0 ** -149)                  # the smallest positive denormal
ONE_UP, ONE_DN = np.nextafter(F32(1), F32(2)), np.nextafter(F32(1), F32(0))
HALF_PI = F32(np.pi / 2)
N_DRAWS = 8192

# name -> (function id, arity); the two unknown ids decode to "function 0": value 0, every adjoint 0
FUNCS = {n: (getattr(R, "F_" + n), 2) for n in ("ADD SUB MUL DIV LOOSE_DIV POW LOOSE_POW MAX MIN LT GT LE GE").split()}
FUNCS.update({n: (getattr(R, "F_" + n), 1) for n in
              ("SIN COS TAN SINH COSH TANH LOG LOOSE_LOG EXP INV LOOSE_INV NEG ABS SQRT LOOSE_SQRT").split()})
FUNCS["IF"] = (R.F_IF, 3)
FUNCS["UNKNOWN_U"] = (99, 1)
FUNCS["UNKNOWN_B"] = (40, 2)
NAMES = list(FUNCS)
assert len(NAMES) == 31

# forward error bounds in ulps (tests/ulp_bounds.py, asserted by tests/test_gpu_ulp.py); + - * are correctly rounded, the rest is exact
FWD = {k: v[0] for k, v in _ULP_UNARY.items()}
FWD.update({k: v[0] for k, v in _ULP_BINARY.items()})
FWD.update(ADD=0.5, SUB=0.5, MUL=0.5)

# rules whose value is exact in fp32 for g = +-1: compared bit for bit on every route
EXACT = {"ADD", "SUB", "MAX", "MIN", "LT", "GT", "LE", "GE", "IF", "NEG", "ABS", "UNKNOWN_U", "UNKNOWN_B"}

# a-priori ceilings per operand, in units u: 0.5 per rounding operation of the rule as written + 1 for the propagated terms
#   SIN g*cos a: 1 op.  COS -g*sin a: 1.  TAN g*(1+r*r): 3.  SINH / COSH g*cosh a, g*sinh a: 1.  TANH g*(1-r*r): 3.  LOG / LOOSE_LOG g/a: 1.
#   EXP g*r: 1.  INV / LOOSE_INV -g*r*r: 2.  SQRT g*0.5/r: 2.  LOOSE_SQRT g*0.5/r*sign a: 3.  MUL g*b, g*a: 1.
#   DIV / LOOSE_DIV g/d: 1, -g*r/d: 2.
#   POW g*b*powf(a, b-1): 3 (two products and b-1), g*r*logf(a): 2.  LOOSE_POW the same with one more product (sign a): 4, 2.
CEILING = {
    "SIN": (1.5,), "COS": (1.5,), "TAN": (2.5,), "SINH": (1.5,), "COSH": (1.5,), "TANH": (2.5,), "LOG": (1.5,), "LOOSE_LOG": (1.5,),
    "EXP": (1.5,), "INV": (2.0,), "LOOSE_INV": (2.0,), "SQRT": (2.0,), "LOOSE_SQRT": (2.5,), "MUL": (1.5, 1.5), "DIV": (1.5, 2.0),
    "LOOSE_DIV": (1.5, 2.0), "POW": (2.5, 2.0), "LOOSE_POW": (3.0, 2.0),
}
for _n in EXACT:
    CEILING[_n] = (0.0,) * FUNCS[_n][1]


# ---- probe trees ------------------------------------------------------------------------------------------------------------------
def probe_forest(name, ops, form="direct", gp_len=64, multi=False):
    """-> (value, type, size, cpos): one probe tree per operand point; cpos[k] is the node index of operand k's CONST.
    multi: the probed node carries the OUT flag to output 0."""
    fid, arity = FUNCS[name]
    n = len(ops[0])
    value, type_, size = np.zeros((n, gp_len), F32), np.zeros((n, gp_len), np.int16), np.zeros((n, gp_len), np.int16)
    per = 1 if form == "direct" else 3
    ftype = {1: U, 2: B, 3: T}[arity]
    value[:, 0] = out_word(fid, 0) if multi else F32(fid)
    type_[:, 0] = ftype | 0x80 if multi else ftype
    size[:, 0] = 1 + arity * per
    cpos, k = [], 1
    for a in range(arity):
        if form == "direct":
            ci = k
        else:
            value[:, k], type_[:, k], size[:, k] = R.F_ADD, B, 3
            ci, xi = (k + 2, k + 1) if multi else (k + 1, k + 2)
            value[:, xi], type_[:, xi], size[:, xi] = 0, V, 1
        value[:, ci], type_[:, ci], size[:, ci] = ops[a], C, 1
        cpos.append(ci)
        k += per
    return value, type_, size, cpos


def effective_operands(ops, form, multi):
    """the operands f sees: the single-output stacked form adds +0 to each (-0 becomes +0)"""
    if form == "stacked" and not multi:
        return [np.where(o == 0, F32(0), o).astype(F32) for o in ops]
    return [np.asarray(o, F32) for o in ops]


# ---- truth --------------------------------------------------------------------------------------------------------------------------
def _fid(name):
    fid = FUNCS[name][0]
    return None if name.startswith("UNKNOWN") else fid


def forward(name, ops32):
    """float64 value of f at the fp32 operands"""
    o = [np.asarray(x, F32).astype(np.float64) for x in ops32]
    with np.errstate(all="ignore"):
        if name == "IF":
            return np.where(o[0] > 0, o[1], o[2])
        return R.unary(_fid(name), o[0]) if len(o) == 1 else R.binary(_fid(name), o[0], o[1])


def rule(name, ops32, g=1.0):
    """-> [d_k]: the float64 adjoint of every operand for the result adjoint g (scalar or per point)"""
    o = [np.asarray(x, F32).astype(np.float64) for x in ops32]
    g = np.broadcast_to(np.asarray(g, np.float64), o[0].shape)
    r = forward(name, ops32)
    with np.errstate(all="ignore"):
        if name == "IF":
            take_b = o[0] > 0
            return [np.zeros_like(o[0]), np.where(take_b, g, 0.0), np.where(take_b, 0.0, g)]
        if len(o) == 1:
            return [np.broadcast_to(R.unary_adjoint(_fid(name), o[0], r, g), o[0].shape)]
        return [np.broadcast_to(d, o[0].shape) for d in R.binary_adjoint(_fid(name), o[0], o[1], r, g)]


def launch_label(pred64):
    """the one label of a launch (fp32): the least pred - max(1, 2|pred|) over the trees with a finite fp32 prediction, or 0"""
    with np.errstate(all="ignore"):
        p32 = pred64.astype(F32)
    fin = np.isfinite(p32)
    if not fin.any():
        return F32(0)
    p = pred64[fin]
    y = float(np.min(p - np.maximum(1.0, 2.0 * np.abs(p))))
    if y <= -FLT_MAX:
        return F32(-FLT_MAX)
    y32 = F32(y)
    return y32 if float(y32) <= y else np.nextafter(y32, F32(-np.inf))


def out_adjoint(pred64, y32):
    """sign(pred - y) as the kernel forms it: +1 / -1 / 0 / NaN"""
    with np.errstate(all="ignore"):
        return np.sign(pred64.astype(F32).astype(np.float64) - float(y32))


# ---- operand draws ------------------------------------------------------------------------------------------------------------------
SPECIAL = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1.1754942e-38, 1.17549435e-38, 3.4028235e38,
                    -3.4028235e38, 0.5, 2.0, np.pi, -np.pi, np.pi / 2, 1e9, -1e9, 1e-9, -1e-9], F32)


def _log_uniform(rng, n, e_lo, e_hi, signed):
    x = np.ldexp(rng.uniform(1.0, 2.0, n), rng.integers(e_lo, e_hi, n)).astype(F32)
    return x * rng.choice([-1.0, 1.0], n).astype(F32) if signed else x


def _operand(rng, n, e_lo=-40, e_hi=40, lo=None, hi=None, signed=True, special=True):
    """tests/test_gpu_ulp.py's inputs() with a chosen exponent range: a third dense around the origin, the rest log-uniform in
    magnitude over [2^e_lo, 2^e_hi), and the special operands"""
    ns = len(SPECIAL) if special else 0
    dense = rng.uniform(-10.0 if signed else 0.0, 10.0, n // 3).astype(F32)
    wide = _log_uniform(rng, n - n // 3 - ns, e_lo, e_hi, signed)
    x = np.concatenate([dense, wide, SPECIAL[:ns]]).astype(F32)
    if lo is not None:
        keep = np.isnan(x) | np.isinf(x) | ((x >= lo) & (x <= hi))
        x = np.where(keep, x, rng.uniform(lo, hi, x.shape).astype(F32))
    return x


# The ranges test_gpu_ulp.py draws from (magnitudes down to 2^-126, bases up to 2^20) leave 0.88 / 0.46 / 0.52 of the points of the
# trigonometric / LOG SQRT / POW rules inside the accuracy comparison; these keep at least 0.9 (tests/test_adjoint_battery.py).
DOMAIN = {
    "SIN": dict(e_hi=17), "COS": dict(e_hi=17), "TAN": dict(e_hi=17), "SINH": dict(e_hi=7, lo=-89.0, hi=89.0),
    "COSH": dict(e_hi=7, lo=-89.0, hi=89.0), "TANH": dict(e_hi=6), "LOG": dict(signed=False), "SQRT": dict(signed=False),
    "EXP": dict(e_hi=7, lo=-104.0, hi=88.7), "DIV": dict(e_lo=-30, e_hi=30), "LOOSE_DIV": dict(e_lo=-30, e_hi=30),
}


def draws(name, n=N_DRAWS):
    """the operands of one function: the same in every run"""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    arity = FUNCS[name][1]
    if "POW" in name:
        a = _operand(rng, n, -8, 8, signed=(name == "LOOSE_POW"))
        b = rng.uniform(-12, 12, n).astype(F32)
        ints = rng.random(n) < 0.25
        b[ints] = np.round(b[ints])
        if name == "POW":                # negative bases with integer exponents
            neg = ints & (rng.random(n) < 0.5)
            a[neg] = -np.abs(a[neg])
        return [a, b]
    ops = [_operand(rng, n, **DOMAIN.get(name, {})) for _ in range(arity)]
    for o in ops[1:]:
        rng.shuffle(o)
    if name in ("MAX", "MIN", "LT", "GT", "LE", "GE"):   # a share of exact ties
        tie = rng.random(n) < 0.1
        ops[1][tie] = ops[0][tie]
    return ops


# ---- units ------------------------------------------------------------------------------------------------------------------------
def ulp32(t64):
    """the fp32 spacing at |t|; from 2^127 on, beyond the fp32 range too, the spacing of the top binade (2^104); inf for inf and NaN"""
    with np.errstate(all="ignore"):
        m = np.abs(np.asarray(t64, np.float64))
        s = np.spacing(np.minimum(m, 2.0 ** 127).astype(F32)).astype(np.float64)
        return np.where(np.isfinite(m), np.maximum(s, 2.0 ** -149), np.inf)


def units(name, ops32):
    """-> per operand (unit u, [the intermediates the rule names]) in float64; g = 1"""
    o = [np.asarray(x, F32).astype(np.float64) for x in ops32]
    a = o[0]
    r = forward(name, ops32)
    d = rule(name, ops32)
    z = np.zeros_like(a)
    with np.errstate(all="ignore"):
        if name in EXACT:
            return [(z, [])] * len(o)
        base = [ulp32(x) for x in d]
        if name == "SIN":
            return [(base[0] + FWD["COS"] * ulp32(np.cos(a)), [np.cos(a)])]
        if name == "COS":
            return [(base[0] + FWD["SIN"] * ulp32(np.sin(a)), [np.sin(a)])]
        if name == "SINH":
            return [(base[0] + FWD["COSH"] * ulp32(np.cosh(a)), [np.cosh(a)])]
        if name == "COSH":
            return [(base[0] + FWD["SINH"] * ulp32(np.sinh(a)), [np.sinh(a)])]
        if name in ("TAN", "TANH"):
            return [(base[0] + 2 * np.abs(r) * FWD[name] * ulp32(r), [r * r])]
        if name in ("LOG", "LOOSE_LOG"):
            return [(base[0], [])]
        if name == "EXP":
            return [(base[0] + FWD["EXP"] * ulp32(r), [])]
        if name in ("INV", "LOOSE_INV"):
            return [(base[0] + 2 * np.abs(r) * FWD[name] * ulp32(r), [r * r])]
        if name in ("SQRT", "LOOSE_SQRT"):
            return [(base[0] + 0.5 / (r * r) * FWD[name] * ulp32(r), [])]
        if name == "MUL":
            return [(base[0], []), (base[1], [])]
        b = o[1]
        if name in ("DIV", "LOOSE_DIV"):
            dd = b if name == "DIV" else np.where(np.abs(b) <= float(DELTA), np.copysign(float(DELTA), b), b)
            return [(base[0], []), (base[1] + np.abs(1 / dd) * FWD[name] * ulp32(r), [r / dd])]
        if name in ("POW", "LOOSE_POW"):
            m = np.abs(a)
            lg = np.where(m > 0, np.log(np.where(m > 0, m, 1.0)), 0.0)
            p = np.power(m, b - 1)
            rr = np.power(m, b)
            ua = base[0] + np.abs(b) * FWD[name] * ulp32(p) + np.abs(b * p * lg) * 0.5 * ulp32(b - 1)
            live = (a > 0) if name == "POW" else (m > 0)
            ub = np.where(live, base[1] + np.abs(lg) * FWD[name] * ulp32(rr) + np.abs(rr) * FWD["LOG"] * ulp32(lg), base[1])
            return [(ua, [p, rr]), (ub, [lg, rr])]
    raise KeyError(name)


LO, HI = 2.0 ** -100, 2.0 ** 100


def _in_range(x):
    with np.errstate(all="ignore"):
        return (x == 0) | ((np.abs(x) >= LO) & (np.abs(x) <= HI))


def accuracy_mask(name, ops32):
    """per operand: the points of the accuracy comparison -- the truth, r and every intermediate the rule names are each zero or of
    magnitude within [2^-100, 2^100] (and the unit is finite); every other point is class-compared only"""
    r = forward(name, ops32)
    d = rule(name, ops32)
    out = []
    for k, (u, inter) in enumerate(units(name, ops32)):
        m = _in_range(d[k]) & _in_range(r) & np.isfinite(u)
        for x in inter:
            m &= _in_range(x)
        out.append(m)
    return out


# ---- the planted edge cells ---------------------------------------------------------------------------------------------------------
# Tokens of an expectation:  "Z" == 0   "N" NaN   "G" / "MG" the bits of 1.0f / -1.0f   "PI" / "NI" +inf / -inf   a float32: those
# bits (the rule is a chain of correctly rounded operations there)   "R" a plain cell: the reference's value within the bound.
# (operands, rule) or (operands, rule, grad): `rule` is the table at g = 1 -- what the Jacobian walk shows, and the gradient walk
# wherever the prediction is finite; `grad` is the gradient word where the prediction is not finite (output adjoint -1 or NaN).
def _f(x):
    return F32(x)


_THREE = F32(3)
EDGES = {
    "ADD": [((5, 3), ("G", "G"))],
    "SUB": [((5, 3), ("G", "MG")), ((3, 5), ("G", "MG"))],
    "MUL": [((2, 3), (_f(3), _f(2))), ((0, 3), (_f(3), "Z"))],
    "DIV": [((1, 0.0), ("PI", "N"), ("N", "N")), ((1, -0.0), ("NI", "N"), ("N", "N")), ((0, 0.0), ("PI", "N"), ("N", "N")),
            ((1, DEN), ("PI", "NI")), ((0, DEN), ("PI", "Z")), ((0, 2), (_f(0.5), "Z")), ((1, -DEN), ("NI", "NI"), ("PI", "PI")),
            ((6, 2), (_f(0.5), _f(-1.5))), ((2, 6), ("R", "R"))],
    "LOOSE_DIV": [((3, DELTA_DN), (_f(1) / DELTA, "Z")), ((3, DELTA), (_f(1) / DELTA, "Z")),
                  ((3, DELTA_UP), (_f(1) / DELTA_UP, -(_THREE / DELTA_UP) / DELTA_UP)),
                  ((3, -DELTA_DN), (_f(-1) / DELTA, "Z")), ((3, -DELTA), (_f(-1) / DELTA, "Z")),
                  ((3, -DELTA_UP), (_f(-1) / DELTA_UP, -(_THREE / -DELTA_UP) / -DELTA_UP)),
                  ((3, 0.0), (_f(1) / DELTA, "Z")), ((3, -0.0), (_f(-1) / DELTA, "Z")), ((0, 0.0), (_f(1) / DELTA, "Z")),
                  ((3, DEN), (_f(1) / DELTA, "Z")), ((6, 2), (_f(0.5), _f(-1.5)))],
    "POW": [((-2, 3), ("R", "Z")), ((-2, 2), ("R", "Z")), ((0, 2), ("Z", "Z")), ((0, 1), ("G", "Z")), ((0, 0), ("N", "Z")),
            ((0, -1), ("NI", "Z")), ((-0.0, 2), ("Z", "Z")), ((-2, 0.5), ("N", "Z")), ((-2, -1.5), ("N", "Z")), ((2, 3), ("R", "R")),
            ((DEN, 1), ("G", "R")), ((1, 5), (_f(5), "Z"))],
    "LOOSE_POW": [((0, 0), ("Z", "Z")), ((-0.0, 0.0), ("Z", "Z")), ((0, 2), ("Z", "Z")), ((0, 1), ("Z", "Z")), ((0, -1), ("N", "Z")),
                  ((-2, 3), ("R", "R")), ((-2, 0.5), ("R", "R")), ((2, 3), ("R", "R")), ((-1e-30, 1), ("MG", "R")),
                  ((1e-30, 1), ("G", "R")), ((-1, 5), (_f(-5), "Z"))],
    "MAX": [((1, 1), ("G", "Z")), ((0.0, -0.0), ("G", "Z")), ((-0.0, 0.0), ("G", "Z")), ((1, ONE_UP), ("Z", "G")),
            ((ONE_UP, 1), ("G", "Z")), ((ONE_DN, 1), ("Z", "G")), ((1, ONE_DN), ("G", "Z")), ((np.nan, 1), ("Z", "G")),
            ((1, np.nan), ("Z", "G"), ("Z", "N")), ((np.inf, np.inf), ("G", "Z")), ((-np.inf, 1), ("Z", "G"))],
    "MIN": [((1, 1), ("G", "Z")), ((0.0, -0.0), ("G", "Z")), ((-0.0, 0.0), ("G", "Z")), ((1, ONE_UP), ("G", "Z")),
            ((ONE_UP, 1), ("Z", "G")), ((ONE_DN, 1), ("G", "Z")), ((1, ONE_DN), ("Z", "G")), ((np.nan, 1), ("Z", "G")),
            ((1, np.nan), ("Z", "G"), ("Z", "N")), ((np.inf, np.inf), ("G", "Z")), ((np.inf, 1), ("Z", "G"))],
    "IF": [((1, 2, 3), ("Z", "G", "Z")), ((0.0, 2, 3), ("Z", "Z", "G")), ((-0.0, 2, 3), ("Z", "Z", "G")), ((-1, 2, 3), ("Z", "Z", "G")),
           ((np.nan, 2, 3), ("Z", "Z", "G")), ((DEN, 2, 3), ("Z", "G", "Z")), ((-DEN, 2, 3), ("Z", "Z", "G")),
           ((np.inf, 2, 3), ("Z", "G", "Z")), ((-np.inf, 2, 3), ("Z", "Z", "G")), ((1, np.nan, 3), ("Z", "G", "Z"), ("Z", "N", "Z")),
           ((-1, np.nan, 3), ("Z", "Z", "G"))],
    "SIN": [((0,), ("G",)), ((HALF_PI,), ("R",))],
    "COS": [((0,), ("Z",)), ((HALF_PI,), ("R",))],
    "TAN": [((HALF_PI,), ("R",)), ((np.nextafter(HALF_PI, F32(0)),), ("R",)), ((0,), ("G",))],
    "SINH": [((89.0,), ("R",)), ((89.5,), ("PI",)), ((-89.5,), ("PI",), ("NI",)), ((0,), ("G",))],
    "COSH": [((89.0,), ("R",)), ((89.5,), ("PI",)), ((-89.5,), ("NI",)), ((0,), ("Z",))],
    "TANH": [((0,), ("G",)), ((20,), ("Z",)), ((-20,), ("Z",))],
    "LOG": [((0.0,), ("PI",), ("NI",)), ((-0.0,), ("NI",), ("PI",)), ((-2,), (_f(-0.5),), ("N",)), ((2,), (_f(0.5),)),
            ((DEN,), ("PI",))],
    "LOOSE_LOG": [((0.0,), ("Z",)), ((-0.0,), ("Z",)), ((-2,), (_f(-0.5),)), ((2,), (_f(0.5),)), ((DEN,), ("PI",)), ((-DEN,), ("NI",))],
    "EXP": [((88.7,), ("R",)), ((88.8,), ("PI",)), ((0,), ("G",)), ((-np.inf,), ("Z",))],
    "INV": [((0.0,), ("N",)), ((-0.0,), ("N",)), ((2,), (_f(-0.25),)), ((-2,), (_f(-0.25),))],
    "LOOSE_INV": [((DELTA_DN,), ("Z",)), ((DELTA,), ("Z",)), ((DELTA_UP,), (-((_f(1) / DELTA_UP) * (_f(1) / DELTA_UP)),)),
                  ((-DELTA_DN,), ("Z",)), ((-DELTA,), ("Z",)), ((-DELTA_UP,), (-((_f(1) / DELTA_UP) * (_f(1) / DELTA_UP)),)),
                  ((0.0,), ("Z",)), ((-0.0,), ("Z",)), ((DEN,), ("Z",)), ((2,), (_f(-0.25),))],
    "NEG": [((3,), ("MG",)), ((-3,), ("MG",)), ((0,), ("MG",)), ((np.inf,), ("MG",), ("G",))],
    "ABS": [((0.0,), ("Z",)), ((-0.0,), ("Z",)), ((-3,), ("MG",)), ((3,), ("G",)), ((-DEN,), ("MG",)), ((DEN,), ("G",))],
    "SQRT": [((0.0,), ("PI",)), ((-0.0,), ("NI",)), ((-4,), ("N",)), ((4,), (_f(0.25),)), ((-DEN,), ("N",))],
    "LOOSE_SQRT": [((0.0,), ("Z",)), ((-0.0,), ("Z",)), ((-4,), (_f(-0.25),)), ((4,), (_f(0.25),)), ((-16,), (_f(-0.125),))],
    "UNKNOWN_U": [((1,), ("Z",)), ((np.nan,), ("Z",)), ((np.inf,), ("Z",)), ((0,), ("Z",)), ((-3,), ("Z",))],
}
for _n in ("LT", "GT", "LE", "GE", "UNKNOWN_B"):
    EDGES[_n] = [((p, q), ("Z", "Z")) for p, q in ((1, 2), (2, 1), (1, 1), (np.nan, 1), (1, np.nan), (np.inf, -np.inf), (0.0, -0.0),
                                                    (-np.inf, np.inf), (DEN, 0))]


def edge_points(name):
    """-> (ops [arity arrays fp32], rule tokens [per point a tuple], grad tokens [per point a tuple or None])"""
    cells = EDGES[name]
    arity = FUNCS[name][1]
    ops = [np.array([c[0][k] for c in cells], F32) for k in range(arity)]
    return ops, [c[1] for c in cells], [c[2] if len(c) > 2 else None for c in cells]


def points(name, form="direct", multi=False):
    """the operands of one launch: the draws, then the edge cells (without those holding a -0 where the form cannot keep one)
    -> (ops, n_draws, rule tokens, grad tokens, the kept cells' indices into EDGES[name]); the tokens are those of the edge part"""
    dr = draws(name)
    eo, rt, gt = edge_points(name)
    keep = np.ones(len(rt), bool)
    if form == "stacked" and not multi:
        for o in eo:
            keep &= ~((o == 0) & np.signbit(o))
    idx = np.flatnonzero(keep)
    ops = [np.concatenate([d, e[idx]]).astype(F32) for d, e in zip(dr, eo)]
    return ops, len(dr[0]), [rt[i] for i in idx], [gt[i] for i in idx], idx


def token_of(x64):
    """the token a float64 reference value implies (class only: a plain value is "R")"""
    if np.isnan(x64):
        return "N"
    if x64 == 0:
        return "Z"
    if np.isinf(x64):
        return "PI" if x64 > 0 else "NI"
    return "G" if x64 == 1 else "MG" if x64 == -1 else "R"


def token_holds(tok, got32):
    """does the fp32 word `got32` meet the token (exactly)?  "R" is not decided here"""
    got32 = F32(got32)
    if isinstance(tok, str):
        if tok == "Z":
            return got32 == 0
        if tok == "N":
            return bool(np.isnan(got32))
        if tok == "G":
            return got32.view(np.uint32) == F32(1).view(np.uint32)
        if tok == "MG":
            return got32.view(np.uint32) == F32(-1).view(np.uint32)
        if tok == "PI":
            return got32 == np.inf
        if tok == "NI":
            return got32 == -np.inf
        return True
    return got32.view(np.uint32) == F32(tok).view(np.uint32)


def expected_tokens(name, ops32, rule_tok, grad_tok, g):
    """the expectation of the gradient word of one edge point whose output adjoint is g (+1, -1, 0 or NaN)"""
    if g == 1:
        return rule_tok
    if grad_tok is not None:
        return grad_tok
    return tuple(token_of(float(d[0])) for d in rule(name, [np.array([o], F32) for o in ops32], g))


# ---- the normal equations of a probe tree (D = 1, y = 0) --------------------------------------------------------------------------
def normal_row(name, ops32):
    """float64 (loss, {(i, j): A_ij}, [b_i]) of the probe tree of every point: A_ij = d_i d_j, b_i = d_i pred, loss = pred^2"""
    d = rule(name, ops32)
    pred = forward(name, ops32)
    with np.errstate(all="ignore"):
        A = {(i, j): d[i] * d[j] for i in range(len(d)) for j in range(i, len(d))}
        return pred * pred, A, [x * pred for x in d]


def tri_index(i, j):
    return LM.TRI.index((i, j))
