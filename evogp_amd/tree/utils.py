"""Encoding tables and small helpers of the Forest tensors.

The numeric values are the wire format shared with the kernels (reference:
src/evogp/cuda/defs.h:10-57, mirrored in src/evogp/tree/utils.py:14-136); the helper semantics
follow src/evogp/tree/utils.py:261-310.
"""
from __future__ import annotations

import torch

DELTA = 1e-9
MAXVAL = 1e9
MAX_STACK = 1024
MAX_FULL_DEPTH = 10


class NType:
    """Node types (low 7 bits) and the output-node flag (bit 7)."""

    VAR = 0
    CONST = 1
    UFUNC = 2
    BFUNC = 3
    TFUNC = 4
    TYPE_MASK = 0x7F
    OUT_NODE = 1 << 7
    UFUNC_OUT = UFUNC + OUT_NODE
    BFUNC_OUT = BFUNC + OUT_NODE
    TFUNC_OUT = TFUNC + OUT_NODE


# function id -> user-facing name; ids 0 ternary, 1..13 binary, 14..28 unary
FUNCS_NAMES = [
    "if",
    "+", "-", "*", "/", "loose_div", "pow", "loose_pow", "max", "min", "<", ">", "<=", ">=",
    "sin", "cos", "tan", "sinh", "cosh", "tanh", "log", "loose_log", "exp", "inv", "loose_inv", "neg", "abs",
    "sqrt", "loose_sqrt",
]


class Func:
    TF_START = 0
    BF_START = 1
    UF_START = 14
    END = 29


for _i, _n in enumerate(
    ["IF", "ADD", "SUB", "MUL", "DIV", "LOOSE_DIV", "POW", "LOOSE_POW", "MAX", "MIN", "LT", "GT", "LE", "GE",
     "SIN", "COS", "TAN", "SINH", "COSH", "TANH", "LOG", "LOOSE_LOG", "EXP", "INV", "LOOSE_INV", "NEG", "ABS",
     "SQRT", "LOOSE_SQRT"]
):
    setattr(Func, _n, _i)

FUNCS = list(range(Func.END))
FUNCS_DISPLAY = list(FUNCS_NAMES)


def func_arity(func_id: int) -> int:
    return 3 if func_id < Func.BF_START else (2 if func_id < Func.UF_START else 1)


_DEVICE = None


def default_device() -> torch.device:
    """The device Forest tensors live on.  The reference hard-codes "cuda" (tree/utils.py:280-285);
    on a GPU-less host (CPU-only unit tests of the host logic) tensors stay on the CPU and any
    attempt to run an op fails loudly because only device kernels are registered."""
    global _DEVICE
    if _DEVICE is None:
        _DEVICE = torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")
    return _DEVICE


def set_default_device(device) -> None:
    """Pin the device (e.g. ``cuda:LOCAL_RANK`` in a multi-process run)."""
    global _DEVICE
    _DEVICE = torch.device(device)


def dict2prob(prob_dict) -> torch.Tensor:
    """{function name: weight} -> normalised probability vector over the 29 function ids."""
    assert len(prob_dict) > 0, "Empty probability dictionary"
    prob = torch.zeros(Func.END)
    for name, weight in prob_dict.items():
        assert name in FUNCS_NAMES, f"Unknown function name: {name}, total functions are {FUNCS_NAMES}"
        prob[FUNCS_NAMES.index(name)] = weight
    return prob / prob.sum()


def check_tensor(x, device=None):
    """Tensor on ``device`` (a Forest passes the device of its own tensors, so operands follow the population in a
    multi-GPU process; default: the default device), detached (non-tensors are converted to float32)."""
    device = default_device() if device is None else device
    if not isinstance(x, torch.Tensor):
        return torch.tensor(x, dtype=torch.float32, device=device)
    return x.to(device).detach().requires_grad_(False)


def randint(size, low, high, dtype=torch.int32, device=None, requires_grad=False):
    """Uniform integers in [low, high) drawn as floor(low + U*(high-low)); low/high may be tensors."""
    device = default_device() if device is None else device
    u = torch.rand(size, device=device, requires_grad=requires_grad)
    return (low + u * (high - low)).to(dtype=dtype)


def draw_keys(device=None) -> torch.Tensor:
    """the two 32-bit keys of a generation launch, from torch's generator of ``device`` (forest.py:51-58)"""
    device = default_device() if device is None else device
    try:
        return torch.randint(low=0, high=1000000, size=(2,), dtype=torch.uint32, device=device)
    except RuntimeError:  # back ends without a uint32 randint
        return torch.randint(0, 1000000, (2,), device=device).to(torch.uint32)


def box_side(bound, n: int) -> torch.Tensor:
    """one side of a box of inputs -- a float for all ``n`` variables, or one value each -- as a flat float32 tensor on the host (the
    caller checks its length)"""
    if isinstance(bound, (int, float)):
        return torch.full((n,), float(bound), dtype=torch.float32)
    return torch.as_tensor(bound).detach().to("cpu", torch.float32).reshape(-1)


def str_tree(value, node_type, subtree_size) -> str:
    """Prefix listing of the live nodes of one tree."""
    out = []
    for i in range(int(subtree_size[0])):
        t = int(node_type[i]) & NType.TYPE_MASK
        if t == NType.VAR:
            out.append(f"x[{int(value[i])}]")
        elif t == NType.CONST:
            out.append(f"{float(value[i]):.2f}")
        else:
            out.append(FUNCS_NAMES[decode_func(value[i], node_type[i])[0]])
    return " ".join(out)


def decode_func(value, node_type):
    """(function id, output index or -1) of a function node."""
    if int(node_type) & NType.OUT_NODE:
        bits = torch.as_tensor(value, dtype=torch.float32).view(torch.int32).item()
        return bits & 0xFFFF, (bits >> 16) & 0xFFFF
    return int(value), -1


# ---- physical units (dimensional analysis, csrc/sr_dims.hip) ----
DIM_DEN = 25200          # EVOGP_DIM_DEN: every exponent is a numerator over 2^4 3^2 5^2 7
DIM_MAX_NUM = 1 << 24    # EVOGP_DIM_MAX_NUM: a numerator is in range when |n| <= 2^24
DIM_MAX_DIMS = 8         # EVOGP_DIM_MAX_DIMS


def unit_numerators(exponents, what: str = "a unit"):
    """Exponents (ints, floats or ``Fraction``s, any nesting) -> the same nesting of int numerators over ``DIM_DEN``, exactly;
    ``ValueError`` for an exponent of another type (a string, a bool), one that is no multiple of 1/25200 or one whose numerator
    leaves the range."""
    from fractions import Fraction

    if isinstance(exponents, torch.Tensor):
        exponents = exponents.tolist()
    elif hasattr(exponents, "tolist"):
        exponents = exponents.tolist()
    if isinstance(exponents, (list, tuple)):
        return [unit_numerators(e, what) for e in exponents]
    if isinstance(exponents, bool) or not isinstance(exponents, (int, float, Fraction)):
        raise ValueError(f"{what} holds {exponents!r}: an exponent is an int, a float or a Fraction")
    try:
        n = Fraction(exponents) * DIM_DEN
    except (ValueError, OverflowError) as e:
        raise ValueError(f"{what} holds {exponents!r}, which is no finite number") from e
    if n.denominator != 1 or abs(n.numerator) > DIM_MAX_NUM:
        raise ValueError(f"{what} holds the exponent {exponents!r}: times {DIM_DEN} it must be an integer of magnitude <= {DIM_MAX_NUM}")
    return int(n.numerator)


def check_units(input_units, label_units, input_len: int):
    """``(var, label, has_label)``: ``input_units`` as ``input_len`` rows of K numerators and ``label_units`` as K numerators (zeros for
    None), checked: ``ValueError`` for a wrong shape, K outside 1 .. ``DIM_MAX_DIMS`` or an exponent ``unit_numerators`` refuses"""
    def flat(row):
        return isinstance(row, list) and len(row) > 0 and all(isinstance(n, int) for n in row)

    var = unit_numerators(input_units, "input_units")
    if not (isinstance(var, list) and len(var) == input_len and all(flat(r) and len(r) == len(var[0]) for r in var)):
        raise ValueError(f"input_units should hold one row of K exponents for each of the {input_len} inputs")
    K = len(var[0])
    if K > DIM_MAX_DIMS:
        raise ValueError(f"a unit has 1 .. {DIM_MAX_DIMS} base dimensions, but input_units has {K}")
    label = [0] * K if label_units is None else unit_numerators(label_units, "label_units")
    if not (flat(label) and len(label) == K):
        raise ValueError(f"label_units should hold {K} exponents, one for each base dimension of input_units")
    return var, label, label_units is not None


# ---- structural constraints (csrc/sr_structure.hip) ----
STRUCT_SYMBOLS = 32        # EVOGP_STRUCT_SYMBOLS: the function ids 0 .. 28, then
STRUCT_NAMES = FUNCS_NAMES + ["var", "const", "unknown"]   # 29 a variable, 30 a constant, 31 a function node with an unknown id
STRUCT_MAX_RULES = 8       # EVOGP_STRUCT_MAX_RULES
STRUCT_MAX_COST = 65535    # of one node
STRUCT_MAX_NEST = 254      # the largest limit of a nesting rule (the counters saturate at 255)
STRUCT_MAX_OPERAND = (1 << 31) - 1


def _struct_symbol(name, what: str) -> int:
    if not isinstance(name, str) or name not in STRUCT_NAMES:
        raise ValueError(f"{what} names {name!r}, but the symbols are {STRUCT_NAMES}")
    return STRUCT_NAMES.index(name)


def _struct_int(x, lo: int, hi: int, what: str) -> int:
    import numbers

    if isinstance(x, bool) or not isinstance(x, numbers.Integral) or not lo <= int(x) <= hi:
        raise ValueError(f"{what} should be an int in [{lo}, {hi}], but got {x!r}")
    return int(x)


def parse_structure(complexity_of=None, nested_constraints=None, operand_constraints=None):
    """Dictionaries -> ``(cost, operand_limit, rules)``, the host tables of ``Forest.SR_structure``: ``cost`` 32 ints, ``operand_limit``
    32 rows of 3 ints (-1: none) and ``rules`` a list of ``(outer_mask, inner_mask, limit)`` with the masks as sets of symbols (bit s).
    The keys are ``FUNCS_NAMES`` plus ``"var"``, ``"const"`` and ``"unknown"`` (a function node whose id is none of its class).
    ``complexity_of={"sin": 3, "const": 2}``: the cost of one node, 1 where not given, each in [0, 65535].
    ``nested_constraints={"sin": {"sin": 0, "cos": 0}, "pow": {"pow": 1}}``: one rule per (outer, inner) pair -- on every path below an
    ``outer`` node at most ``limit`` (0 .. 254) ``inner`` nodes; at most 8 rules.
    ``operand_constraints={"pow": (-1, 1), "sin": 5}``: the largest complexity of each operand, -1 for none -- an int for a unary
    function, a tuple of the function's arity otherwise (``"unknown"``: an int or a tuple of 1 or 2).
    ``ValueError`` for an unknown name, a bool or another non-int, a value outside its range, a tuple of the wrong arity, a leaf in
    ``operand_constraints``, or more than 8 rules."""
    cost = [1] * STRUCT_SYMBOLS
    for name, c in dict(complexity_of or {}).items():
        cost[_struct_symbol(name, "complexity_of")] = _struct_int(c, 0, STRUCT_MAX_COST, f"the cost of {name!r}")
    rules = []
    for outer, inners in dict(nested_constraints or {}).items():
        so = _struct_symbol(outer, "nested_constraints")
        if not isinstance(inners, dict):
            raise ValueError(f"nested_constraints[{outer!r}] should be a dictionary {{inner: limit}}, but got {inners!r}")
        for inner, limit in inners.items():
            si = _struct_symbol(inner, f"nested_constraints[{outer!r}]")
            rules.append((1 << so, 1 << si, _struct_int(limit, 0, STRUCT_MAX_NEST, f"the limit of {inner!r} inside {outer!r}")))
    if len(rules) > STRUCT_MAX_RULES:
        raise ValueError(f"nested_constraints holds {len(rules)} (outer, inner) pairs, but at most {STRUCT_MAX_RULES} rules are supported")
    operand_limit = [[-1, -1, -1] for _ in range(STRUCT_SYMBOLS)]
    for name, lim in dict(operand_constraints or {}).items():
        s = _struct_symbol(name, "operand_constraints")
        if s in (STRUCT_NAMES.index("var"), STRUCT_NAMES.index("const")):
            raise ValueError(f"operand_constraints names {name!r}, which has no operands")
        arities = (1, 2) if name == "unknown" else (func_arity(s),)
        if isinstance(lim, (tuple, list)):
            lims = list(lim)
        elif 1 in arities:
            lims = [lim]
        else:
            raise ValueError(f"operand_constraints[{name!r}] should be a tuple of {arities[0]} limits, but got {lim!r}")
        if len(lims) not in arities:
            raise ValueError(f"operand_constraints[{name!r}] should hold {' or '.join(map(str, arities))} limits, but got {len(lims)}")
        for k, l in enumerate(lims):
            operand_limit[s][k] = _struct_int(l, -1, STRUCT_MAX_OPERAND, f"the limit of operand {k} of {name!r}")
    return cost, operand_limit, rules


def parse_monotonic(constraints, input_len=None):
    """``{variable: +1 | -1 | (dmin, dmax)}`` -> ``(variables, bounds, signs)``, three lists in the dictionary's order: the keys, the
    admissible range of the partial derivative as a pair of floats ([0, inf] for +1, [-inf, 0] for -1) and the sign itself (0 for a
    pair).  ``ValueError`` for any other constraint.  ``input_len``: also hold every key to an int in [0, input_len) and the
    dictionary to at least one entry; without it the caller checks the variables (``Forest._wrt``)."""
    variables, bounds, signs = [], [], []
    for v, c in dict(constraints).items():
        if input_len is not None and (not isinstance(v, int) or not 0 <= v < input_len):
            raise ValueError(f"monotonic names variable {v!r}, but the inputs are 0 .. {input_len - 1}")
        pair = isinstance(c, (tuple, list))
        if pair and len(c) == 2 and float(c[0]) <= float(c[1]):
            bounds.append((float(c[0]), float(c[1])))
        elif not pair and c in (1, -1):
            bounds.append((0.0, float("inf")) if c == 1 else (float("-inf"), 0.0))
        else:
            raise ValueError(f"a monotonic constraint must be +1, -1 or a (dmin, dmax) pair with dmin <= dmax, but variable {v} has {c!r}")
        variables.append(v)
        signs.append(0 if pair else int(c))
    if input_len is not None and not variables:
        raise ValueError("monotonic must constrain at least one variable")
    return variables, bounds, signs


def str_unit(unit, names=None) -> str:
    """One unit row (K numerators over ``DIM_DEN``) as text, e.g. ``m s^-2`` or ``m^1/2``; ``1`` for the dimensionless unit.  ``names``: the
    K base names (default ``d0, d1, ..``).  The exponents are exact fractions in lowest terms."""
    from fractions import Fraction

    unit = [int(n) for n in (unit.tolist() if hasattr(unit, "tolist") else unit)]
    names = [f"d{k}" for k in range(len(unit))] if names is None else list(names)
    if len(names) != len(unit):
        raise ValueError(f"{len(unit)} base dimensions, but {len(names)} names")
    parts = []
    for name, n in zip(names, unit):
        if n == 0:
            continue
        e = Fraction(n, DIM_DEN)
        parts.append(name if e == 1 else f"{name}^{e}")
    return " ".join(parts) if parts else "1"
