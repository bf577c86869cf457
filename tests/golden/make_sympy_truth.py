#!/usr/bin/env python3
"""The exact value of whole trees, taken from the REFERENCE's second statement of tree semantics: `Tree.to_sympy_expr`
(/root/reference/src/evogp/tree/tree.py:259-324) with `SYMPY_MAP` (tree/utils.py:201-232), evaluated by mpmath at 50 digits on float32
inputs converted exactly.  Everything else that checks what a tree computes descends from the reference's device code (oracle/_ref ->
oracle/evogp_oracle.c -> the kernels); this does not.

The reference package is imported as tests/golden/make_mutation_golden.py imports it ("cuda" means the CPU, evogp.evogp_cuda is a stub);
only `Tree`, `to_sympy_expr` and `SYMPY_MAP` are used, no op is called.  The trees are drawn by the CPU oracle's `generate`, with a few
hand-written rows spliced in front (every non-commutative operand order, every `if` branch, the forwarded operand of an OUT node).

A tree is handed to the reference's `Tree` with its constants as exact rationals (every float32 is one), so that sympy folds constant
subtrees exactly instead of at float32's 24 bits; the three `Loose*` classes are evaluated by their own `eval`.

Written per group to tests/golden/sympy_truth_<group>.npz (data only: forest rows cut to the shortest L, X float32, T float64,
`exported` per tree, `mp_ok` per entry, `hand` per tree, a JSON header with the seeds, the versions and the counts of what was left out):
  * a tree whose export or lambdify raises, or whose expression sympy folds to zoo / nan / a complex number, stays in the file with
    exported = False (no truth);
  * multi-output trees with a UNARY OUT node are not stored: tree.py:319-321 pushes a `right` that was never assigned for such a node;
  * multi-output trees in which the value of a function node WITHOUT the OUT flag reaches an OUT node are not stored: the reference's two
    statements contradict each other there (forward.cu:237-243 forwards the last operand of EVERY function node, tree.py:322-323
    forwards the node's own result); DESIGN.md section 4;
  * drawn trees of fewer than three nodes, and multi-output trees that write fewer than two outputs, are passed over: a lone leaf or an
    output that no node writes compares zeros and shows nothing.

    python tests/golden/make_sympy_truth.py          (needs /root/reference, sympy, mpmath; never runs on the GPU box)
"""
import io
import json
import os
import sys
import types
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = "/root/reference/src"


# ---- "cuda" means the CPU; the reference package under its own name ---------------------------------------------------------------
def _is_cuda(d):
    return d is not None and str(d).startswith("cuda")


def _decuda(fn):
    def wrapped(*a, **k):
        if _is_cuda(k.get("device")):
            k["device"] = "cpu"
        return fn(*a, **k)
    return wrapped


for _name in ("arange", "rand", "randint", "zeros", "ones", "empty", "tensor", "full", "randn"):
    setattr(torch, _name, _decuda(getattr(torch, _name)))
for _m in [m for m in sys.modules if m == "evogp" or m.startswith("evogp.")]:
    del sys.modules[_m]
sys.modules["evogp.evogp_cuda"] = types.ModuleType("evogp.evogp_cuda")
sys.path.insert(0, REF)
import evogp  # noqa: E402  (the reference)

assert evogp.__file__.startswith(REF), evogp.__file__
import mpmath  # noqa: E402
import sympy as sp  # noqa: E402
from mpmath import mp  # noqa: E402
import evogp.tree.utils as ref_utils  # noqa: E402
from evogp.tree import Tree  # noqa: E402

import exact_eval_ref as ex  # noqa: E402
from oracle.pyoracle import Oracle, depth2leaf  # noqa: E402

mp.dps = 50
ROWS = 100
CS = [-1.0, 0.0, 1.0, 0.5, 2.0]
NONZERO = [-1.0, 1.0, 0.5, 2.0]   # where a literal x / 0 would cost more than a tenth of the trees their export (NaN trees have tests of their own)
F = ex.F


def roulette(weights):
    p = np.zeros(29, np.float64)
    for f, w in weights.items():
        p[f] = w
    return np.cumsum((p / p.sum()).astype(np.float32), dtype=np.float32)


def uniform(funcs):
    return {f: 1.0 for f in funcs}


# ---- hand-written rows: plain data, prefix order.  ("v", i) a variable, ("c", x) a constant, (name, children...) a function,
#      ("out", o, name, children...) a function node with the OUT flag for output o --------------------------------------------------
x0, x1, x2 = ("v", 0), ("v", 1), ("v", 2)
HAND_ARITH = [("SUB", x0, x1), ("DIV", x0, x1), ("SUB", x0, ("SUB", x1, x2)), ("DIV", ("SUB", x0, x1), ("DIV", x2, ("c", 2.0))),
              ("DIV", ("c", 1.0), ("MUL", x2, x2))]
HAND_WIDE = [("SUB", x0, x1), ("DIV", x0, x1), ("LOOSE_DIV", x0, x1), ("LOOSE_POW", x0, x1), ("IF", ("SUB", x0, x1), x1, x2),
             ("IF", ("SUB", x1, x0), x1, x2), ("IF", ("SUB", x0, x1), ("IF", ("SUB", x1, x2), x0, x1), ("IF", ("SUB", x2, x0), x2, ("NEG", x1))),
             ("IF", ("IF", ("SUB", x0, x2), ("NEG", x1), x1), ("SUB", x2, x0), ("DIV", x2, x0)), ("MAX", ("SUB", x0, x1), ("SUB", x1, x2)),
             ("MIN", ("SUB", x0, x1), ("SUB", x1, x2))]
HAND_POS = [("POW", x0, x1), ("POW", x0, ("SUB", x1, x2)), ("LOG", ("DIV", x0, x1)), ("SQRT", ("DIV", x0, x1))]
HAND_MO3 = [("out", 0, "SUB", x0, ("out", 1, "MUL", x1, x2)),                       # out1 = x1 x2; its LAST operand x2 goes up: out0 = x0 - x2
            ("out", 2, "SUB", ("out", 2, "SUB", x0, x1), x2),                       # two nodes add into one output: (x0 - x1) + (x1 - x2)
            ("out", 0, "MAX", ("out", 1, "SUB", x1, x0), ("out", 2, "SUB", x0, ("out", 1, "MUL", x2, x2))),
            ("ADD", ("out", 0, "SUB", x0, x1), ("out", 1, "SUB", x2, x0)),           # a root without the flag: its value is nobody's
            ("out", 1, "SUB", ("c", 2.0), ("out", 0, "MUL", ("out", 2, "ADD", x0, x1), x2))]


def flatten(node, out):
    """prefix order -> list of (value float32, type, children); returns the subtree size"""
    if node[0] == "v":
        out.append((np.float32(node[1]), 0, 1)); return 1
    if node[0] == "c":
        out.append((np.float32(node[1]), 1, 1)); return 1
    flag, name, kids = (0x80, node[2], node[3:]) if node[0] == "out" else (0, node[0], node[1:])
    f = F[name]
    val = np.array([(node[1] << 16) | f], np.uint32).view(np.float32)[0] if flag else np.float32(f)
    at = len(out)
    out.append(None)
    s = 1 + sum(flatten(k, out) for k in kids)
    assert len(kids) == (3 if f == 0 else 2 if f < 14 else 1)
    out[at] = (val, (len(kids) + 1) | flag, s)
    return s


def hand_rows(trees, L):
    v = np.zeros((len(trees), L), np.float32); t = np.zeros((len(trees), L), np.int16); s = np.zeros((len(trees), L), np.int16)
    for k, tree in enumerate(trees):
        nodes = []
        flatten(tree, nodes)
        for i, (a, b, c) in enumerate(nodes):
            v[k, i], t[k, i], s[k, i] = a, b, c
    return v, t, s


# ---- groups -------------------------------------------------------------------------------------------------------------------------
ARITH = [F[n] for n in ("ADD", "SUB", "MUL", "DIV")]
PAPER7 = ARITH + [F["SIN"], F["COS"], F["TAN"]]
GROUPS = {
    # name: generate arguments, inputs, how many drawn trees to keep, which sizes, hand rows
    "arith": dict(L=64, out_len=1, mlc=5, rou=uniform(ARITH), keys=[20261, 1], cs=NONZERO, lo=-3.0, hi=3.0, keep=100, sizes=(3, 64), hand=HAND_ARITH, xseed=11),
    "paper7": dict(L=64, out_len=1, mlc=4, rou=uniform(PAPER7), keys=[20261, 2], cs=NONZERO, lo=-3.0, hi=3.0, keep=100, sizes=(3, 64), hand=HAND_ARITH, xseed=12),
    "wide_pos": dict(L=64, out_len=1, mlc=4, rou=uniform(ex.TRUTH_FUNCS), keys=[20261, 3], lo=0.5, hi=3.0, keep=100, sizes=(3, 64),
                     hand=HAND_WIDE + HAND_POS, xseed=13),
    "wide_signed": dict(L=64, out_len=1, mlc=4, rou=uniform(ex.TRUTH_FUNCS), keys=[20261, 4], lo=-3.0, hi=3.0, keep=100, sizes=(3, 64),
                        hand=HAND_WIDE, xseed=14),
    "long": dict(L=256, out_len=1, mlc=8, leaf=0.08, rou={F["ADD"]: 0.62, F["SUB"]: 0.10, F["MUL"]: 0.24, F["DIV"]: 0.04}, keys=[20261, 5],
                 cs=[1.0, 0.5, 2.0], lo=0.5, hi=1.5, keep=100, sizes=(100, 250), hand=[], xseed=15),
    "mo3": dict(L=64, out_len=3, mlc=5, out_prob=0.9, rou=uniform([F[n] for n in ("ADD", "SUB", "MUL", "MAX", "NEG")]), keys=[20261, 6],
                lo=-3.0, hi=3.0, keep=80, sizes=(3, 64), hand=HAND_MO3, xseed=16),
}
VAR_LEN = 3
DRAW = 4000


def draw_inputs(seed, lo, hi):
    """100 distinct rows of U(lo, hi); a row with a coordinate within 0.05 of zero or of another coordinate is drawn again, so that the
    hand-written rows (DIV(x0, x1), IF(x0 - x1, ...)) are regular on every row"""
    r = np.random.default_rng(seed)
    rows = []
    while len(rows) < ROWS:
        x = r.uniform(lo, hi, VAR_LEN).astype(np.float32)
        gaps = [abs(float(x[i]) - float(x[j])) for i in range(VAR_LEN) for j in range(i)]
        if np.abs(x).min() >= 0.05 and min(gaps) >= 0.05:
            rows.append(x)
    return np.stack(rows)


# ---- multi-output trees on which the reference says nothing usable -------------------------------------------------------------------
def multi_output_verdict(type_, size):
    """'unary_out' / 'contradiction' / None.  A pushed value is TAINTED where the two statements of the reference may differ on it: a
    function node without the OUT flag pushes its own result in tree.py:322-323 and its last operand in forward.cu:241; an OUT node
    pushes its last operand in both.  The statements agree on a tree when no OUT node reads a tainted operand."""
    stack = []
    for i in range(int(size[0]) - 1, -1, -1):
        t = int(type_[i]) & 0xFF
        kind, out = t & 0x7F, bool(t & 0x80)
        if kind <= 1:
            stack.append(False); continue
        ops = [stack.pop() for _ in range(kind - 1)]
        if out and kind == 2:
            return "unary_out"
        if out and any(ops):
            return "contradiction"
        stack.append(ops[-1] if out else True)
    return None


# ---- the reference's expression and its value ------------------------------------------------------------------------------------------
def to_mp(r):
    """a sympy number (what the Loose* classes return) as an mpmath number of the working precision"""
    return r._to_mpmath(mp.prec) if isinstance(r, sp.Basic) else r


LOOSE = {name: (lambda cls: lambda *a: to_mp(cls.eval(*a)))(getattr(ref_utils, name)) for name in ("LooseDiv", "LooseInv", "LooseLog")}


def reference_function(value, type_, size, out_len):
    """the reference's Tree -> its sympy expression(s) -> a function of mpmath numbers; raises where the reference or sympy does"""
    n = int(size[0])
    vals = np.empty(len(value), object)
    for i in range(len(value)):
        kind = int(type_[i]) & 0x7F
        if i < n and kind == 1:
            vals[i] = sp.Rational(*float(value[i]).as_integer_ratio())     # exact: every float32 is a dyadic rational
        elif i < n and kind == 0:
            vals[i] = int(value[i])
        else:
            vals[i] = value[i]                                             # np.float32: a function id, or the packed word of an OUT node
    tree = Tree(VAR_LEN, out_len, vals, np.asarray(type_), np.asarray(size))
    expr = tree.to_sympy_expr()
    exprs = [sp.sympify(e) for e in (expr if out_len > 1 else [expr])]
    for e in exprs:
        if e.has(sp.zoo, sp.nan, sp.oo, sp.I) or e.is_real is False:
            raise ValueError("sympy folded the tree to a value that is no real number")
    syms = sp.symbols(f"x:{VAR_LEN}", real=True)
    return [sp.lambdify(syms, e, modules=[LOOSE, "mpmath"]) for e in exprs]


def truth_of(fns, X):
    T = np.full((X.shape[0], len(fns)), np.nan)
    ok = np.zeros(T.shape, bool)
    for d in range(X.shape[0]):
        args = [mp.mpf(float(x)) for x in X[d]]
        for o, fn in enumerate(fns):
            try:
                r = to_mp(fn(*args))
                if isinstance(r, (complex, mpmath.mpc)):
                    if r.imag != 0:
                        continue
                    r = r.real
                T[d, o] = float(mp.mpf(r))
                ok[d, o] = bool(np.isfinite(T[d, o]))
            except (ZeroDivisionError, ValueError, TypeError, OverflowError, mpmath.libmp.NoConvergence):
                continue
    return T, ok


def save(path, arrays):
    """a compressed npz whose bytes depend on its contents alone (numpy's own writer stamps the time of day into every member)"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def make(name, g, oracle):
    L, out_len = g["L"], g["out_len"]
    drawn = oracle.generate(DRAW, L, VAR_LEN, out_len, g.get("out_prob", 0.5), 0.3, g["keys"], depth2leaf(g["mlc"], g.get("leaf", 0.2)),
                            roulette(g["rou"]), g.get("cs", CS))
    hv, ht, hs = hand_rows(g["hand"], L)
    X = draw_inputs(g["xseed"], g["lo"], g["hi"])
    counts = dict(considered=0, wrong_size=0, unary_out=0, contradiction=0, few_outputs=0, export_failed=0)
    rows, T, OK, exported, hand = [], [], [], [], []

    def take(v, t, s, is_hand):
        try:
            fns = reference_function(v, t, s, out_len)
            tt, ok = truth_of(fns, X)
            good = True
        except Exception as e:  # noqa: BLE001  (whatever the reference or sympy raises: the tree has no truth)
            assert not is_hand, f"{name}: a hand-written row does not export: {e!r}"
            counts["export_failed"] += 1
            tt, ok, good = np.full((ROWS, out_len), np.nan), np.zeros((ROWS, out_len), bool), False
        rows.append((v, t, s)); T.append(tt); OK.append(ok); exported.append(good); hand.append(is_hand)

    for k in range(len(g["hand"])):
        assert oracle.validate_tree(ht[k], hs[k]) == 0
        if out_len > 1:
            assert multi_output_verdict(ht[k], hs[k]) is None
        take(hv[k], ht[k], hs[k], True)
    kept = 0
    for k in range(DRAW):
        if kept == g["keep"]:
            break
        v, t, s = drawn[0][k], drawn[1][k], drawn[2][k]
        if not (g["sizes"][0] <= int(s[0]) <= g["sizes"][1]) or oracle.validate_tree(t, s) != 0:
            counts["wrong_size"] += 1; continue
        if out_len > 1:
            verdict = multi_output_verdict(t, s)
            if verdict:
                counts[verdict] += 1; continue
            if ex.written_outputs(v[None], t[None], s[None], out_len).sum() < 2:     # a tree that writes one output or none shows no accumulation
                counts["few_outputs"] += 1; continue
        counts["considered"] += 1
        take(v, t, s, False)
        kept += 1
    assert kept == g["keep"], f"{name}: only {kept} usable trees among {DRAW} drawn"
    value, type_, size = (np.stack([r[i] for r in rows]) for i in range(3))
    cut = int(size[:, 0].max())
    header = dict(group=name, out_len=out_len, var_len=VAR_LEN, gp_len=L, functions=sorted(int(f) for f in g["rou"]), generate_keys=g["keys"],
                  max_layer_cnt=g["mlc"], input_seed=g["xseed"], input_range=[g["lo"], g["hi"]], const_samples=g.get("cs", CS), digits=mp.dps,
                  sympy=sp.__version__, mpmath=mpmath.__version__, hand_rows=len(g["hand"]), left_out=counts)
    arrays = dict(value=value[:, :cut], type=type_[:, :cut], size=size[:, :cut], X=X, T=np.stack(T), mp_ok=np.stack(OK), exported=np.array(exported),
                  hand=np.array(hand), header=np.frombuffer(json.dumps(header, sort_keys=True).encode(), dtype=np.uint8))
    path = os.path.join(HERE, f"sympy_truth_{name}.npz")
    save(path, arrays)
    # the counts the tests assert, printed where the fixture is made: a floor that is missed here is met by other inputs or descriptors
    ex._groups.pop(name, None)
    gr = ex.group(name)
    share, tight = gr.shares()
    live = gr.compared & gr.counted
    dev = np.abs(gr.V - gr.T)[gr.regular] / np.maximum(np.abs(gr.T[gr.regular]), 1e-300)
    print(f"{name}: {len(exported)} trees ({len(g['hand'])} by hand), L {cut}, left out {counts}, regular {gr.regular[gr.exported].mean():.3f}, "
          f"compared {share:.3f} (floor {ex.FLOORS[name]}), tight {tight:.3f}, hand rows fully compared {bool(gr.compared[gr.hand].all())}, "
          f"float64 helper off by {dev.max():.2e} at most, compared entries with T != 0: {(gr.T[live] != 0).mean():.3f}, median size {int(np.median(size[:, 0]))}, "
          f"{os.path.getsize(path)} bytes")
    return gr


def main():
    oracle = Oracle("port")
    census = {}
    for name, g in GROUPS.items():
        if len(sys.argv) > 1 and name not in sys.argv[1:]:
            continue
        gr = make(name, g, oracle)
        for f, n in ex.function_census(gr).items():
            census[f] = census.get(f, 0) + n
    print("trees per function with at least half their rows compared:", {ex.NAMES[f]: census.get(f, 0) for f in ex.TRUTH_FUNCS})


if __name__ == "__main__":
    main()
