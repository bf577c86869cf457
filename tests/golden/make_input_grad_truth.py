#!/usr/bin/env python3
"""The partial derivatives of whole trees on data rows, from a source that does not descend from the adjoint table: the REFERENCE's sympy
export of the tree (`Tree.to_sympy_expr`, imported as tests/golden/make_sympy_truth.py imports it), lambdified on mpmath and differentiated
NUMERICALLY at 50 digits (`mpmath.diff`, central differences at twice the working precision).  Nothing here knows a derivative rule of
ours; for the two groups whose functions sympy differentiates in closed form (`arith`, `paper7`) the script also evaluates `sympy.diff` of
the export at 50 digits and asserts that it agrees with the numeric derivative to 1e-20 relative, which validates the differentiator.

The trees and X are those of the committed tests/golden/sympy_truth_<group>.npz (single-output groups), first ROWS rows.  Written per group
to tests/golden/input_grad_truth_<group>.npz (data only): dT float64 [trees][ROWS][3], d_ok bool of the same shape, and a JSON header
with the versions, the counts and what was left out.  An entry has a truth (d_ok) when the export exists, both step sizes give a real
finite number and they agree to 1e-15 relative.

The script prints, per group, the share of the entries of these rows that a test compares -- d_ok, the exclusion rule of
tests/input_grad_ref.py `comparable`, and a value on which the export states the function the device computes (`regular` in
tests/exact_eval_ref.py) -- and asserts the group's floor minus 0.05.

    python tests/golden/make_input_grad_truth.py [group ...]      (needs what make_sympy_truth.py needs: the reference's sources, sympy, mpmath;
                                                                   it runs where the fixtures are made, never under pytest)
"""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_sympy_truth as M  # noqa: E402  (puts the reference package and tests/ on the path; no op of the reference is called)

import mpmath  # noqa: E402
import sympy as sp  # noqa: E402
from mpmath import mp  # noqa: E402

import exact_eval_ref as ex  # noqa: E402
import input_grad_ref as XR  # noqa: E402

GROUPS = ("arith", "paper7", "wide_pos", "wide_signed", "long")
SYMBOLIC = ("arith", "paper7")
FLOORS = {"arith": 0.90, "paper7": 0.90, "wide_pos": 0.90, "wide_signed": 0.80, "long": 0.90}
ROWS = 32
STEPS = (None, mp.ldexp(1, -150))   # mpmath's own step (2^-176 at 50 digits) and a coarser one
AGREE = mp.mpf(10) ** -15
SYM_AGREE = mp.mpf(10) ** -20
mp.dps = 50


def expression(value, type_, size):
    """the reference's export of a single-output tree, constants as exact rationals (make_sympy_truth.reference_function's first half)"""
    n = int(size[0])
    vals = np.empty(len(value), object)
    for i in range(len(value)):
        kind = int(type_[i]) & 0x7F
        if i < n and kind == 1:
            vals[i] = sp.Rational(*float(value[i]).as_integer_ratio())
        elif i < n and kind == 0:
            vals[i] = int(value[i])
        else:
            vals[i] = value[i]
    e = sp.sympify(M.Tree(M.VAR_LEN, 1, vals, np.asarray(type_), np.asarray(size)).to_sympy_expr())
    if e.has(sp.zoo, sp.nan, sp.oo, sp.I) or e.is_real is False:
        raise ValueError("sympy folded the tree to a value that is no real number")
    return e


def real(r):
    """an mpmath real from what a lambdified export returns, or None"""
    r = M.to_mp(r)
    if isinstance(r, (complex, mpmath.mpc)):
        if r.imag != 0:
            return None
        r = r.real
    r = mp.mpf(r)
    return r if mp.isfinite(r) else None


class NoValue(Exception):
    pass


def numeric(fn, args, k, h):
    order = tuple(1 if j == k else 0 for j in range(M.VAR_LEN))

    def f(*a):
        r = real(fn(*a))
        if r is None:
            raise NoValue
        return r

    return mp.diff(f, tuple(args), order) if h is None else mp.diff(f, tuple(args), order, h=h)


def close(a, b, rel):
    return abs(a - b) <= rel * max(abs(a), abs(b))


def make(name):
    z = np.load(os.path.join(HERE, f"sympy_truth_{name}.npz"))
    value, type_, size, X, exported = z["value"], z["type"], z["size"], z["X"][:ROWS], z["exported"]
    n = len(exported)
    dT = np.full((n, ROWS, M.VAR_LEN), np.nan)
    ok = np.zeros(dT.shape, bool)
    syms = sp.symbols(f"x:{M.VAR_LEN}", real=True)
    counts = dict(no_export=0, no_value=0, steps_disagree=0, symbolic_checked=0)
    worst_sym = mp.mpf(0)
    for t in range(n):
        if not exported[t]:
            counts["no_export"] += ROWS * M.VAR_LEN
            continue
        e = expression(value[t], type_[t], size[t])
        fn = sp.lambdify(syms, e, modules=[M.LOOSE, "mpmath"])
        dfn = [sp.lambdify(syms, sp.diff(e, s), modules="mpmath") for s in syms] if name in SYMBOLIC else None
        for d in range(ROWS):
            args = [mp.mpf(float(x)) for x in X[d]]
            for k in range(M.VAR_LEN):
                try:
                    a, b = (numeric(fn, args, k, h) for h in STEPS)
                except (NoValue, ZeroDivisionError, ValueError, TypeError, OverflowError, mpmath.libmp.NoConvergence):
                    counts["no_value"] += 1
                    continue
                if not (mp.isfinite(a) and mp.isfinite(b) and close(a, b, AGREE)):
                    counts["steps_disagree"] += 1
                    continue
                dT[t, d, k], ok[t, d, k] = float(a), bool(np.isfinite(float(a)))
                if dfn is not None:
                    s = real(dfn[k](*args))
                    assert s is not None and close(s, a, SYM_AGREE), (name, t, d, k, s, a)
                    if a != 0:
                        worst_sym = max(worst_sym, abs(s - a) / abs(a))
                    counts["symbolic_checked"] += 1
    # the share a test compares on these rows: d_ok, the exclusion rule (from the restatement alone) and a regular value
    rule = XR.comparable(value, type_, size, X.astype(np.float64), list(range(M.VAR_LEN))).transpose(1, 2, 0)
    regular = ex.group(name).regular[:, :ROWS, :1]
    share = float((ok & rule & regular).mean())
    header = dict(group=name, rows=ROWS, var_len=M.VAR_LEN, digits=mp.dps, steps=["mpmath default (2^-176)", "2^-150"], agree=1e-15,
                  symbolic_agree=1e-20 if name in SYMBOLIC else None, worst_symbolic=float(worst_sym), sympy=sp.__version__,
                  mpmath=mpmath.__version__, entries=int(ok.size), d_ok=int(ok.sum()), rule=int(rule.sum()), compared=int((ok & rule & regular).sum()),
                  left_out=counts)
    path = os.path.join(HERE, f"input_grad_truth_{name}.npz")
    M.save(path, dict(dT=dT, d_ok=ok, header=np.frombuffer(json.dumps(header, sort_keys=True).encode(), dtype=np.uint8)))
    print(f"{name}: {n} trees x {ROWS} rows x {M.VAR_LEN} variables, d_ok {ok.mean():.3f}, rule {rule.mean():.3f}, compared {share:.3f} "
          f"(floor {FLOORS[name]} - 0.05), left out {counts}, symbolic off by {float(worst_sym):.1e} at most, {os.path.getsize(path)} bytes", flush=True)
    assert share >= FLOORS[name] - 0.05, f"{name}: only {share:.3f} of the entries of the first {ROWS} rows are compared: take other rows"


def main():
    for name in GROUPS:
        if len(sys.argv) > 1 and name not in sys.argv[1:]:
            continue
        t0 = time.time()
        make(name)
        print(f"  ({time.time() - t0:.0f} s)", flush=True)


if __name__ == "__main__":
    main()
