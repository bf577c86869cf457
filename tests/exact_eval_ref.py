"""TEST-ONLY: a plain node-by-node evaluator of a forest on a set of rows with the project's semantics (the prefix array read backwards
over an operand stack, forward.cu:79-244), float64 results computed in the host's widest float (x87 extended where numpy has it: 2^-64 per
operation, so that its own rounding stays below 1e-10 B), which also carries what nothing else in the
tests has:

  * a first-order RUNNING ERROR BOUND `B` of a correct float32 evaluation of the same tree: a leaf has 0 (the inputs and constants are
    float32, taken exactly); an arithmetic node adds 2^-24 |value| (half an ulp) to sum |d/d child| B_child; a division or inverse adds
    one ulp, 2^-23 |value| (the default division is the faithfully rounded sequence); a library node adds bound_f 2^-23 |value| with
    bound_f from tests/ulp_bounds.py (the larger of its routes and ranges); neg, abs, max, min and if round nothing;
  * a REGULAR flag per (tree, row): every node of the tree on that row is finite and inside float32's normal range, inside its domain
    (log, sqrt and pow base > 0 where the function requires it; the loose functions away from their zero operand, where the reference's
    sympy classes differ from the kernels), no division or inverse by |d| < 1e-3, no max / min within 1e-3 relative of a tie (two exact operands that are equal are no tie: either is the value), no `if`
    condition within 1e-3 of its threshold -- nor a tie or threshold closer than twice the operands' own error bounds.

Both come from this side only, never from the code under test.  tests/test_sympy_truth.py holds the evaluator itself to the
reference-held truth of tests/golden/sympy_truth_*.npz (1e-12 relative wherever an entry carries digits), so it cannot drift.  The four comparisons (< > <= >=) are
evaluated (+-1) but never regular: the truth does not cover them.  No GPU import."""
import os

import numpy as np

import ulp_bounds

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GROUPS = ("arith", "paper7", "wide_pos", "wide_signed", "long", "mo3")
FLOORS = {"arith": 0.9, "paper7": 0.9, "wide_pos": 0.9, "wide_signed": 0.5, "long": 0.9, "mo3": 0.9}   # share of entries compared

U = 2.0 ** -24          # half an ulp, relative: one correctly rounded float32 operation
ULP = 2.0 ** -23        # one ulp, relative
NEAR = 1e-3             # the margin of "regular"
RTOL = 1e-5             # the project's bar
NO_DIGITS = 1e-3        # B beyond this share of |T|: the entry carries no digits
FLT_MAX, FLT_MIN = 3.4028234663852886e38, 1.1754943508222875e-38
WIDE = np.longdouble   # the evaluator's working type: the host's widest float (x87 extended: 64 bits), results returned as float64

NAMES = ["IF", "ADD", "SUB", "MUL", "DIV", "LOOSE_DIV", "POW", "LOOSE_POW", "MAX", "MIN", "LT", "GT", "LE", "GE", "SIN", "COS", "TAN", "SINH", "COSH",
         "TANH", "LOG", "LOOSE_LOG", "EXP", "INV", "LOOSE_INV", "NEG", "ABS", "SQRT", "LOOSE_SQRT"]
F = {n: i for i, n in enumerate(NAMES)}
COMPARISONS = (F["LT"], F["GT"], F["LE"], F["GE"])
TRUTH_FUNCS = [f for f in range(29) if f not in COMPARISONS]     # the 25 functions the truth covers


def lib_bound(name):
    """ulps granted to one call of a library function: the largest of its routes (register kernels, threaded code) and ranges"""
    b = list((ulp_bounds.UNARY.get(name) or ulp_bounds.BINARY[name])[:2])
    if name in ulp_bounds.LARGE:
        b += list(ulp_bounds.LARGE[name])
    return max(b)


def _unary(f, a, Ba):
    """-> value, bound, regular of a unary node over the rows"""
    with np.errstate(all="ignore"):
        ok = np.ones(a.shape, bool)
        absa = np.abs(a)
        if f == F["NEG"]:
            return -a, Ba, ok
        if f == F["ABS"]:
            return absa, Ba, ok
        name = NAMES[f]
        if f == F["SIN"]:
            v, d = np.sin(a), np.abs(np.cos(a))
        elif f == F["COS"]:
            v, d = np.cos(a), np.abs(np.sin(a))
        elif f == F["TAN"]:
            v = np.tan(a); d = 1.0 + v * v
        elif f == F["SINH"]:
            v, d = np.sinh(a), np.cosh(a)
        elif f == F["COSH"]:
            v, d = np.cosh(a), np.abs(np.sinh(a))
        elif f == F["TANH"]:
            v = np.tanh(a); d = 1.0 - v * v
        elif f in (F["LOG"], F["LOOSE_LOG"]):
            ok = a > 0 if f == F["LOG"] else a != 0
            v, d = np.log(absa), 1.0 / absa
        elif f == F["EXP"]:
            v = np.exp(a); d = v
        elif f in (F["INV"], F["LOOSE_INV"]):
            ok = absa >= NEAR
            v = 1.0 / a; d = v * v
            return v, d * Ba + ULP * np.abs(v), ok
        elif f in (F["SQRT"], F["LOOSE_SQRT"]):
            ok = a >= 0 if f == F["SQRT"] else ok
            v = np.sqrt(absa)
            d = np.where(v > 0, 0.5 / np.where(v > 0, v, 1.0), np.where(Ba > 0, np.inf, 0.0))
        else:   # an id without a function leaves the zero-initialised result (forward.cu:117); nothing the truth speaks about
            return np.zeros_like(a), np.zeros_like(a), np.zeros(a.shape, bool)
        B = np.where(Ba > 0, d * Ba, 0.0) + lib_bound(name) * ULP * np.abs(v)
        return v, B, ok


def _binary(f, a, b, Ba, Bb):
    with np.errstate(all="ignore"):
        ok = np.ones(a.shape, bool)
        if f == F["ADD"] or f == F["SUB"]:
            v = a + b if f == F["ADD"] else a - b
            return v, Ba + Bb + U * np.abs(v), ok
        if f == F["MUL"]:
            v = a * b
            return v, np.abs(b) * Ba + np.abs(a) * Bb + U * np.abs(v), ok
        if f in (F["DIV"], F["LOOSE_DIV"]):
            ok = np.abs(b) >= NEAR
            v = a / b
            return v, (Ba + np.abs(v) * Bb) / np.abs(b) + ULP * np.abs(v), ok
        if f in (F["POW"], F["LOOSE_POW"]):
            base = a if f == F["POW"] else np.abs(a)
            ok = base > 0
            v = np.power(np.where(ok, base, 1.0), b)
            B = np.abs(b * v / np.where(ok, base, 1.0)) * Ba + np.abs(v * np.log(np.where(ok, base, 1.0))) * Bb + lib_bound(NAMES[f]) * ULP * np.abs(v)
            return v, B, ok
        if f in (F["MAX"], F["MIN"]):
            first = a >= b if f == F["MAX"] else a <= b
            gap = np.abs(a - b)
            ok = (gap > NEAR * np.maximum(np.abs(a), np.abs(b))) & (gap > 2.0 * (Ba + Bb))
            ok |= (a == b) & (Ba == 0) & (Bb == 0)   # the same exact number twice (max(x0, x0), a forwarded operand): either choice is that number
            return np.where(first, a, b), np.where(first, Ba, Bb), ok
        if f in COMPARISONS:
            t = {F["LT"]: a < b, F["GT"]: a > b, F["LE"]: a <= b, F["GE"]: a >= b}[f]
            return np.where(t, 1.0, -1.0), np.zeros_like(a), np.zeros(a.shape, bool)
        return np.zeros_like(a), np.zeros_like(a), np.zeros(a.shape, bool)


def evaluate(value, type_, size, X, out_len):
    """-> V float64 [trees][rows][out_len], B (same shape), regular bool [trees][rows]"""
    value, type_, size = np.asarray(value, np.float32), np.asarray(type_), np.asarray(size)
    X = np.asarray(X, np.float32).astype(WIDE)
    n, D = value.shape[0], X.shape[0]
    multi = out_len > 1
    V = np.zeros((n, D, out_len)); BB = np.zeros((n, D, out_len)); REG = np.ones((n, D), bool)
    zero = np.zeros(D, WIDE)
    for k in range(n):
        stack = []
        outs = [(zero, zero) for _ in range(out_len)]
        reg = np.ones(D, bool)
        for i in range(int(size[k, 0]) - 1, -1, -1):
            t, v = int(type_[k, i]), value[k, i]
            is_out = bool(t & 0x80) if multi else False
            t &= 0x7F if multi else 0xFFFF
            if t == 1:
                stack.append((np.full(D, float(v), WIDE), zero)); continue
            if t == 0:
                stack.append((X[:, int(v)], zero)); continue
            f, oi = int(v), 0
            if is_out:
                w = int(np.float32(v).view(np.uint32))
                f, oi = w & 0xFFFF, w >> 16
            if t == 2:
                a, Ba = stack.pop()
                last = (a, Ba)
                r, Br, ok = _unary(f, a, Ba)
            elif t == 3:
                a, Ba = stack.pop(); b, Bb = stack.pop()
                last = (b, Bb)
                r, Br, ok = _binary(f, a, b, Ba, Bb)
            else:
                a, Ba = stack.pop(); b, Bb = stack.pop(); c, Bc = stack.pop()
                last = (c, Bc)
                ok = (np.abs(a) > NEAR) & (np.abs(a) > 2.0 * Ba)
                r, Br = np.where(a > 0, b, c), np.where(a > 0, Bb, Bc)
            with np.errstate(all="ignore"):
                mag = np.abs(r)
                reg &= ok & np.isfinite(r) & (mag <= FLT_MAX) & ((mag >= FLT_MIN) | (r == 0))
            if multi:
                if is_out and oi < out_len:
                    acc, Bacc = outs[oi]
                    with np.errstate(all="ignore"):
                        acc = acc + r
                        outs[oi] = (acc, Bacc + Br + U * np.abs(acc))
                stack.append(last)
            else:
                stack.append((r, Br))
        assert len(stack) == 1, f"tree {k} is malformed"
        if not multi:
            outs = [stack[0]]
        with np.errstate(over="ignore"):   # beyond float64: inf, and irregular long before
            for o in range(out_len):
                V[k, :, o], BB[k, :, o] = outs[o]
        REG[k] = reg
    return V, BB, REG


# ---- the fixture and what a test derives from it ----------------------------------------------------------------------------------
class Group:
    """One tests/golden/sympy_truth_<group>.npz with everything the tests share, computed once: the truth T, the helper's own values,
    the bounds, which entries are compared and with what tolerance.  `rows(D)` gives the views for the first 8 rows, all 100, or the
    100 tiled to 600 (the 1-, 4- and 8-row interpreter builds)."""

    def __init__(self, name):
        import json

        z = np.load(os.path.join(GOLD, f"sympy_truth_{name}.npz"))
        self.name = name
        self.header = json.loads(bytes(z["header"]).decode())
        self.out_len, self.var_len = int(self.header["out_len"]), int(self.header["var_len"])
        self.forest = (z["value"], z["type"], z["size"])
        self.X, self.exported, self.hand = z["X"], z["exported"], z["hand"]
        self.T = z["T"].reshape(len(self.exported), self.X.shape[0], self.out_len)
        self.mp_ok = z["mp_ok"].reshape(self.T.shape)
        self.V, self.B, reg = evaluate(*self.forest, self.X, self.out_len)
        self.regular = reg[:, :, None] & self.mp_ok & self.exported[:, None, None] & np.isfinite(self.T)
        with np.errstate(all="ignore"):
            self.compared = self.regular & (self.B <= NO_DIGITS * np.abs(self.T))
        self.tol = RTOL * np.abs(self.T) + 2.0 * self.B
        # an output that no OUT node of the tree writes is 0 on both sides: it is compared (exactly), but it is no evidence, so the
        # shares the floors are about are taken over the outputs some node writes (every output of a single-output tree)
        self.written = written_outputs(*self.forest, self.out_len)
        self.counted = self.written[:, None, :] & self.exported[:, None, None] & np.ones(self.T.shape, bool)

    def shares(self):
        """-> (share of the entries compared, share of the compared entries whose grant is at most twice the 1e-5 bar), both over the
        written outputs of the trees that have a truth (`exported`; the trees without one are capped separately, from the header)"""
        c = self.compared & self.counted
        return c.sum() / self.counted.sum(), (self.tol[c] <= 2.0 * RTOL * np.abs(self.T[c])).mean()

    def rows(self, D):
        n = self.X.shape[0]
        idx = np.arange(D) % n if D > n else np.arange(D)
        return self.X[idx], idx

    def labels(self, idx):
        """the fitness labels: a fixed expression of X, float32"""
        X = self.X[idx]
        if self.out_len == 1:
            return (X[:, 0] * X[:, 1] + X[:, 2] - np.float32(0.5)).astype(np.float32)[:, None]
        cols = [X[:, 0] + X[:, 1], X[:, 1] * X[:, 2], X[:, 0] - X[:, 2]]
        return np.stack([cols[o % 3] for o in range(self.out_len)], 1).astype(np.float32)

    def fitness_truth(self, idx, use_mse):
        """-> truth float64 [trees], tolerance, which trees are compared (all their rows and outputs are)"""
        y = self.labels(idx).astype(np.float64)
        T, tol = self.T[:, idx], self.tol[:, idx]
        full = self.compared[:, idx].all((1, 2))
        D = len(idx)
        with np.errstate(all="ignore"):
            diff = np.abs(y[None] - T)
            if use_mse:
                truth = (diff * diff).sum(2).mean(1)
                ftol = (2.0 * diff * tol + tol * tol).sum(2).mean(1) + D * U * truth
            else:
                truth = diff.sum(2).mean(1)
                ftol = tol.sum(2).mean(1) + D * U * truth
        return truth, ftol, full


def written_outputs(value, type_, size, out_len):
    """bool [trees][out_len]: the outputs at least one OUT node of the tree adds to (all of them for single-output trees)"""
    n = len(value)
    if out_len == 1:
        return np.ones((n, 1), bool)
    w = np.zeros((n, out_len), bool)
    for k in range(n):
        for i in range(int(size[k, 0])):
            t = int(type_[k, i])
            if (t & 0x80) and (t & 0x7F) >= 2:
                o = int(np.float32(value[k, i]).view(np.uint32)) >> 16
                if o < out_len:
                    w[k, o] = True
    return w


_groups = {}


def group(name):
    if name not in _groups:
        _groups[name] = Group(name)
    return _groups[name]


def worst_ratio(got, T, tol, mask):
    """max |got - T| / tol over the compared entries (an entry whose tolerance is 0 must be met exactly)"""
    got = np.asarray(got, np.float64)
    assert got.shape == T.shape, (got.shape, T.shape)
    if not mask.any():
        return 0.0
    err = np.abs(got[mask] - T[mask])
    t = tol[mask]
    with np.errstate(all="ignore"):
        ratio = np.where(err == 0, 0.0, err / np.where(t > 0, t, np.nan))
    ratio = np.where(np.isnan(ratio), np.inf, ratio)       # a NaN result, or any error where none is granted
    return float(ratio.max())


def function_census(g):
    """-> {function id: trees of the group that use it and have at least half their rows compared}"""
    value, type_, size = g.forest
    half = g.compared.all(2).mean(1) >= 0.5
    out = {}
    for k in np.flatnonzero(half):
        seen = set()
        for i in range(int(size[k, 0])):
            t = int(type_[k, i])
            if (t & 0x7F) >= 2:
                seen.add(int(np.float32(value[k, i]).view(np.uint32)) & 0xFFFF if (t & 0x80) else int(value[k, i]))
        for f in seen:
            out[f] = out.get(f, 0) + 1
    return out


# ---- the assertions both test files share --------------------------------------------------------------------------------------------
def copies(g, idx):
    """the forest with one copy of every tree per row of idx, and the rows to go with them: what `evaluate` (one row per tree) takes"""
    n = len(g.exported)
    forest = tuple(np.repeat(a, len(idx), axis=0) for a in g.forest)
    return forest, np.tile(g.X[idx], (n, 1))


def assert_entries(got, g, idx, what, report=None):
    """every compared entry of got [trees][rows][out_len] within its own tolerance of the truth; no allowed-bad fraction"""
    got = np.asarray(got, np.float64).reshape(len(g.exported), len(idx), g.out_len)
    T, tol, mask = g.T[:, idx], g.tol[:, idx], g.compared[:, idx]
    ratio = worst_ratio(got, T, tol, mask)
    if report is not None:
        report[what] = ratio
    if not ratio <= 1.0:
        with np.errstate(all="ignore"):
            r = np.where(mask, np.abs(got - T) / tol, 0.0)
        r = np.where(mask & ~(np.abs(got - T) <= tol), np.where(np.isfinite(r), r, np.inf), 0.0)
        k, d, o = np.unravel_index(np.argmax(r), r.shape)
        raise AssertionError(f"{what}: tree {k} row {idx[d]} output {o}: got {got[k, d, o]!r}, truth {T[k, d, o]!r}, granted {tol[k, d, o]:.3g} "
                             f"(B {g.B[k, idx[d], o]:.3g}); {int((r > 0).sum())} of {int(mask.sum())} compared entries beyond their tolerance")


def assert_fitness(got, g, idx, use_mse, what, report=None):
    truth, ftol, full = g.fitness_truth(idx, use_mse)
    got = np.asarray(got, np.float64)
    assert full.mean() >= 0.4, f"{what}: only {full.mean():.0%} of the trees have all their rows compared"
    ratio = worst_ratio(got, truth, ftol, full)
    if report is not None:
        report[what] = ratio
    if not ratio <= 1.0:
        bad = full & ~(np.abs(got - truth) <= ftol)
        k = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{what}: tree {k}: got {got[k]!r}, truth {truth[k]!r}, granted {ftol[k]:.3g}; {int(bad.sum())} of {int(full.sum())} trees beyond their tolerance")
