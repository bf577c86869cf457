"""GPU: the device adjoint table (csrc/sr_adjoint.hpp) rule by rule, read directly off probe trees (tests/adjoint_battery.py), through
the four call sites that read the header:

    single_lds     tree_SR_gradient, one output, gp_len 64: the tape in LDS, r read from the tape
    multi          tree_SR_gradient, two outputs, gp_len 64: the probed node carries the OUT flag to output 0 (output 1 has label 0);
                   r is recomputed in the reverse walk
    single_global  tree_SR_gradient, one output, gp_len 128: the smallest row whose tape leaves LDS
    lm             tree_SR_normal_eq, gp_len 64, label 0: A_ij = d_i d_j, b_i = d_i pred (the Jacobian walk, seeded with 1)

each with the direct form f(c...) and the stacked form f(ADD(c, x0)...), for all 29 functions and two unknown function ids.  One tree per
operand point, D = 1, MAE: the gradient word at a CONST operand is the fp32 value of the rule itself.  Per function and route:

  * every planted edge cell of the table: class and value exact (a zero == 0, NaN NaN, "g" the bits of 1.0f, a correctly rounded
    chain its bits);
  * every drawn point: the NaN / zero / infinity class of the float64 truth, and on the points of the accuracy comparison
        |word - truth| <= BOUND[f][route] * u,      u the derived unit of the point (adjoint_battery.units)
    with the EXACT rules (ADD SUB MAX MIN IF NEG ABS, the comparisons, unknown ids) compared bit for bit instead;
  * cross-route identities, bit for bit: LDS tape == global tape; stacked == direct (operands other than -0); a second launch; and
    the multi-output walk (r recomputed) == the single-output walk (r from the tape).

BOUND is the largest error measured on MI355X, rounded up to one decimal, and never above the a-priori CEILING of the rule (0.5 per
rounding operation as written + 1 for the propagated terms); this test writes the measured maxima to
sr_adjoint_report.json in the directory EVOGP_REPORT_DIR names, when it names one (profiles/sr_adjoint_01_report.json is a copy of
such a report; DESIGN.md section 3.7 quotes it).  A measured maximum above its ceiling is a bug or an effect to derive, never a
bound to pin.  The device turned out bit-identical between r recomputed and r read from the tape for the library-backed rules too
(TAN TANH EXP POW LOOSE_POW), so that identity is pinned for every rule."""
import functools
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adjoint_battery as AB  # noqa: E402
import sr_lm_ref as LM  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
GRAD_ROUTES = {"single_lds": (64, False), "multi": (64, True), "single_global": (128, False)}
ROUTES = list(GRAD_ROUTES) + ["lm"]
FORMS = ("direct", "stacked")
REPORT = {}

# Largest error MEASURED on MI355X per function and route in units u (profiles/sr_adjoint_01_report.json), rounded up to one decimal;
# every one is below the rule's ceiling.  A rule or a reverse walk that strays from the table's arithmetic by one rounding fails here.
MEASURED = {
    "MUL": dict(single_lds=0.0, multi=0.0, single_global=0.0, lm=0.3),
    "DIV": dict(single_lds=0.8, multi=0.8, single_global=0.8, lm=0.7),
    "LOOSE_DIV": dict(single_lds=0.7, multi=0.7, single_global=0.7, lm=0.7),
    "POW": dict(single_lds=1.0, multi=1.0, single_global=1.0, lm=1.0),
    "LOOSE_POW": dict(single_lds=1.0, multi=1.0, single_global=1.0, lm=1.0),
    "SIN": dict(single_lds=0.6, multi=0.6, single_global=0.6, lm=0.5),
    "COS": dict(single_lds=0.5, multi=0.5, single_global=0.5, lm=0.5),
    "TAN": dict(single_lds=0.7, multi=0.7, single_global=0.7, lm=0.6),
    "SINH": dict(single_lds=0.4, multi=0.4, single_global=0.4, lm=0.4),
    "COSH": dict(single_lds=0.5, multi=0.5, single_global=0.5, lm=0.4),
    "TANH": dict(single_lds=0.7, multi=0.7, single_global=0.7, lm=0.7),
    "LOG": dict(single_lds=0.5, multi=0.5, single_global=0.5, lm=0.5),
    "LOOSE_LOG": dict(single_lds=0.5, multi=0.5, single_global=0.5, lm=0.5),
    "EXP": dict(single_lds=0.4, multi=0.4, single_global=0.4, lm=0.4),
    "INV": dict(single_lds=0.8, multi=0.8, single_global=0.8, lm=0.7),
    "LOOSE_INV": dict(single_lds=0.8, multi=0.8, single_global=0.8, lm=0.8),
    "SQRT": dict(single_lds=0.8, multi=0.8, single_global=0.8, lm=0.7),
    "LOOSE_SQRT": dict(single_lds=0.8, multi=0.8, single_global=0.8, lm=0.7),
}
BOUND = {n: {r: MEASURED.get(n, {}).get(r, max(AB.CEILING[n])) for r in ROUTES} for n in AB.NAMES}
# b_i = d_i pred of the normal-equation route, in its own unit (_check_lm_route): a-priori ceiling 1, pinned at the measured maximum
MEASURED_B = {
    "ADD": 0.4, "SUB": 0.4, "MUL": 0.5, "DIV": 0.5, "LOOSE_DIV": 0.5, "POW": 0.4, "LOOSE_POW": 0.4, "MAX": 0.0,
    "MIN": 0.0, "LT": 0.0, "GT": 0.0, "LE": 0.0, "GE": 0.0, "SIN": 0.4, "COS": 0.4, "TAN": 0.4,
    "SINH": 0.4, "COSH": 0.4, "TANH": 0.3, "LOG": 0.7, "LOOSE_LOG": 0.6, "EXP": 0.4, "INV": 0.5, "LOOSE_INV": 0.5,
    "NEG": 0.0, "ABS": 0.0, "SQRT": 0.2, "LOOSE_SQRT": 0.2, "IF": 0.0, "UNKNOWN_U": 0.0, "UNKNOWN_B": 0.0,
}
for _n in AB.NAMES:
    BOUND[_n]["lm_b"] = MEASURED_B.get(_n, 1.0)


# ---- launches -----------------------------------------------------------------------------------------------------------------------
def _dev(*arrs):
    import torch

    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _gradient(value, type_, size, y, use_mse=False):
    import torch

    import evogp_amd  # noqa: F401  (registers the ops)

    pop, L = value.shape
    v, t, s, Xd, yd = _dev(value, type_, size, np.zeros((1, 1), F32), np.asarray(y, F32).reshape(1, -1))
    loss, grad = torch.ops.evogp_hip.tree_SR_gradient(pop, 1, L, 1, yd.shape[1], use_mse, v, t, s, Xd, yd)
    return loss.cpu().numpy(), grad.cpu().numpy()


def _normal_eq(value, type_, size):
    import torch

    import evogp_amd  # noqa: F401

    pop, L = value.shape
    v, t, s, Xd, yd = _dev(value, type_, size, np.zeros((1, 1), F32), np.zeros((1, 1), F32))
    loss, normal = torch.ops.evogp_hip.tree_SR_normal_eq(pop, 1, L, 1, 1, v, t, s, Xd, yd)
    return loss.cpu().numpy(), normal.cpu().numpy()


class Run:
    """one launch of one function through one route and form, with everything its checks need"""


@functools.lru_cache(maxsize=None)
def _run(name, route, form):
    r = Run()
    gp_len, multi = GRAD_ROUTES.get(route, (64, False))
    ops, r.n_draws, r.rule_tok, r.grad_tok, r.edge_idx = AB.points(name, form, multi)
    r.raw = ops
    r.ops = AB.effective_operands(ops, form, multi)
    r.forest = functools.partial(AB.probe_forest, name, ops, form, gp_len, multi)   # (rebuilt on demand: 250 launches are cached)
    value, type_, size, r.cpos = r.forest()
    r.pred = AB.forward(name, r.ops)
    if route == "lm":
        r.y = F32(0)
        r.loss, r.normal = _normal_eq(value, type_, size)
        return r
    r.y = AB.launch_label(r.pred)
    r.g = AB.out_adjoint(r.pred, r.y)
    r.loss, grad = _gradient(value, type_, size, [r.y, 0.0] if multi else [r.y])
    r.got = [grad[:, c].copy() for c in r.cpos]     # (the operand columns only: the cache must not keep every gradient array alive)
    rest = np.ones(gp_len, bool)
    rest[r.cpos] = False
    assert np.all(grad[:, rest].view(np.uint32) == 0), f"{name} via {route}/{form}: a word that is no CONST operand is not +0"
    return r


# ---- comparisons ------------------------------------------------------------------------------------------------------------------
THRESHOLD = AB.FLT_MAX + 2.0 ** 103     # a magnitude from here on rounds to an fp32 infinity


def _same_bits(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def _slack(want64, slack):
    """the error a word may carry next to the overflow threshold: the derived bound of the point, or half the truth's magnitude where
    no bound can be derived (a non-finite unit, an intermediate of the rule that itself overflows fp32)"""
    with np.errstate(all="ignore"):
        slack = np.broadcast_to(np.asarray(slack, np.float64), want64.shape)
        return np.where(np.isfinite(slack), slack, 0.5 * np.abs(want64))


def _check_class(got, want64, what, slack=0.0):
    """NaN where the truth is NaN, == 0 where it is zero, the signed infinity where the truth less its error bound still rounds to an
    fp32 infinity, finite where the truth plus its error bound stays below that threshold"""
    with np.errstate(all="ignore"):
        bad = np.isnan(got) != np.isnan(want64)
        assert not bad.any(), f"{what}: NaN sets differ at {np.flatnonzero(bad)[:5]}"
        zero = want64 == 0
        assert np.all(got[zero] == 0), f"{what}: {int((got[zero] != 0).sum())} words are not 0 where the table gives 0"
        s = _slack(want64, slack)
        big = np.abs(want64) - s >= THRESHOLD
        assert np.array_equal(got[big], np.where(want64[big] > 0, F32(np.inf), F32(-np.inf))), f"{what}: infinities differ"
        small = np.abs(want64) + s < THRESHOLD
        bad = small & ~np.isfinite(got)
        assert not bad.any(), f"{what}: {int(bad.sum())} non-finite words for a finite truth, first at point {np.flatnonzero(bad)[:1]}"


def _rule_slack(name, ops, k, unit):
    """CEILING * u of operand k, or NaN (no derived bound) where an intermediate the rule names overflows fp32 on its own"""
    u, inter = unit[k]
    with np.errstate(all="ignore"):
        s = AB.CEILING[name][k] * u
        for x in inter:
            s = np.where(np.abs(x) < 2.0 ** 127, s, np.nan)
        return s


def _holds_plain(got32, want64):
    """a plain ("R") cell: a finite, non-zero word of the truth's sign"""
    return bool(np.isfinite(got32) and got32 != 0 and np.sign(got32) == np.sign(want64))


def _as_fp32(x64, slack):
    """a factor of a product as fp32 holds it (overflowed to inf where fp32 overflows), and where that is certain: not within its
    error bound of the overflow threshold, not denormal"""
    with np.errstate(all="ignore"):
        m, s = np.abs(x64), _slack(x64, slack)
        sure = ((m + s < THRESHOLD) | (m - s >= THRESHOLD) | np.isnan(m)) & ~((m > 0) & (m < 2.0 ** -126))
        return x64.astype(F32).astype(np.float64), s, sure


def _check_product_class(got, x64, sx, y64, sy, what):
    """the class of the fp32 product of two fp32 factors known to sx and sy (inf * 0 is NaN in fp32 where the float64 product is not)"""
    (x, sx, ux), (y, sy, uy) = _as_fp32(x64, sx), _as_fp32(y64, sy)
    sure = ux & uy
    with np.errstate(all="ignore"):
        p = x * y
        sp = np.abs(x) * sy + np.abs(y) * sx + sx * sy + AB.ulp32(p)
        _check_class(got[sure], p[sure], what, sp[sure])


def _units_error(got, want64, unit, mask):
    with np.errstate(all="ignore"):
        err = np.abs(got[mask].astype(np.float64) - want64[mask]) / unit[mask]
    return (float(err.max()), int(np.flatnonzero(mask)[int(np.argmax(err))])) if err.size else (0.0, -1)


def _record(name, route, form, key, worst):
    REPORT.setdefault(name, {}).setdefault(route, {})[f"{form}.{key}"] = round(worst, 3)


def _check_gradient_route(name, route, form):
    r = _run(name, route, form)
    what = f"{name} via {route}/{form}"
    want = AB.rule(name, r.ops, r.g)
    unit = AB.units(name, r.ops)
    mask = AB.accuracy_mask(name, r.ops)
    n = len(r.ops[0])
    for k in range(len(r.ops)):
        got = r.got[k]
        _check_class(got, want[k], f"{what}, operand {k}", _rule_slack(name, r.ops, k, unit))
        if name in AB.EXACT:
            with np.errstate(all="ignore"):
                w32 = want[k].astype(F32)
            ok = _same_bits(got, w32) | ((w32 == 0) & (got == 0))
            assert ok.all(), f"{what}, operand {k}: {int((~ok).sum())} words differ from the exact rule, first at {np.flatnonzero(~ok)[:1]}"
            continue
        acc = mask[k] & (r.g == 1)
        worst, at = _units_error(got, want[k], unit[k][0], acc)
        _record(name, route, form, "abc"[k], worst)
        bound = min(BOUND[name][route], AB.CEILING[name][k])
        assert worst <= bound, (f"{what}, operand {k}: {worst:.3f} units at point {at} (operands {[float(o[at]) for o in r.ops]}), "
                                f"bound {bound}")
    # the planted cells: exact; a plain cell is finite, non-zero and of the truth's sign (and within the bound, above, where it is
    # accuracy-compared)
    for e, i in enumerate(range(r.n_draws, n)):
        toks = AB.expected_tokens(name, [o[i] for o in r.ops], r.rule_tok[e], r.grad_tok[e], float(r.g[i]))
        for k, tok in enumerate(toks):
            ok = _holds_plain(r.got[k][i], want[k][i]) if isinstance(tok, str) and tok == "R" else AB.token_holds(tok, r.got[k][i])
            assert ok, (f"{what}: edge cell {[float(o[i]) for o in r.raw]} operand {k}: got {r.got[k][i]!r}, the table gives {tok!r} "
                        f"(truth {want[k][i]!r}, output adjoint {r.g[i]})")


def _check_lm_route(name, form):
    r = _run(name, "lm", form)
    what = f"{name} via lm/{form}"
    loss_w, A_w, b_w = AB.normal_row(name, r.ops)
    d = AB.rule(name, r.ops)
    units = AB.units(name, r.ops)
    unit = [u for u, _ in units]
    slack = [_rule_slack(name, r.ops, k, units) for k in range(len(d))]
    mask = AB.accuracy_mask(name, r.ops)
    ceil = max(AB.CEILING[name])
    fwd = AB.FWD.get(name, 0.0)
    with np.errstate(all="ignore"):
        pred_slack = fwd * AB.ulp32(r.pred)
    used = []
    _check_product_class(r.loss, r.pred, pred_slack, r.pred, pred_slack, f"{what}, loss")
    for (i, j), want in A_w.items():
        w = AB.tri_index(i, j)
        used.append(w)
        got = r.normal[:, w]
        _check_product_class(got, d[i], slack[i], d[j], slack[j], f"{what}, A[{i}][{j}]")
        if name in AB.EXACT:
            with np.errstate(all="ignore"):
                w32 = want.astype(F32)
            ok = _same_bits(got, w32) | ((w32 == 0) & (got == 0))
            assert ok.all(), f"{what}, A[{i}][{j}]: {int((~ok).sum())} words differ from the exact rule"
            continue
        # d_i d_j with each factor within bound * u of its truth, then one rounding
        with np.errstate(all="ignore"):
            u = np.abs(d[i]) * unit[j] + np.abs(d[j]) * unit[i] + ceil * unit[i] * unit[j] + AB.ulp32(want)
            acc = mask[i] & mask[j] & AB._in_range(want) & np.isfinite(u)
        worst, at = _units_error(got, want, u, acc)
        _record(name, "lm", form, f"A{i}{j}", worst)
        assert worst <= BOUND[name]["lm"], f"{what}, A[{i}][{j}]: {worst:.3f} units at point {at}, bound {BOUND[name]['lm']}"
    for i, want in enumerate(b_w):
        used.append(len(LM.TRI) + i)
        _check_product_class(r.normal[:, used[-1]], d[i], slack[i], r.pred, pred_slack, f"{what}, b[{i}]")
    rest = np.ones(LM.WORDS, bool)
    rest[used] = False
    assert np.all(r.normal[:, rest].view(np.uint32) == 0), f"{what}: rows or columns of absent constants are not +0"
    # b is half the MSE gradient of the same trees at label 0 (the relation of test_gpu_sr_lm.py's _compare)
    value, type_, size, cpos = r.forest()
    _, grad = _gradient(value, type_, size, [0.0], use_mse=True)
    for i, want in enumerate(b_w):
        got, half = r.normal[:, len(LM.TRI) + i].astype(np.float64), grad[:, cpos[i]].astype(np.float64) / 2
        with np.errstate(all="ignore"):
            ok = np.isfinite(want) & np.isfinite(got) & np.isfinite(half) & (np.abs(want) < 2.0 ** 126)
            assert np.all(np.abs(got[ok] - half[ok]) <= 1e-3 * np.abs(want[ok]) + 1e-7), f"{what}: b[{i}] is not half the MSE gradient"
            # against the reference, in a unit of its own: d_i within its ceiling, the prediction within the forward bound, one rounding
            # (a-priori ceiling 1; the pinned bound is the measured maximum)
            u = np.abs(r.pred) * max(ceil, 0.5) * unit[i] + np.abs(d[i]) * fwd * AB.ulp32(r.pred) + AB.ulp32(want)
            acc = mask[i] & AB._in_range(want) & AB._in_range(r.pred) & np.isfinite(u)
        worst, at = _units_error(r.normal[:, len(LM.TRI) + i], want, u, acc)
        _record(name, "lm_b", form, f"b{i}", worst)
        assert worst <= BOUND[name]["lm_b"], (f"{what}: b[{i}] is {worst:.3f} of its unit from the reference at point {at}, "
                                              f"bound {BOUND[name]['lm_b']}")
    # the planted cells: the diagonal is the square of the table's value at g = 1
    for e, p in enumerate(range(r.n_draws, len(r.ops[0]))):
        for k, tok in enumerate(r.rule_tok[e]):
            got = r.normal[p, AB.tri_index(k, k)]
            if isinstance(tok, str) and tok == "R":     # a plain cell: positive, and finite and non-zero where the square stays in range
                sq = float(d[k][p]) ** 2
                ok = _holds_plain(got, 1.0) if 2.0 ** -126 <= sq < 2.0 ** 127 else bool(got >= 0)
            else:
                sq = {"Z": "Z", "N": "N", "G": "G", "MG": "G", "PI": "PI", "NI": "PI"}[tok] if isinstance(tok, str) else F32(tok) * F32(tok)
                ok = AB.token_holds(sq, got)
            assert ok, f"{what}: edge cell {[float(o[p]) for o in r.raw]} A[{k}][{k}]: got {got!r}, the table gives {tok!r} squared"


# ---- the tests --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", AB.NAMES)
def test_rule_on_route(name, route, form):
    if route == "lm":
        _check_lm_route(name, form)
    else:
        _check_gradient_route(name, route, form)


def _aligned(r1, r2):
    """-> (index into r1, index into r2, same operands?) over the points the two launches share: every draw and every planted cell
    both kept (a form that cannot hold a -0 leaves those cells out); operands that differ (a -0 turned +0) are marked"""
    nd = r1.n_draws
    e1, e2 = list(r1.edge_idx), list(r2.edge_idx)
    common = [e for e in e1 if e in e2]
    i1 = np.concatenate([np.arange(nd), nd + np.array([e1.index(e) for e in common], np.int64)])
    i2 = np.concatenate([np.arange(nd), nd + np.array([e2.index(e) for e in common], np.int64)])
    same = np.all([_same_bits(a[i1], b[i2]) for a, b in zip(r1.ops, r2.ops)], axis=0)
    return i1, i2, same


@pytest.mark.parametrize("name", AB.NAMES)
def test_cross_route_identities(name):
    runs = {(route, form): _run(name, route, form) for route in GRAD_ROUTES for form in FORMS}
    arity = AB.FUNCS[name][1]
    for form in FORMS:
        lds, glb, mo = runs["single_lds", form], runs["single_global", form], runs["multi", form]
        for k in range(arity):
            assert _same_bits(lds.got[k], glb.got[k]).all(), f"{name}/{form}, operand {k}: the LDS tape and the global tape differ"
        assert _same_bits(lds.loss, glb.loss).all()
        # r recomputed against r read from the tape: the draws and every planted cell both launches hold, same output adjoint
        i1, i2, same_ops = _aligned(lds, mo)
        same_ops &= _same_bits(lds.g[i1].astype(F32), mo.g[i2].astype(F32))
        assert same_ops[lds.n_draws:].sum() >= len(lds.edge_idx) - 1 and same_ops.mean() > 0.99
        for k in range(arity):
            same = _same_bits(lds.got[k][i1], mo.got[k][i2]) | ~same_ops
            REPORT.setdefault(name, {}).setdefault("multi_vs_single_bits_differ", {})[f"{form}.{'abc'[k]}"] = int((~same).sum())
            assert same.all(), f"{name}/{form}, operand {k}: {int((~same).sum())} words differ between r recomputed and r from the tape"
    for route in GRAD_ROUTES:
        di, st = runs[route, "direct"], runs[route, "stacked"]
        i1, i2, keep = _aligned(di, st)                       # (a -0 operand becomes +0 when stacked: not compared)
        keep &= _same_bits(di.g[i1].astype(F32), st.g[i2].astype(F32))
        assert keep.mean() > 0.99
        for k in range(arity):
            assert (_same_bits(di.got[k][i1], st.got[k][i2]) | ~keep).all(), f"{name} via {route}, operand {k}: stacked and direct differ"
    # a second launch
    first = runs["single_lds", "direct"]
    value, type_, size, cpos = first.forest()
    loss2, grad2 = _gradient(value, type_, size, [first.y])
    assert all(_same_bits(first.got[k], grad2[:, c]).all() for k, c in enumerate(cpos)) and _same_bits(first.loss, loss2).all()
    lm = _run(name, "lm", "direct")
    loss2, normal2 = _normal_eq(*lm.forest()[:3])
    assert _same_bits(lm.normal, normal2).all() and _same_bits(lm.loss, loss2).all()
    lm_st = _run(name, "lm", "stacked")
    i1, i2, keep = _aligned(lm, lm_st)
    assert (_same_bits(lm.normal[i1], lm_st.normal[i2]) | ~keep[:, None]).all(), f"{name} via lm: stacked and direct differ"


@pytest.mark.parametrize("route", ROUTES)
def test_if_on_the_smallest_denormal_takes_the_branch_its_loss_shows(route):
    """IF(2^-149, 2, 3): the float64 reference takes the first branch (the condition is > 0); the device's adjoints must go where its
    own forward pass went -- label -2 (0 on the Jacobian route), so the loss of the same launch is 4 against 5 (4 against 9)"""
    conds = np.array([AB.DEN, -AB.DEN, 0.0, 1.0], F32)
    ops = [conds, np.full(4, 2, F32), np.full(4, 3, F32)]
    gp_len, multi = GRAD_ROUTES.get(route, (64, False))
    for form in FORMS:
        value, type_, size, cpos = AB.probe_forest("IF", ops, form, gp_len, multi)
        if route == "lm":
            loss, normal = _normal_eq(value, type_, size)
            took_b = loss == 4.0
            assert np.all(took_b | (loss == 9.0))
            d = [normal[:, AB.tri_index(k, k)] for k in range(3)]
        else:
            loss, grad = _gradient(value, type_, size, [-2.0, 0.0] if multi else [-2.0])
            took_b = loss == 4.0
            assert np.all(took_b | (loss == 5.0))
            d = [grad[:, c] for c in cpos]
        assert np.array_equal(took_b, [True, False, False, True]), f"IF via {route}/{form}: the forward pass disagrees with the reference"
        assert np.all(d[0] == 0) and np.array_equal(d[1], took_b.astype(F32)) and np.array_equal(d[2], (~took_b).astype(F32))


def test_write_adjoint_report():
    """not a check: leaves the measured maxima in the directory EVOGP_REPORT_DIR names"""
    out = os.environ.get("EVOGP_REPORT_DIR", "")
    if out and os.path.isdir(out) and REPORT:
        table = {n: {r: max([v for key, v in REPORT[n].get(r, {}).items()], default=0.0) for r in ROUTES + ["lm_b"]} for n in REPORT}
        json.dump({"worst_per_route": table, "ceiling": {n: list(AB.CEILING[n]) for n in AB.NAMES}, "detail": REPORT},
                  open(os.path.join(out, "sr_adjoint_report.json"), "w"), indent=1, sort_keys=True)
