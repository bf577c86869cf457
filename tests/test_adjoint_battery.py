"""CPU: the adjoint battery (tests/adjoint_battery.py) against the references, without a GPU: its probe trees read the rule they claim
(forest_grad on a subsample, both forms, both output modes), its hand-written edge expectations are the reference's, its operand draws
keep 90 % of their points inside the accuracy comparison, its normal-equation rows are sr_lm_ref's, and its expectations tell the
table from seven single-edit mutants of it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adjoint_battery as AB  # noqa: E402
import sr_grad_ref as R  # noqa: E402
import sr_lm_ref as LM  # noqa: E402

F32 = np.float32
SUB = 200   # drawn points per function and form tied to forest_grad, plus every edge cell


def _subsample(name, form, multi):
    ops, nd, rt, gt, _ = AB.points(name, form, multi)
    pick = np.concatenate([(np.arange(SUB) * 7919) % nd, np.arange(nd - len(AB.SPECIAL), nd), np.arange(nd, len(ops[0]))])
    return [o[pick] for o in ops]


def _same(got, want, rel=1e-12):
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    inf = ok & np.isinf(want)
    assert np.array_equal(got[inf], want[inf])
    fin = ok & ~inf
    assert np.all(np.abs(got[fin] - want[fin]) <= rel * np.abs(want[fin]))


@pytest.mark.parametrize("multi", [False, True])
@pytest.mark.parametrize("form", ["direct", "stacked"])
@pytest.mark.parametrize("name", AB.NAMES)
def test_probe_trees_read_the_rule_off_forest_grad(name, form, multi):
    ops = _subsample(name, form, multi)
    value, type_, size, cpos = AB.probe_forest(name, ops, form, 16, multi)
    eff = AB.effective_operands(ops, form, multi)
    pred = AB.forward(name, eff)
    y32 = AB.launch_label(pred)
    g = AB.out_adjoint(pred, y32)
    with np.errstate(all="ignore"):
        fin = np.isfinite(pred.astype(F32))
    assert np.all(g[fin & (pred > -1e38)] == 1.0)          # the label makes the output adjoint exactly 1 wherever it can
    want = AB.rule(name, eff, g)
    y = np.array([[y32, 0.0]] if multi else [[y32]], F32)
    with np.errstate(all="ignore"):
        loss, grad, _ = R.forest_grad(value, type_, size, np.zeros((1, 1), F32), y, use_mse=False)
        _same(loss, np.abs(pred - float(y32)))
    for k, c in enumerate(cpos):
        _same(grad[:, c], want[k])
    rest = np.ones(grad.shape[1], bool)
    rest[cpos] = False
    assert np.all(grad[:, rest] == 0)


@pytest.mark.parametrize("name", AB.NAMES)
def test_edge_expectations_are_the_reference(name):
    ops, rule_tok, grad_tok = AB.edge_points(name)
    assert len(rule_tok) >= 1
    pred = AB.forward(name, ops)
    with np.errstate(all="ignore"):
        p32 = pred.astype(F32)
    g = np.where(np.isfinite(p32), 1.0, np.sign(p32.astype(np.float64)))
    at_one, at_g = AB.rule(name, ops, 1.0), AB.rule(name, ops, g)
    for i in range(len(rule_tok)):
        assert grad_tok[i] is None or g[i] != 1, (name, i, "a gradient expectation of its own needs a non-finite prediction")
        for toks, vals in ((rule_tok[i], at_one), (AB.expected_tokens(name, [o[i] for o in ops], rule_tok[i], grad_tok[i], g[i]), at_g)):
            assert len(toks) == len(ops)
            for k, tok in enumerate(toks):
                with np.errstate(all="ignore"):
                    v64 = float(vals[k][i])
                    v32 = F32(v64)
                if isinstance(tok, str) and tok != "R":
                    assert AB.token_holds(tok, v32), (name, i, k, tok, v64)
                elif isinstance(tok, str):
                    assert np.isfinite(v32) and v32 != 0, (name, i, k, v64)
                else:   # an exact fp32 value: the chain of fp32 roundings may sit one ulp from the rounded float64 value
                    assert abs(float(tok) - v64) <= float(np.spacing(np.abs(v32))), (name, i, k, tok, v64)


@pytest.mark.parametrize("name", [n for n in AB.NAMES if n not in AB.EXACT])
def test_ninety_percent_of_the_draws_are_accuracy_compared(name):
    ops = AB.draws(name)
    assert len(ops[0]) == AB.N_DRAWS
    for k, m in enumerate(AB.accuracy_mask(name, ops)):
        assert m.mean() >= 0.9, (name, k, float(m.mean()))
    for u, _ in AB.units(name, ops):
        assert np.all(u[np.isfinite(u)] >= 0)


@pytest.mark.parametrize("form", ["direct", "stacked"])
@pytest.mark.parametrize("name", AB.NAMES)
def test_normal_rows_are_sr_lm_ref(name, form):
    """the rows the device's Jacobian walk is compared with: A_ij = d_i d_j, b_i = d_i pred, loss = pred^2 (D = 1, label 0), every
    other word of the row +0 -- on the subsample and on every edge cell"""
    ops = _subsample(name, form, False)
    value, type_, size, cpos = AB.probe_forest(name, ops, form, 16, False)
    eff = AB.effective_operands(ops, form, False)
    loss_w, A_w, b_w = AB.normal_row(name, eff)
    with np.errstate(all="ignore"):
        loss, normal, _ = LM.forest_normal_eq(value, type_, size, np.zeros((1, 1), F32), np.zeros((1, 1), F32))
    _same(loss, loss_w)
    used = []
    for (i, j), want in A_w.items():
        used.append(AB.tri_index(i, j))
        _same(normal[:, used[-1]], want)
    for i, want in enumerate(b_w):
        used.append(len(LM.TRI) + i)
        _same(normal[:, used[-1]], want)
    rest = np.ones(LM.WORDS, bool)
    rest[used] = False
    assert np.all(normal[:, rest] == 0)
    for t in range(len(ops[0])):
        assert list(LM.optimised_consts(type_[t], size[t])[:len(cpos)]) == cpos


# ---- the expectations tell the table from single-edit mutants of it -----------------------------------------------------------------
def _mut_sub(f, a, b, r, g):
    return (-g, g) if f == R.F_SUB else None


def _mut_max(f, a, b, r, g):
    if f == R.F_MAX:
        c = a > b
        return np.where(c, g, 0.0), np.where(c, 0.0, g)


def _mut_pow(f, a, b, r, g):
    if f == R.F_POW:
        return g * b * np.power(a, b - 1), np.where(a >= 0, g * r * np.log(a), 0.0)


def _mut_loose_inv(f, a, r, g):
    return np.where(np.abs(a) < R.DELTA, 0.0, -g * r * r) if f == R.F_LOOSE_INV else None


def _mut_loose_sqrt(f, a, r, g):
    return np.where(a == 0, 0.0, g * 0.5 / r) if f == R.F_LOOSE_SQRT else None


def _mut_default(f, a, r, g):
    return g + np.zeros_like(a) if f is None else None


def _mut_sqrt(f, a, r, g):
    return g * 0.25 / r if f == R.F_SQRT else None


MUTANTS = [("SUB", 2, _mut_sub), ("MAX", 2, _mut_max), ("POW", 2, _mut_pow), ("LOOSE_INV", 1, _mut_loose_inv),
           ("LOOSE_SQRT", 1, _mut_loose_sqrt), ("UNKNOWN_U", 1, _mut_default), ("SQRT", 1, _mut_sqrt)]


@pytest.mark.parametrize("name,arity,mutant", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_edge_expectations_reject_the_mutant(monkeypatch, name, arity, mutant):
    """each single edit of the table (restated here in float64) breaks at least one EXACT edge expectation of the battery: a token
    other than "R" that the mutant's fp32 value does not meet"""
    target = "unary_adjoint" if arity == 1 else "binary_adjoint"
    original = getattr(R, target)

    def patched(f, *args):
        with np.errstate(all="ignore"):
            out = mutant(f, *args)
        return original(f, *args) if out is None else out

    monkeypatch.setattr(R, target, patched)
    ops, rule_tok, _ = AB.edge_points(name)
    vals = AB.rule(name, ops, 1.0)
    broken = 0
    for i, toks in enumerate(rule_tok):
        for k, tok in enumerate(toks):
            with np.errstate(all="ignore"):
                v32 = F32(float(vals[k][i]))
            if not (isinstance(tok, str) and tok == "R") and not AB.token_holds(tok, v32):
                broken += 1
    assert broken >= 1
