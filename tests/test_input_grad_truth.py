"""CPU: the float64 restatement of the input gradients (tests/input_grad_ref.py) against a derivative truth that does not descend from the
adjoint table -- tests/golden/input_grad_truth_<group>.npz: the reference's sympy export of every fixture tree, differentiated numerically
by mpmath at 50 digits (tests/golden/make_input_grad_truth.py), first 32 rows of the five single-output groups of sympy_truth_*.npz.

An entry (tree, row, variable) is compared when it has a truth (d_ok) and passes the exclusion rule (input_grad_ref.comparable: finite,
and two draws of a 3-ulp jitter of every function result and adjoint move the derivative by at most 1e-4 scale + 1e-9) -- and the export
states the function the device computes there: the entry's VALUE is `regular` in tests/exact_eval_ref.py.  The last leaves out what
tests/test_sympy_truth.py leaves out of the value comparison for the same reason, e.g. a loose division by a literal 0, which the export
folds to the constant 1e9 (derivative 0) and the device computes as a * 1e9 (2 trees, 96 entries; without it the comparison holds the
restatement to another function).  The bound is
1e-9 scale + 1e-12.  Derivation: the rule admits entries whose derivative moves by at most 1e-4 scale under relative perturbations of
~2^-22 of every intermediate, a condition number of a few hundred; times at most 2 * 1024 float64 roundings of 2^-53 that is ~1e-10 scale,
and the bound leaves a decade of margin.  The share of entries the rule keeps, over all 100 rows, must reach the floors below: they are
conditions of the tests, not measurements (measured: arith 0.946, paper7 0.998, wide_pos 0.926, wide_signed 0.871, long 0.980).

The worst |restatement - truth| / bound per group goes to input_grad_truth_report.json in the directory EVOGP_REPORT_DIR names, when it
names one (profiles/input_grad_truth_report.json is such a report, with the GPU's ratios of tests/test_gpu_input_grad.py merged in)."""
import functools
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_eval_ref as ex  # noqa: E402
import input_grad_ref as XR  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GROUPS = ("arith", "paper7", "wide_pos", "wide_signed", "long")
FLOORS = {"arith": 0.90, "paper7": 0.90, "wide_pos": 0.90, "wide_signed": 0.80, "long": 0.90}
WRT = [0, 1, 2]
TRUTH_ROWS = 32
REPORT = {}


class Fixture:
    """one group: the forest and X of sympy_truth_<group>.npz, the derivative truth of its first 32 rows, and -- computed once, shared by
    the CPU and the GPU tests, never written to -- the float64 restatement on all 100 rows and the entries the exclusion rule keeps"""

    def __init__(self, name):
        z = np.load(os.path.join(GOLD, f"sympy_truth_{name}.npz"))
        t = np.load(os.path.join(GOLD, f"input_grad_truth_{name}.npz"))
        self.name = name
        self.forest = (z["value"], z["type"], z["size"])
        self.X = z["X"]
        self.header = json.loads(bytes(t["header"]).decode())
        self.dT = t["dT"].transpose(2, 0, 1)        # (V, trees, 32)
        self.d_ok = t["d_ok"].transpose(2, 0, 1)
        assert self.dT.shape == (3, self.forest[0].shape[0], TRUTH_ROWS) and self.header["rows"] == TRUTH_ROWS
        base = XR.forest_xgrad(*self.forest, self.X.astype(np.float64), WRT)
        self.pred, self.d, self.scale = base
        self.rule = XR.comparable(*self.forest, self.X.astype(np.float64), WRT, base=base)   # (V, trees, 100)
        # the entries held to the truth: a truth, the rule, and a value on which the export and the device state the same function
        self.truth_mask = self.rule[:, :, :TRUTH_ROWS] & self.d_ok & ex.group(name).regular[None, :, :TRUTH_ROWS, 0]
        for a in (self.pred, self.d, self.scale, self.rule, self.dT, self.d_ok, self.truth_mask):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def fixture(name):
    return Fixture(name)


def write_report(report):
    out = os.environ.get("EVOGP_REPORT_DIR", "")
    if out and os.path.isdir(out) and report:
        path = os.path.join(out, "input_grad_truth_report.json")
        merged = json.load(open(path)) if os.path.exists(path) else {}
        merged.update(report)
        json.dump(merged, open(path, "w"), indent=1, sort_keys=True)


def worst_ratio(got, want, tol, mask):
    with np.errstate(all="ignore"):
        err = np.abs(np.asarray(got, np.float64) - want)
        ratio = np.where(mask, np.where(err <= 0, 0.0, err / tol), 0.0)
    ratio = np.where(mask & ~np.isfinite(ratio), np.inf, ratio)   # a NaN or infinite result on a compared entry
    return float(ratio.max()), ratio


@pytest.mark.parametrize("name", GROUPS)
def test_the_rule_keeps_its_floor_of_the_entries(name):
    f = fixture(name)
    share = float(f.rule.mean())
    REPORT[f"{name} share compared (100 rows)"] = share
    assert share >= FLOORS[name], f"{name}: the exclusion rule keeps {share:.3f} of the entries, the floor is {FLOORS[name]}"
    truth_share = float(f.truth_mask.mean())
    REPORT[f"{name} share compared against the truth (32 rows)"] = truth_share
    assert truth_share >= FLOORS[name] - 0.05, (name, truth_share)


@pytest.mark.parametrize("name", GROUPS)
def test_restatement_meets_the_truth(name):
    f = fixture(name)
    mask = f.truth_mask
    d, scale = f.d[:, :, :TRUTH_ROWS], f.scale[:, :, :TRUTH_ROWS]
    worst, ratio = worst_ratio(d, f.dT, 1e-9 * scale + 1e-12, mask)
    REPORT[f"{name} float64 restatement against the truth, worst |d - truth| / (1e-9 scale + 1e-12)"] = worst
    if not worst <= 1.0:
        k, t, r = np.unravel_index(np.argmax(ratio), ratio.shape)
        raise AssertionError(f"{name}: variable {k} tree {t} row {r}: restatement {d[k, t, r]!r}, truth {f.dT[k, t, r]!r}, scale {scale[k, t, r]:.3g}; "
                             f"{int((ratio > 1).sum())} of {int(mask.sum())} compared entries beyond the bound")
    assert (f.dT[mask] != 0).mean() > 0.25   # the comparison is not one of zeros (a tree holds two of the three variables on average)


def test_write_report():
    write_report(REPORT)
