"""GPU: every route that evaluates a whole tree, through the C ABI, against the exact value of the tree as the REFERENCE's sympy export
states it (tests/golden/sympy_truth_*.npz: mpmath at 50 digits; tests/golden/make_sympy_truth.py) -- not against the oracle, which is our own
restatement of the reference's device code.  Operand order of - / pow, the branch an `if` takes, the operand an OUT node forwards and what
the program compilers' folds and reorderings do to a value are held here to something that is not ours.

Every compared entry is within 1e-5 |T| + 2 B of the truth T, B the running float32 error bound of tests/exact_eval_ref.py (from the
reference side only); a fitness within mean(2 |y - T| tol + tol^2) + D 2^-24 truth.  No allowed-bad fraction; the conditions that keep the
comparison from being empty are asserted by tests/test_sympy_truth.py on the same fixtures.  The worst |got - T| / tol per route and group
goes to sympy_truth_report.json in the directory EVOGP_REPORT_DIR names, when it names one, as tests/test_gpu_sr_adjoint.py writes its
report (profiles/sympy_truth_report.json is a copy of such a report)."""
import json
import os

import numpy as np
import pytest

import exact_eval_ref as ex

pytestmark = pytest.mark.gpu
REPORT = {}
ARITH_MASK = 0b11110   # + - * /
DS = (8, 100, 600)     # the 1-, 4- and 8-row interpreter builds


@pytest.fixture(scope="module")
def g():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import gpu_capi

    return gpu_capi


@pytest.fixture(scope="module", params=ex.GROUPS)
def grp(request):
    return ex.group(request.param)


def test_evaluate_and_batch_evaluate_meet_the_truth(g, grp):
    t = grp
    for D in DS:
        X, idx = t.rows(D)
        ex.assert_entries(g.batch_evaluate(*t.forest, X, t.out_len), t, idx, f"{t.name} batch_evaluate D={D}", REPORT)
    for D in DS:
        X, idx = t.rows(D)
        forest, rows = ex.copies(t, idx)   # one row per tree copy
        ex.assert_entries(g.evaluate(*forest, rows, t.out_len), t, idx, f"{t.name} evaluate D={D}", REPORT)


def fitness_both(g, t, what, **kw):
    for D in DS:
        X, idx = t.rows(D)
        y = t.labels(idx)
        for mse in (True, False):
            got = g.sr_fitness(*t.forest, X, y, mse, **kw)
            ex.assert_fitness(got, t, idx, mse, f"{t.name} sr_fitness {what} D={D} {'mse' if mse else 'mae'}", REPORT)


def test_sr_fitness_meets_the_truth(g, grp):
    fitness_both(g, grp, "default")


@pytest.mark.parametrize("name", ["arith", "long"])
def test_sr_fitness_through_every_program_compiler_meets_the_truth(g, name):
    """the routes tests/test_gpu_tc_wide.py::test_every_program_compiler_gives_the_same_fitness_words compares with each other: the one-tree
    compiler and the packed one at every batch size, the handlers' twins always / never, long trees through the general compiler's staged
    passes, a forest that carries its function mask (the arithmetic-only instantiation).  The kernel_type codes of the reference's signature
    are accepted and choose nothing here (one route): they are called so that a code that began to choose something would be held as well"""
    t = ex.group(name)
    lib = g.L
    try:
        for batch in (0, 8, 16, 32, 64):
            assert lib.evogp_hip_debug_compile_batch(batch) == 0
            fitness_both(g, t, f"compile_batch {batch}")
        assert lib.evogp_hip_debug_compile_batch(-1) == 0
        for twins in (1, 0):
            assert lib.evogp_hip_debug_twins(twins) == 0
            for batch in (0, 16, -1):
                assert lib.evogp_hip_debug_compile_batch(batch) == 0
                fitness_both(g, t, f"twins {twins} compile_batch {batch}")
        assert lib.evogp_hip_debug_twins(-1) == 0 and lib.evogp_hip_debug_compile_batch(-1) == 0
        if name == "long":
            assert lib.evogp_hip_debug_long_compiler(0) == 0
            fitness_both(g, t, "long trees through compile_general")
            assert lib.evogp_hip_debug_long_compiler(-1) == 0
    finally:
        lib.evogp_hip_debug_compile_batch(-1)
        lib.evogp_hip_debug_long_compiler(-1)
        lib.evogp_hip_debug_twins(-1)
    fitness_both(g, t, "function mask", func_mask=ARITH_MASK)
    for kt in (1, 2, 3, 4):
        fitness_both(g, t, f"kernel_type {kt}", kernel_type=kt)


def test_evaluate_prepared_meets_the_truth(g):
    """the rollout path: OUT-node records prepared once, evaluated step by step.  evogp_hip_evaluate_prepare takes forests of two and more
    outputs only (a single-output policy goes through evogp_hip_evaluate, held to the truth above), so `mo3` is the group it can see"""
    t = ex.group("mo3")
    X, idx = t.rows(100)
    forest, rows = ex.copies(t, idx)
    got, _ = g.evaluate_prepared(*forest, rows, t.out_len, steps=2)
    ex.assert_entries(got, t, idx, f"{t.name} evaluate_prepared", REPORT)


def test_write_sympy_truth_report():
    out = os.environ.get("EVOGP_REPORT_DIR", "")
    if out and os.path.isdir(out) and REPORT:
        json.dump(REPORT, open(os.path.join(out, "sympy_truth_report.json"), "w"), indent=1, sort_keys=True)
    assert all(r <= 1.0 for r in REPORT.values())
