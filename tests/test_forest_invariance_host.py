"""CPU: the forest invariants (tests/forest_invariance.py: dead words, row order, slices) on every op that has a CPU stand-in
(tests/cpu_*_ops.py), which keeps the harness and the numpy / C restatements honest without a GPU; three toy ops that prove the checker
can fail, each under the invariant it violates; and the table's coverage of the ops evogp_amd defines."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

import evogp_amd  # noqa: F401  (defines the schemas)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forest_invariance as FI  # noqa: E402

POP, D = 40, 50   # the per-tree numpy loops of the restatements stay within seconds per op
HOST = sorted(op for op, row in FI.TABLE.items() if row["cpu"])


def _case(name):
    return FI.build_case(name, min(POP, FI.CASES[name]["pop"]), D)


@pytest.mark.parametrize("op,case", [(op, c) for op in HOST for c in FI.cases_for(op)])
def test_cpu_stand_in_keeps_the_invariants(op, case):
    row = FI.TABLE[op]
    for module in row["cpu"]:
        importlib.import_module(module).register()
    FI.check(op, row, _case(case), "cpu")


def _toy(fn):
    return FI._row(lambda f, s, p, device: (np.asarray(fn(*f), np.float32),), out="any", data=False)


@pytest.mark.parametrize("name,fn,invariant,passes", [
    ("sum over all L words", lambda v, t, s: v.sum(1), "A (dead words)", "BC"),
    ("value[:, 0] + arange(pop)", lambda v, t, s: v[:, 0] + np.arange(len(v)), "B (row order)", "A"),
    ("value[:, 0] * pop", lambda v, t, s: v[:, 0] * len(v), "C (slices)", "AB"),
])
def test_the_checker_fails_on_a_toy_op(name, fn, invariant, passes):
    case, row = _case("arith_L64"), _toy(fn)
    with pytest.raises(AssertionError) as e:
        FI.check("toy::" + name, row, case, "cpu")
    assert f"invariant {invariant}" in str(e.value), str(e.value)
    assert "tree " in str(e.value)
    FI.check("toy::" + name, row, case, "cpu", invariants=passes)   # ... and under no other invariant


def test_a_well_behaved_toy_op_passes():
    live = lambda v, t, s: np.where(np.arange(v.shape[1])[None, :] < FI.live_len(s)[:, None], v, 0).sum(1)  # noqa: E731
    FI.check("toy::sum over the live words", _toy(live), _case("arith_L64"), "cpu")


def test_the_transforms_meet_the_issue():
    for name in FI.CASES:
        c = _case(name)
        n, L = FI.live_len(c.forest[2]), c.L
        raw = c.forest[2][:, 0]
        assert (n == 1).any() and (raw == L).any() and (raw == 0).any() and (raw < 0).any() and (raw > L).any(), name
        if L > 64:
            assert {63, 64, 65} <= set(n.tolist()) and (n > 65).any(), name
        assert set(c.planted) == set(FI._patterns(L, c.out_len)), name
        sv, st, ss = c.stale
        dead = FI.dead_mask(c.forest[2])
        assert np.isin(st[dead] & 0x7F, [0, 1, 2, 3, 4]).all(), name                       # type codes of the alphabet
        fn = dead & np.isin(st & 0x7F, [2, 3, 4])
        flagged = fn & ((st & 0x80) != 0)
        assert (sv[fn & ~flagged] < 29).all() and (sv[fn & ~flagged] >= 0).all(), name       # function ids
        assert ((sv[flagged].view(np.uint32) & 0xFFFF) < 29).all() and ((sv[flagged].view(np.uint32) >> 16) < c.out_len).all(), name
        var = dead & ((st & 0x7F) == 0)
        assert (sv[var] >= 0).all() and (sv[var] < c.var_len).all(), name                    # variable indices
        t = c.planted["nan_const"]
        assert np.isnan(sv[t, n[t]]) and st[t, n[t]] == 1, name
    assert FI.slices(257) == [(0, 1), (256, 257), (61, 131), (0, 256)]
    assert all(sorted(p.tolist()) == list(range(9)) for p in FI.permute(np.random.default_rng(0), 9))


def test_the_table_and_the_exemptions_cover_every_op():
    have = {n.split(".")[0] for n in torch._C._dispatch_get_all_op_names() if n.startswith(("evogp_cuda::", "evogp_hip::"))}
    listed = set(FI.TABLE) | set(FI.EXEMPT)
    assert not set(FI.TABLE) & set(FI.EXEMPT)
    assert have == listed, (sorted(have - listed), sorted(listed - have))
    assert all(FI.cases_for(op) for op in FI.TABLE)
