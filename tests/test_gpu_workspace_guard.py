"""GPU: the caller-provided workspaces of evogp_hip_tree_classes, evogp_hip_lexicase_select and evogp_hip_pareto_rank, through the C ABI
(as tests/gpu_capi.py).  Each call gets exactly the bytes its *_workspace_bytes function asks for, in the middle of a larger buffer
filled with one byte value: the 4096 bytes in front of the workspace and the 4096 bytes behind it must come back untouched, the
outputs must equal the torch op's on the same inputs bit for bit, and they must not depend on what the workspace held on entry
(fill 0x00 against fill 0xFF)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import evogp_amd  # noqa: F401  (registers the ops)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dedup_cases import half_copies, planted_forest  # noqa: E402
from gpu_capi import DEV, L, _stream, dev  # noqa: E402
from test_nsga2_ref import population  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 4096
FILLS = (0x00, 0xFF)


def _bytes(fn, *args):
    n = ctypes.c_ulonglong(0)
    rc = fn(*args, ctypes.byref(n))
    assert rc == 0, L.evogp_hip_error_string(rc)
    return int(n.value)


def _guarded(nbytes, fill, call):
    """run call(workspace pointer) on nbytes of workspace between two guard zones of a buffer filled with ``fill``"""
    buf = torch.full((nbytes + 2 * GUARD,), fill, dtype=torch.uint8, device=DEV)
    rc = call(buf.data_ptr() + GUARD)
    assert rc == 0, L.evogp_hip_error_string(rc)
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == fill).all()), f"fill {fill:#04x}: bytes in front of the workspace were written"
    assert bool((buf[GUARD + nbytes:] == fill).all()), f"fill {fill:#04x}: bytes behind the workspace were written"


def _same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), what


@pytest.mark.parametrize("pop", [1, 63, 200, 5000])
def test_tree_classes(rng, pop):
    gp_len = 64
    forests = [planted_forest(rng, pop, gp_len)] + ([half_copies(rng, pop, gp_len)] if pop >= 63 else [])
    nbytes = _bytes(L.evogp_hip_tree_classes_workspace_bytes, pop)
    for value, type_, size in forests:
        v, t, s = dev(value, np.float32), dev(type_, np.int16), dev(size, np.int16)
        h = torch.ops.evogp_hip.tree_hash(v, t, s)
        want = torch.ops.evogp_hip.tree_classes(v, t, s, h)
        if pop >= 63:
            assert int((want != torch.arange(pop, dtype=torch.int32, device=DEV)).sum()) >= 4   # (the forest holds clones)
        runs = []
        for fill in FILLS:
            got = torch.full((pop,), -7, dtype=torch.int32, device=DEV)
            _guarded(nbytes, fill, lambda ws: L.evogp_hip_tree_classes(pop, gp_len, v.data_ptr(), t.data_ptr(), s.data_ptr(), h.data_ptr(),
                                                                       got.data_ptr(), ws, _stream()))
            _same_bits(got, want, f"class ids, fill {fill:#04x}")
            runs.append(got)
        _same_bits(runs[0], runs[1], "class ids under the two fills")


def _lex_errors(rng, n, pop, quantised):
    E = rng.integers(0, 4, (n, pop)).astype(np.float32) * 0.25 if quantised else rng.exponential(1.0, (n, pop)).astype(np.float32)
    E[rng.random((n, pop)) < 0.03] = np.nan
    E[rng.random((n, pop)) < 0.02] = -0.0
    return E


@pytest.mark.parametrize("pop,n", [(1, 1), (7, 3), (4099, 64)])
def test_lexicase_select(rng, pop, n):
    n_events = pop
    nbytes = _bytes(L.evogp_hip_lexicase_workspace_bytes, n, pop, n_events)
    # quantised errors: few clone classes, pools that fit a wave's LDS list; continuous ones with a wide epsilon: pools of thousands
    # of classes (the bit masks in the workspace)
    for quantised, width in ((True, 0.25), (False, 8.0)):
        E = dev(_lex_errors(rng, n, pop, quantised), np.float32)
        eps = dev(rng.choice([0.0, width], n), np.float32)
        want = torch.ops.evogp_hip.lexicase_select(E, eps, n_events, 77, 3)
        runs = []
        for fill in FILLS:
            got = torch.full((n_events,), -7, dtype=torch.int32, device=DEV)
            _guarded(nbytes, fill, lambda ws: L.evogp_hip_lexicase_select(n, pop, E.data_ptr(), eps.data_ptr(), n_events, 77, 3, got.data_ptr(),
                                                                          ws, _stream()))
            _same_bits(got, want, f"winners, quantised {quantised}, fill {fill:#04x}")
            runs.append(got)
        _same_bits(runs[0], runs[1], "winners under the two fills")


@pytest.mark.parametrize("pop", [1, 7, 4099])
def test_pareto_rank(rng, pop):
    cx_bound = 64
    nbytes = _bytes(L.evogp_hip_pareto_rank_workspace_bytes, pop)
    for kind in ("quantised", "continuous"):   # quantised: runs of equal keys
        err_h, cx_h = population(rng, pop, kind, cx_bound)
        err, cx = dev(err_h, np.float32), dev(cx_h, np.int32)
        want = torch.ops.evogp_hip.pareto_rank(err, cx, cx_bound)
        runs = []
        for fill in FILLS:
            front = torch.full((pop,), -7, dtype=torch.int32, device=DEV)
            crowding = torch.full((pop,), float("nan"), dtype=torch.float32, device=DEV)
            order = torch.full((pop,), -7, dtype=torch.int32, device=DEV)
            _guarded(nbytes, fill, lambda ws: L.evogp_hip_pareto_rank(pop, cx_bound, err.data_ptr(), cx.data_ptr(), front.data_ptr(),
                                                                      crowding.data_ptr(), order.data_ptr(), ws, _stream()))
            for name, g, w in zip(("front", "crowding", "order"), (front, crowding, order), want):
                _same_bits(g, w, f"{name}, {kind}, fill {fill:#04x}")
            runs.append((front, crowding, order))
        for name, a, b in zip(("front", "crowding", "order"), *runs):
            _same_bits(a, b, f"{name} under the two fills")
