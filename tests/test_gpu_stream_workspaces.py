"""GPU: the per-stream workspace pool (csrc/launch.hpp StreamWorkspaces) through the ops that use it: the global tapes of the tape
kernels (rows longer than 64 nodes; one block per stream, shared by the gradient, subtree and normal-equation passes) and the
prediction buffer of the per-case errors.  A larger request grows the block and retires the old one, evogp_hip_release_workspaces
frees both, and the results do not depend on which block they were computed in.  No stream capture is involved."""
import os
import sys

import numpy as np
import pytest
import torch

import evogp_amd  # noqa: F401  (registers the ops)
from evogp_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from grad_trees import ALL_FUNCS, random_forest  # noqa: E402

pytestmark = pytest.mark.gpu

VAR_LEN = 3
HIP = torch.ops.evogp_hip


def _dev(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _same(a, b):
    """bit equality of two results (a tensor or a tuple of tensors)"""
    a, b = (a if isinstance(a, (tuple, list)) else (a,)), (b if isinstance(b, (tuple, list)) else (b,))
    return len(a) == len(b) and all(torch.equal(x.view(torch.int32), z.view(torch.int32)) for x, z in zip(a, b))


def _release():
    assert _lib.lib.evogp_hip_release_workspaces() == 0


def test_tape_block_grows_is_released_and_is_shared(rng):
    L, D = 128, 100
    value, type_, size = random_forest(rng, 600, L, ALL_FUNCS, VAR_LEN, 1, max_depth=5)
    Xd, yd = _dev(rng.uniform(0.5, 1.5, (D, VAR_LEN)).astype(np.float32), rng.uniform(-1, 1, (D, 1)).astype(np.float32))
    big = _dev(value, type_, size)
    small = [a[:8].contiguous() for a in big]

    def grad(f):
        return HIP.tree_SR_gradient(f[0].shape[0], D, L, VAR_LEN, 1, True, *f, Xd, yd)

    def sub(f):
        return HIP.tree_SR_subtree_errors(f[0].shape[0], D, L, VAR_LEN, 1, True, *f, Xd, yd)

    def neq(f):
        return HIP.tree_SR_normal_eq(f[0].shape[0], D, L, VAR_LEN, 1, *f, Xd, yd)

    _release()
    # 8 trees, then 600: the second call needs more resident tapes, so the block grows and the old one is retired; the subtree and the
    # normal-equation pass follow on the same stream in the block the gradient left
    first = [grad(small), grad(big), sub(big), neq(big)]
    assert torch.isfinite(first[1][0]).any()
    _release()
    again = [grad(small), grad(big)]
    assert _same(first[0], again[0]) and _same(first[1], again[1])
    _release()
    assert _same(first[2], sub(big))     # each from a fresh state of its own
    _release()
    assert _same(first[3], neq(big))
    _release()
    assert _same(first[1], grad(big))    # (and the large block first, without a retired one)
    _release()


def test_case_error_block_grows_and_is_released(rng):
    L = 32
    value, type_, size = random_forest(rng, 600, L, ALL_FUNCS, VAR_LEN, 1, max_depth=4)
    big = _dev(value, type_, size)
    small = [a[:8].contiguous() for a in big]
    X = rng.uniform(0.5, 1.5, (256, VAR_LEN)).astype(np.float32)
    y = rng.uniform(-1, 1, (256, 1)).astype(np.float32)
    Xb, yb = _dev(X, y)
    Xs, ys = _dev(X[:64], y[:64])

    def both():
        return [HIP.tree_SR_case_errors(8, 64, L, VAR_LEN, 1, True, *small, Xs, ys),
                HIP.tree_SR_case_errors(600, 256, L, VAR_LEN, 1, True, *big, Xb, yb)]

    _release()
    first = both()
    assert first[0].shape == (64, 8) and first[1].shape == (256, 600) and torch.isfinite(first[1]).any()
    _release()
    again = both()
    assert _same(first[0], again[0]) and _same(first[1], again[1])
    _release()
