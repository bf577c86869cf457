"""GPU: the three tape passes (csrc/sr_grad.hip, csrc/sr_subtree.hip, csrc/sr_lm.hip) choose their waves per workgroup and their
workgroups by ONE plan (csrc/sr_forward.hpp plan_tape_launch), so the same rows are summed in the same order and the three losses of
a tree are one bit pattern.  One case per regime of the plan: the number of row tiles against the waves of a workgroup, tapes in LDS
and in the global workspace, a population that fills the chip."""
import os
import sys

import numpy as np
import pytest
import torch

import evogp_amd  # noqa: F401  (registers the ops)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from grad_trees import ALL_FUNCS, random_forest  # noqa: E402
from helpers import fbits  # noqa: E402

pytestmark = pytest.mark.gpu

VAR_LEN = 3


def _cases():
    fill = 16 * torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 4096
    return [(64, 64, 50, "one tile, W 1"), (64, 64, 130, "three tiles, W 3"), (64, 64, 300, "W 4, LDS tapes"),
            (64, 65, 300, "global tapes at the smallest length that takes them"), (fill, 16, 100, "the population fills the chip, W 1")]


@pytest.mark.parametrize("case", range(5))
def test_three_passes_one_loss(rng, case):
    pop, gp_len, D, regime = _cases()[case]
    base = min(pop, 64)   # (the chip-filling population repeats 64 trees: the plan depends on the count, not on the trees)
    value, type_, size = random_forest(rng, base, gp_len, ALL_FUNCS, VAR_LEN, 1, max_depth=2 if gp_len < 64 else 5)
    size[7, 0] = 0        # one malformed row: an empty tree
    if pop > base:
        assert pop % base == 0
        value, type_, size = (np.tile(a, (pop // base, 1)) for a in (value, type_, size))
    X = rng.uniform(0.5, 1.5, (D, VAR_LEN)).astype(np.float32)
    y = rng.uniform(-1, 1, (D, 1)).astype(np.float32)
    v, t, s, Xd, yd = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (value, type_, size, X, y))
    hip = torch.ops.evogp_hip
    grad_loss = hip.tree_SR_gradient(pop, D, gp_len, VAR_LEN, 1, True, v, t, s, Xd, yd)[0].cpu().numpy()
    sub_loss = hip.tree_SR_subtree_errors(pop, D, gp_len, VAR_LEN, 1, True, v, t, s, Xd, yd)[0][:, 0].cpu().numpy()
    lm_loss = hip.tree_SR_normal_eq(pop, D, gp_len, VAR_LEN, 1, v, t, s, Xd, yd)[0].cpu().numpy()
    # Equal bits; for a NaN that means the same POSITIONS: every NaN is compared as one pattern (helpers.fbits), because its sign and
    # payload depend on the operand order the compiler chose in each kernel and carry no meaning.
    g, sb, lm = fbits(grad_loss), fbits(sub_loss), fbits(lm_loss)
    print(f"{regime}: pop {pop} gp_len {gp_len} D {D}: {int(np.isnan(grad_loss).sum())} NaN losses, "
          f"{int((g != sb).sum())} gradient/subtree and {int((g != lm).sum())} gradient/normal-equation losses differ in bits")
    assert np.isnan(grad_loss[7::base]).all() and np.isfinite(grad_loss).sum() >= pop // 4
    assert np.array_equal(g, sb), np.flatnonzero(g != sb)[:5]
    assert np.array_equal(g, lm), np.flatnonzero(g != lm)[:5]
