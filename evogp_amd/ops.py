"""``torch.ops.evogp_cuda.*`` — the reference's operator boundary, registered from C++.

Loading ``evogp_amd/lib/libevogp_torch.so`` (csrc/torch_ops.cpp) runs its static registrars, exactly as importing the
reference's extension module does (src/evogp/tree/__init__.py:2, torch_wrapper.cu:287-307):

* ``TORCH_LIBRARY(evogp_cuda)`` with the reference's five schemas verbatim (torch_wrapper.cu:294-298) and
  ``TORCH_LIBRARY_IMPL(evogp_cuda, CUDA)`` — ``tree_generate / tree_mutate / tree_crossover / tree_evaluate /
  tree_SR_fitness`` — so code written against them runs unchanged.  ROCm builds of PyTorch dispatch HIP tensors on the
  ``CUDA`` key; there is deliberately no CPU implementation (the reference has none, torch_wrapper.cu:301) and no fallback;
* the extra ops of this engine in the ``evogp_hip`` namespace (no counterpart in the reference).  The list lives in
  csrc/torch_ops.cpp, one schema per op in its ``TORCH_LIBRARY(evogp_hip)`` block; evogp_amd/tree/forest.py says which
  method calls which.  The functions below spell out some of them for callers that hold raw tensors, not a Forest.

Every implementation validates like the reference's wrapper, allocates its outputs and calls the C ABI of
include/evogp_hip.h (``libevogp_hip.so``, loaded by ``_lib``) on torch's current stream; no Python runs per call.
"""
from __future__ import annotations

import os

import torch

from . import _lib  # the engine itself: fails loudly when the HIP library is missing

MAX_STACK = 1024
MAX_FULL_DEPTH = 10
FUNC_END = 29

TORCH_LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), "libevogp_torch.so")

if not os.path.exists(TORCH_LIB_PATH):
    raise ImportError(
        f"{TORCH_LIB_PATH} is missing: build the engine first (python -c 'import __graft_entry__ as g; g.build()'  or  "
        "make -C evogp_amd/csrc).  evogp_amd has no Python or CPU fallback for its operators.")
torch.ops.load_library(TORCH_LIB_PATH)


def tree_intervals(value, node_type, subtree_size, lower, upper):
    """``(lo, hi, flags)``, each (pop, gp_len): ``torch.ops.evogp_hip.tree_intervals`` (csrc/sr_interval.hip), the interval of every
    subtree of every single-output tree over the box ``lower[v] <= x[v] <= upper[v]`` (float32 ``(var_len,)`` tensors on the forest's
    device); flags bit 0 = the subtree may be a NaN, bit 1 = the row is malformed"""
    return torch.ops.evogp_hip.tree_intervals(value, node_type, subtree_size, lower, upper)


def tree_derivative_intervals(value, node_type, subtree_size, lower, upper, wrt):
    """``(vlo, vhi, vflags, dlo, dhi, dflags)``: ``torch.ops.evogp_hip.tree_derivative_intervals`` (csrc/sr_deriv.hip).  The first three,
    each (pop, gp_len), enclose the real value of every subtree over the box; the last three, each (K, pop, gp_len), bound its partial
    derivative in variable ``wrt[k]`` (int32 ``(K,)`` tensor on the forest's device, each entry in [0, var_len)); dflags bit 0 = the
    subtree may be discontinuous in that variable, bit 1 = the row is malformed, bit 2 = the variable occurs in it"""
    return torch.ops.evogp_hip.tree_derivative_intervals(value, node_type, subtree_size, lower, upper, wrt)


def tree_dimensions(value, node_type, subtree_size, var_units, label_units, check_root):
    """``(units, flags, violations)``: ``torch.ops.evogp_hip.tree_dimensions`` (csrc/sr_dims.hip), dimensional analysis of every
    single-output tree.  ``var_units`` int32 ``(var_len, K)`` and ``label_units`` int32 ``(K,)`` on the forest's device: numerators over
    25200, ``1 <= K <= 8``; ``check_root``: hold the root to ``label_units``.  ``units`` int32 (pop, gp_len, K): the unit of every subtree
    (of a consistent tree: under one consistent assignment of units to its constants); ``flags`` uint8 (pop, gp_len): 1 = free, 2 =
    violation, 4 = the row is malformed, 8 = root mismatch; ``violations`` int32 (pop,): 0 = consistent, -1 = malformed"""
    return torch.ops.evogp_hip.tree_dimensions(value, node_type, subtree_size, var_units, label_units, check_root)


def tree_structure(value, node_type, subtree_size, cost, operand_limit, rule_outer, rule_inner, rule_limit, max_depth, max_complexity):
    """``(complexity, height, depth, nest, flags, violations)``: ``torch.ops.evogp_hip.tree_structure`` (csrc/sr_structure.hip), the
    structural pass over every single-output tree.  int32 tensors on the forest's device: ``cost`` ``(32,)`` per symbol (function ids
    0 .. 28, 29 = variable, 30 = constant, 31 = unknown id), each in [0, 65535]; ``operand_limit`` ``(32, 3)``, -1 = none; ``rule_outer``,
    ``rule_inner`` ``(R,)`` sets of symbols (bit s = symbol s) and ``rule_limit`` ``(R,)`` in [0, 254], ``0 <= R <= 8``
    (``tree.utils.parse_structure`` makes them from dictionaries); ``max_depth``, ``max_complexity``: -1 = none.  ``complexity`` int32,
    ``height`` and ``depth`` int16, each (pop, gp_len); ``nest`` uint8 (pop, gp_len, R); ``flags`` uint8 (pop, gp_len): 1 = nesting, 2 =
    operand, 4 = the row is malformed, 8 = depth, 16 = complexity; ``violations`` int32 (pop,): 0 = passes, -1 = malformed"""
    return torch.ops.evogp_hip.tree_structure(value, node_type, subtree_size, cost, operand_limit, rule_outer, rule_inner, rule_limit,
                                              max_depth, max_complexity)


def tree_SR_semantic_hash(pop_size, data_points, gp_len, var_len, out_len, value, node_type, subtree_size, variables):
    """int64 ``(pop,)``: ``torch.ops.evogp_hip.tree_SR_semantic_hash`` (csrc/sr_semantic.hip), the bits of the 64-bit signature of every
    single-output tree's float32 predictions on the rows of ``variables`` ``(data_points, var_len)`` (-0.0 as +0.0, every NaN as one);
    trees that predict the same value on every row carry the same signature, a malformed row carries 0"""
    return torch.ops.evogp_hip.tree_SR_semantic_hash(pop_size, data_points, gp_len, var_len, out_len, value, node_type, subtree_size, variables)


def tree_SR_semantic_classes(pop_size, data_points, gp_len, var_len, out_len, value, node_type, subtree_size, variables, hash):
    """int32 ``(pop,)``: ``torch.ops.evogp_hip.tree_SR_semantic_classes``, the smallest index of a well-formed tree whose predictions
    equal those of tree t on every row; a malformed row is a class of its own.  ``hash`` int64 ``(pop,)`` only decides which trees are
    compared and may be any tensor in which equal trees carry equal words (``tree_SR_semantic_hash``'s, normally)"""
    return torch.ops.evogp_hip.tree_SR_semantic_classes(pop_size, data_points, gp_len, var_len, out_len, value, node_type, subtree_size,
                                                        variables, hash)


def tree_SR_subtree_signatures(pop_size, data_points, gp_len, var_len, out_len, value, node_type, subtree_size, variables):
    """int64 ``(pop, gp_len)``: ``torch.ops.evogp_hip.tree_SR_subtree_signatures`` (csrc/sr_subtree_sig.hip), ``tree_SR_semantic_hash``'s
    signature of EVERY SUBTREE of every single-output tree: entry ``[t, i]`` is the word ``tree_SR_semantic_hash`` gives the row that
    holds the nodes ``[i, i + size[t, i])`` alone (so column 0 is ``tree_SR_semantic_hash`` itself); 0 on the tail and on malformed rows"""
    return torch.ops.evogp_hip.tree_SR_subtree_signatures(pop_size, data_points, gp_len, var_len, out_len, value, node_type, subtree_size,
                                                          variables)


def subtree_library_select(sig, size, min_size, max_size, k):
    """``(member, count, n_classes)``: ``torch.ops.evogp_hip.subtree_library_select`` (csrc/sr_subtree_sig.hip).  Among the nodes with
    ``sig != 0`` and ``min_size <= size <= max_size`` (``sig`` int64, ``size`` int16, both ``(pop, gp_len)``), the classes of equal
    signature ordered by (count descending, representative ascending), a class's representative being its member of smallest (size,
    flat index).  ``member`` int32 ``(k,)``: the representatives' flat indices ``t * gp_len + i``, -1 past the last class; ``count`` int32
    ``(k,)``: the class sizes, 0 there; ``n_classes`` int32 ``(1,)``.  ``1 <= k <= 1024``.  Signatures alone decide: a collision merges
    two classes"""
    return torch.ops.evogp_hip.subtree_library_select(sig, size, min_size, max_size, k)


def tree_SR_subtree_introns(pop_size, data_points, gp_len, var_len, out_len, value, node_type, subtree_size, variables, sig):
    """int16 ``(pop, gp_len)``: ``torch.ops.evogp_hip.tree_SR_subtree_introns`` (csrc/sr_introns.hip).  ``rep[t, i]`` is the descendant
    of node i that takes the value of the subtree at i on EVERY row of ``variables`` (equal bit patterns, or both NaN), or i itself.  ``sig``
    int64 ``(pop, gp_len)`` proposes -- ``tree_SR_subtree_signatures``' output on the same rows finds the introns, any other array finds
    fewer -- and the tape verifies, so ``rep`` never names an unequal node; i on the tail and on malformed rows"""
    return torch.ops.evogp_hip.tree_SR_subtree_introns(pop_size, data_points, gp_len, var_len, out_len, value, node_type, subtree_size,
                                                       variables, sig)


def tree_remove_introns(value, node_type, subtree_size, rep):
    """``(value, node_type, subtree_size, removed)``: ``torch.ops.evogp_hip.tree_remove_introns`` (csrc/sr_introns.hip): every node
    replaced by ``rep`` (int16 ``(pop, gp_len)``; an entry that is no descendant of its node counts as the node) from the root down, zero
    tails, malformed rows copied; ``removed`` int32 ``(pop,)``: the nodes each tree lost"""
    return torch.ops.evogp_hip.tree_remove_introns(value, node_type, subtree_size, rep)


def tree_SR_pair_moments(value, node_type, subtree_size, mate_value, mate_type, mate_size, variables, labels, first, candidates):
    """``(own, moments)``: ``torch.ops.evogp_hip.tree_SR_pair_moments`` (csrc/sr_pair.hip).  Event e pairs tree ``first[e]`` (int32
    ``(E,)``) of the forest with the trees ``candidates[e, m]`` (int32 ``(E, M)``, ``M <= 16``) of the mate forest (any ``gp_len``, the same
    ``var_len``); with ``r = (double)p - (double)labels`` (``labels`` float32 ``(D,)`` or None: 0) ``own`` float64 ``(E,)`` is ``sum r_a^2`` and
    ``moments`` float64 ``(E, M, 3)`` is ``sum r_b^2, sum r_a r_b, sum (p_a - p_b)^2``; NaN by the rule of the unusable tree.  A word
    depends on its pair and the dataset alone, bit for bit"""
    return torch.ops.evogp_hip.tree_SR_pair_moments(value, node_type, subtree_size, mate_value, mate_type, mate_size, variables, labels, first,
                                                    candidates)


def tree_SR_gram(value, node_type, subtree_size, variables, labels, index, residuals):
    """``(G, lin, usable)``: ``torch.ops.evogp_hip.tree_SR_gram`` (csrc/sr_gram.hip).  For the trees ``index`` (int32 ``(n,)``, ``n <= 8192``)
    of a single-output forest, with ``v = (double)p - (double)labels`` under ``residuals`` (``labels`` float32 ``(D,)``) and ``v = (double)p``
    otherwise: ``G`` float64 ``(n, n)`` is ``sum_d v_i v_j`` on the float64 matrix cores, ``lin`` float64 ``(n, 2)`` is ``sum v_i, sum v_i y``
    (0 without labels), ``usable`` bool ``(n,)``; the row, column and ``lin`` words of an unusable tree (malformed, a non-finite prediction, an
    index outside the forest) are NaN.  A word depends on its two trees and the dataset alone, bit for bit, and ``G`` equals ``G.T``"""
    return torch.ops.evogp_hip.tree_SR_gram(value, node_type, subtree_size, variables, labels, index, residuals)


def tree_SR_neighbours(value, node_type, subtree_size, variables, index, k, radius2):
    """``(dist2, neighbour, count, norm, usable)``: ``torch.ops.evogp_hip.tree_SR_neighbours`` (csrc/sr_neigh.hip).  For the trees
    ``index`` (int32 ``(n,)``, ``n <= 131072``, ``n * roundup4(D) <= 2^29``) of a single-output forest, with ``G`` and its order those of
    ``tree_SR_gram`` without residuals and ``d2(i, j) = max(0, fma(-2, G_ij, G_ii + G_jj))``: ``dist2`` float64 and ``neighbour`` int32
    ``(n, k)``, ``k <= 16``, are the k usable positions ``j != i`` smallest by ``(d2, j)`` (``+inf`` / -1 beyond their number, NaN / -1 for an
    unusable tree); ``count`` int32 ``(n, R)`` the neighbours with ``d2 <= radius2[r]`` (float64 ``(R,)``, ``R <= 8``, squared radii);
    ``norm`` float64 ``(n,)`` is ``G_ii``; ``usable`` bool ``(n,)``.  The ``(n, n)`` matrix is never stored; bit-identical under any split"""
    return torch.ops.evogp_hip.tree_SR_neighbours(value, node_type, subtree_size, variables, index, k, radius2)


def tree_SR_simulate(value, node_type, subtree_size, x0, u, scheme, dt):
    """``states`` float32 ``(pop, B, T, S)``: ``torch.ops.evogp_hip.tree_SR_simulate`` (csrc/sr_simulate.hip).  Every tree of a forest with
    ``input_len = S + U`` and ``output_len = S`` (``scheme`` 3, narx: ``output_len = 1``, S lags) is stepped T times from ``x0`` float32
    ``(B, S)`` under ``u`` float32 ``(B, T, U)`` inside one kernel; ``scheme`` 0 map, 1 euler, 2 rk4, 3 narx; ``dt`` is rounded to float32.
    A trajectory whose new state is not finite is dead: NaN from that step on; a malformed tree is NaN everywhere.  The bits are those
    of stepping ``tree_evaluate`` with the float32 formulas of include/evogp_hip.h"""
    return torch.ops.evogp_hip.tree_SR_simulate(value, node_type, subtree_size, x0, u, scheme, dt)


def tree_SR_simulation_loss(value, node_type, subtree_size, x0, u, target, scheme, dt):
    """``loss`` float64 ``(pop, S)`` (``(pop, 1)`` for narx): ``torch.ops.evogp_hip.tree_SR_simulation_loss`` (csrc/sr_simulate.hip).  The
    mean over trajectories and steps of ``((double)x_s - (double)target_s)^2`` of ``tree_SR_simulate``'s states against ``target`` float32
    ``(B, T, S)`` (``(B, T)`` for narx), in a fixed order, without the ``(pop, B, T, S)`` array; NaN for a tree with a dead trajectory and
    for a malformed tree.  The same bits from run to run and whatever population the tree stands in"""
    return torch.ops.evogp_hip.tree_SR_simulation_loss(value, node_type, subtree_size, x0, u, target, scheme, dt)


def tree_SR_simulation_sensitivities(value, node_type, subtree_size, x0, u, scheme, dt):
    """``(states, sens)``: ``torch.ops.evogp_hip.tree_SR_simulation_sensitivities`` (csrc/sr_simulate_sens.hip).  ``states`` float32
    ``(pop, B, T, S)`` are ``tree_SR_simulate``'s bits; ``sens`` float32 ``(pop, B, T, S, 8)`` their derivatives in each tree's first 8
    CONST nodes in prefix order, carried through time by dual numbers inside the kernel (include/evogp_hip.h has the rule).  Slots past
    the tree's constants are exactly 0; every slot is NaN from the step a trajectory dies and for a malformed tree"""
    return torch.ops.evogp_hip.tree_SR_simulation_sensitivities(value, node_type, subtree_size, x0, u, scheme, dt)


def tree_SR_simulation_normal_eq(value, node_type, subtree_size, x0, u, target, state_weight, scheme, dt):
    """``(loss64, loss, normal)``: ``torch.ops.evogp_hip.tree_SR_simulation_normal_eq`` (csrc/sr_simulate_sens.hip).  ``loss64`` float64
    ``(pop, SC)`` is ``tree_SR_simulation_loss``'s, bit for bit; ``loss`` float32 ``(pop,)`` its sum weighted by ``state_weight`` float32
    ``(SC,)``; ``normal`` float32 ``(pop, 44)`` the Gauss-Newton model of that sum in the tree's first 8 constants, in the layout
    ``tree_SR_lm_step`` takes.  A tree with a dead trajectory or a malformed tree: NaN losses, a zero row.  No ``(pop, B, T, S, 8)`` array"""
    return torch.ops.evogp_hip.tree_SR_simulation_normal_eq(value, node_type, subtree_size, x0, u, target, state_weight, scheme, dt)


def rank_rows(values, payload, seg_start, max_segment):
    """``(r2, consts, status)``: ``torch.ops.evogp_hip.rank_rows`` (csrc/sr_rank.hip).  ``values`` float32 ``(D,)`` are mid-ranked within
    the contiguous segments ``seg_start`` int32 ``(G + 1,)`` (each of at most ``max_segment <= 8192`` rows): ``r2`` int32 ``(D,)`` is the
    doubled mid-rank, ``#less + #less-or-equal + 1``; ``consts`` int64 ``(G, 2)`` is ``sum q, sum q^2`` of ``payload`` int32 ``(D,)`` per
    segment, or of ``r2`` when ``payload`` is None; ``status`` int32 ``(G,)`` is 1 for a segment that holds a NaN (its ``r2`` is 0)"""
    return torch.ops.evogp_hip.rank_rows(values, payload, seg_start, max_segment)


def tree_SR_rank_stats(value, node_type, subtree_size, variables, payload, seg_start, max_segment, metric, want_words, want_fused,
                       want_scores):
    """``(words, fused, scores, status)``: ``torch.ops.evogp_hip.tree_SR_rank_stats`` (csrc/sr_rank.hip).  Per tree and row segment the float32
    predictions are sorted inside the evaluation kernel; with ``R2`` their doubled mid-ranks and ``payload`` int32 ``(D,)`` in [0, 16384],
    ``words`` int64 ``(pop, G, 2)`` is ``sum R2 * payload, sum R2^2``; ``fused`` float64 ``(pop, 3)`` is the sum, the sum of squares and the
    count of the defined segment scores of ``metric`` (0 Spearman, 1 AUC), added in ascending segment; ``scores`` float64 ``(pop, G)`` is those scores themselves, NaN where undefined; ``status`` uint8 ``(pop,)`` is 1
    for a malformed tree or one with a NaN prediction (words 0, fused and scores NaN).  An output that is not wanted comes back empty"""
    return torch.ops.evogp_hip.tree_SR_rank_stats(value, node_type, subtree_size, variables, payload, seg_start, max_segment, metric,
                                                  want_words, want_fused, want_scores)
