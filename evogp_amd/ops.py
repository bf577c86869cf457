"""``torch.ops.evogp_cuda.*`` — the reference's operator boundary, registered from C++.

Loading ``evogp_amd/lib/libevogp_torch.so`` (csrc/torch_ops.cpp) runs its static registrars, exactly as importing the
reference's extension module does (src/evogp/tree/__init__.py:2, torch_wrapper.cu:287-307):

* ``TORCH_LIBRARY(evogp_cuda)`` with the reference's five schemas verbatim (torch_wrapper.cu:294-298) and
  ``TORCH_LIBRARY_IMPL(evogp_cuda, CUDA)`` — ``tree_generate / tree_mutate / tree_crossover / tree_evaluate /
  tree_SR_fitness`` — so code written against them runs unchanged.  ROCm builds of PyTorch dispatch HIP tensors on the
  ``CUDA`` key; there is deliberately no CPU implementation (the reference has none, torch_wrapper.cu:301) and no fallback;
* the extra ops of this engine in the ``evogp_hip`` namespace (no counterpart in the reference).  The list lives in
  csrc/torch_ops.cpp, one schema per op in its ``TORCH_LIBRARY(evogp_hip)`` block; evogp_amd/tree/forest.py says which
  method calls which.  The six functions below spell out six of them for callers that hold raw tensors, not a Forest.

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
