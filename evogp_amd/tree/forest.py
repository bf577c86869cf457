"""Forest — a population of expression trees as three dense row-major device tensors.

    batch_node_value   float32 (pop, max_tree_len)   variable index / constant / function id / OUT bits
    batch_node_type    int16   (pop, max_tree_len)   NType, bit 7 = OUT_NODE
    batch_subtree_size int16   (pop, max_tree_len)   subtree sizes, [:, 0] = live tree length

The constructor, generation, evaluation, the genetic operators and the container protocol follow src/evogp/tree/forest.py:11-499; the
rest has no counterpart in the reference.  Every heavy method is one call into ``torch.ops.evogp_cuda.*`` / ``evogp_hip.*``
(evogp_amd/ops.py), i.e. one HIP kernel.

    construction          random_generate, zero_generate
    evaluation            forward, batch_forward, prepare_forward, SR_fitness, SR_case_errors (per case, for lexicase selection)
    constants             SR_gradient, SR_normal_equations, optimize_constants (gradient descent or Levenberg-Marquardt)
    structural duplicates structure_hash, duplicate_classes, unique (csrc/dedup.hip); ``dedup=True`` elsewhere runs once per class
    semantic duplicates   semantic_hash, semantic_classes, semantic_unique: trees equal on every data row
    subtrees              SR_subtree_errors, simplify: the loss of every subtree; the smaller tree that is no worse
    subtree library       SR_subtree_signatures, subtree_library: the signature of every subtree; the distinct subtrees of a forest
    introns               SR_subtree_introns, remove_introns: the nodes that take a descendant's value on every row, and the forest without them
    linear scaling        SR_scaled_fitness, apply_scaling: the loss under the least-squares slope and intercept; the tree with them
    weighted losses       SR_weighted_loss: sample weights, Huber / pinball / log-cosh, training and validation columns in one pass
    weighted scaling      SR_weighted_scaled_fitness: linear scaling fitted on one weight row, scored on up to 8, in one pass
    multi-gene            SR_gene_fitness, SR_gene_moments, gene_predict: a tree's outputs as features of a least-squares model
    intervals             SR_intervals, safe_mask: bounds of every subtree over a box of inputs; the trees finite on all of it
    derivative bounds     SR_derivative_intervals, monotone_mask: bounds of the partial derivatives; the trees proven monotone
    input gradients       SR_input_gradients, SR_derivative_loss: d tree / d x on the data rows; the derivative loss and violations
    backpropagation       SR_desired_semantics, SR_backprop_match: the values a subtree would have to return; the nearest library member
    pairs                 SR_pair_moments, semantic_distance: the residual inner products of pairs of trees; their distance
    midpoint              SR_midpoint_semantics, SR_midpoint_match: the same towards the midpoint of a tree and its mate (no labels)
    dimensions            SR_dimensions, dimension_mask: the physical unit of every subtree; the trees that can be made consistent
    structure             SR_structure, structure_mask, complexity: depth, weighted complexity, operand and nesting limits
    genetic operators     mutate, crossover
    container, pickling   indexing, iteration, ``+``, ``__getstate__`` / ``__setstate__``

Two deliberate differences from the reference: ``batch_forward`` does NOT replicate the forest ``batch`` times (forest.py:151-161:
three ``repeat_interleave`` copies + ``x.repeat``) but calls the non-replicating ``evogp_hip::tree_batch_evaluate`` and returns the same
``(pop, batch, out)`` tensor; ``random_generate`` accepts ``tree_index_offset`` / ``keys`` so that a sharded population can be made
bit-identical to the single-device one.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch
from torch import Tensor

from . import utils as _utils
from .descriptor import GenerateDescriptor
from .tree import Tree
from .utils import NType, box_side, check_tensor, check_units, draw_keys, parse_monotonic, parse_structure

_PREPARED_FORWARD = __import__("os").environ.get("EVOGP_PREPARED_FORWARD", "1") != "0"
LM_MAX_CONSTS = 8  # constants per tree the Levenberg-Marquardt optimiser tunes (include/evogp_hip.h EVOGP_LM_MAX_CONSTS)
GENES_MAX = 8  # outputs per tree SR_gene_fitness takes as features (include/evogp_hip.h EVOGP_GENES_MAX)
WLOSS_MAX_WEIGHTS = 8  # weight rows per SR_weighted_loss call (include/evogp_hip.h EVOGP_WLOSS_MAX_WEIGHTS)
PAIR_MAX_CANDIDATES = 16     # candidates per event of SR_pair_moments (include/evogp_hip.h EVOGP_PAIR_MAX_CANDIDATES)
BACKPROP_MAX_LIBRARY = 1024  # library members per SR_backprop_match call (include/evogp_hip.h EVOGP_BACKPROP_MAX_LIB)
XGRAD_MAX_VARS = 8  #variables per SR_input_gradients / SR_derivative_loss call (include/evogp_hip.h EVOGP_XGRAD_MAX_VARS)
LOSS_KINDS = {"mse": 0, "mae": 1, "huber": 2, "pinball": 3, "logcosh": 4}  # include/evogp_hip.h EVOGP_LOSS_*
_WRAP_FUNCS = (1 << 1) | (1 << 3)  # Func.ADD, Func.MUL: the two nodes apply_scaling puts on top of a tree
_SR_MODES = {"hybrid parallel": 0, "data parallel": 1, "tree parallel": 2, "auto": 4}  # forest.py:340-347


def check_loss(loss, param) -> Optional[float]:
    """the parameter of ``SR_weighted_loss``'s ``loss`` as a float (None for a loss that has none), or ``ValueError``"""
    if loss not in LOSS_KINDS:
        raise ValueError(f"loss should be one of {list(LOSS_KINDS)}, but got {loss!r}")
    if loss not in ("huber", "pinball"):
        if param is not None:
            raise ValueError(f"loss={loss!r} takes no param, but got {param!r}")
        return None
    if param is None or isinstance(param, bool) or not isinstance(param, (int, float)):
        raise ValueError(f"loss={loss!r} needs a float param, but got {param!r}")
    param = float(param)
    if loss == "huber" and not 0.0 < param < float("inf"):
        raise ValueError(f"the delta of the huber loss should be finite and > 0, but got {param}")
    if loss == "pinball" and not 0.0 < param < 1.0:
        raise ValueError(f"the tau of the pinball loss should lie in (0, 1), but got {param}")
    return param


def _symmetric(packed: Tensor, K: int) -> Tensor:
    """``(pop, K (K + 1) / 2)`` upper triangles in row-major order, as the kernels pack them -> the mirrored ``(pop, K, K)`` matrices"""
    iu = torch.triu_indices(K, K, device=packed.device)
    full = packed.new_zeros((packed.shape[0], K, K))
    full[:, iu[0], iu[1]] = packed
    full[:, iu[1], iu[0]] = packed
    return full


def _root_safe(lo: Tensor, hi: Tensor, flags: Tensor, max_abs: float) -> Tensor:
    """(pop,) bool from per-node enclosures: the root can not be a NaN, both its bounds are finite and neither exceeds ``max_abs``"""
    lo, hi = lo[:, 0], hi[:, 0]
    return (flags[:, 0] == 0) & torch.isfinite(lo) & torch.isfinite(hi) & (torch.maximum(lo.abs(), hi.abs()) <= max_abs)


class Forest:
    def __init__(self, input_len, output_len, batch_node_value: Tensor, batch_node_type: Tensor,
                 batch_subtree_size: Tensor, func_mask: int = 0):
        """``func_mask`` (no counterpart in the reference): bit f = function id f may occur in the trees, 0 = unknown.  Set by
        ``random_generate`` from the descriptor and handed on by the operators that combine forests; a forest built from raw
        tensors is "unknown".  ``SR_fitness`` passes it on as long as the tensors are untouched."""
        self.input_len = input_len
        self.output_len = output_len
        self.pop_size, self.max_tree_len = batch_node_value.shape
        shape = (self.pop_size, self.max_tree_len)
        assert batch_node_type.shape == shape, f"node_type shape should be {shape}, but got {batch_node_type.shape}"
        assert batch_subtree_size.shape == shape, (
            f"subtree_size shape should be {shape}, but got {batch_subtree_size.shape}")
        self.batch_node_value = batch_node_value
        self.batch_node_type = batch_node_type
        self.batch_subtree_size = batch_subtree_size
        self._func_mask = (int(func_mask), self._forest_key()) if func_mask else None

    @property
    def func_mask(self) -> int:
        """the functions that may occur in this forest (bit f = function id f), 0 when unknown or when a tensor was replaced or
        written in place since the mask was set"""
        m = getattr(self, "_func_mask", None)
        if m is None or m[1] != self._forest_key():
            return 0
        return m[0]

    @staticmethod
    def join_masks(*masks: int) -> int:
        """the mask of a forest whose trees come from forests / descriptors with these masks: unknown if any is"""
        out = 0
        for m in masks:
            if not m:
                return 0
            out |= m
        return out

    # ---- construction -------------------------------------------------------------------------
    @staticmethod
    def random_generate(pop_size: int, descriptor: GenerateDescriptor, keys: Optional[Tensor] = None,
                        tree_index_offset: int = 0) -> "Forest":
        assert isinstance(pop_size, int) and pop_size > 0, "pop_size should be a positive integer"
        if keys is None:
            keys = draw_keys()
        args = (pop_size, descriptor.max_tree_len, descriptor.input_len, descriptor.output_len,
                descriptor.const_samples.shape[0], descriptor.out_prob, descriptor.const_prob, keys,
                descriptor.depth2leaf_probs, descriptor.roulette_funcs, descriptor.const_samples)
        if tree_index_offset:
            value, ntype, size = torch.ops.evogp_hip.tree_generate_offset(*args, tree_index_offset)
        else:
            value, ntype, size = torch.ops.evogp_cuda.tree_generate(*args)
        return Forest(descriptor.input_len, descriptor.output_len, value, ntype, size, func_mask=descriptor.func_mask)

    @staticmethod
    def zero_generate(pop_size: int, max_tree_len: int, input_len: int, output_len: int) -> "Forest":
        """pop_size copies of the constant-0 tree (forest.py:86-110)."""
        dev = _utils.default_device()
        value = torch.zeros((pop_size, max_tree_len), dtype=torch.float32, device=dev)
        ntype = torch.zeros((pop_size, max_tree_len), dtype=torch.int16, device=dev)
        size = torch.zeros((pop_size, max_tree_len), dtype=torch.int16, device=dev)
        ntype[:, 0] = NType.CONST
        size[:, 0] = 1
        return Forest(input_len, output_len, value, ntype, size)

    def _tensors(self):
        return (self.batch_node_value.contiguous(), self.batch_node_type.contiguous(),
                self.batch_subtree_size.contiguous())

    # ---- evaluation ---------------------------------------------------------------------------
    def _forest_key(self):
        v, t, s = self.batch_node_value, self.batch_node_type, self.batch_subtree_size
        return (v.data_ptr(), t.data_ptr(), s.data_ptr(), v._version, t._version, s._version, self.pop_size, self.max_tree_len)

    def prepare_forward(self):
        """Decode a multi-output forest once for many ``forward`` calls (a rollout evaluates the same forest once per
        environment step, src/evogp/problem/brax_problem.py:54-93): the operation lists of csrc/evaluate_prepared.hip.  Returns
        the cached (workspace, with_fallback) or None when the forest is not eligible.  The cache is keyed on the tensors'
        identity and version counters, so an in-place edit of the forest invalidates it; ``forward`` calls this itself from
        its SECOND call on an unchanged forest on (one host sync per preparation: the count of trees left to the stack
        interpreter)."""
        v, t, s = self.batch_node_value, self.batch_node_type, self.batch_subtree_size
        if not (v.is_cuda and 2 <= self.output_len <= 32 and self.input_len <= 255 and v.is_contiguous() and t.is_contiguous() and s.is_contiguous()):
            return None
        key = self._forest_key()
        cached = getattr(self, "_prepared", None)
        if cached is not None and cached[0] == key:
            return cached[1], cached[2]
        ws, info = torch.ops.evogp_hip.tree_evaluate_prepare(self.pop_size, self.max_tree_len, self.input_len, self.output_len, v, t, s)
        with_fallback = bool(int(info[0]) != 0)
        self._prepared = (key, ws, with_fallback)
        return ws, with_fallback

    def forward(self, x: Tensor) -> Tensor:
        """One input row per tree: x (pop, input_len) -> (pop, output_len)."""
        x = check_tensor(x, self.batch_node_value.device)
        assert x.shape == (self.pop_size, self.input_len), (
            f"x shape should be ({self.pop_size}, {self.input_len}), but got {x.shape}")
        # a forest that is evaluated AGAIN unchanged is a policy population inside a rollout: from the second call on it runs
        # from its operation lists (multi-output forests only; EVOGP_PREPARED_FORWARD=0 switches this off).  Preparing costs a
        # host sync, so it never happens while the stream is being captured: RolloutProblem prepares before it captures.
        if self.output_len > 1 and x.is_cuda and _PREPARED_FORWARD:
            key = self._forest_key()
            prepared = None
            cached = getattr(self, "_prepared", None)
            if cached is not None and cached[0] == key:
                prepared = cached[1:]
            elif getattr(self, "_forward_seen", None) == key and not torch.cuda.is_current_stream_capturing():
                prepared = self.prepare_forward()
            self._forward_seen = key
            if prepared is not None:
                return torch.ops.evogp_hip.tree_evaluate_prepared(self.pop_size, self.max_tree_len, self.input_len, self.output_len,
                                                                  *self._tensors(), prepared[0], prepared[1], x.contiguous().to(torch.float32))
        return torch.ops.evogp_cuda.tree_evaluate(self.pop_size, self.max_tree_len, self.input_len, self.output_len,
                                                  *self._tensors(), x.contiguous().to(torch.float32))

    def batch_forward(self, x: Tensor) -> Tensor:
        """Shared input rows: x (batch, input_len) -> (pop, batch, output_len)."""
        x = check_tensor(x, self.batch_node_value.device)
        assert x.dim() == 2 and x.shape[1] == self.input_len, (
            f"x shape[1] should be {self.input_len}, but got {tuple(x.shape)}")
        return torch.ops.evogp_hip.tree_batch_evaluate(*self._shape(x), *self._tensors(), x.contiguous().to(torch.float32))

    def class_stats(self, inputs: Tensor, labels: Tensor, groups: Optional[Tensor] = None, n_groups: Optional[int] = None):
        """``(hits, predicted, loss)`` of a classifier forest (one output per class) in one interpretation (csrc/cls_stats.hip), over up
        to 8 row splits at once: ``hits[t, g, c]`` int32, the rows of split g with label c that tree t predicts as c; ``predicted[t, g,
        c]`` int32, the rows of split g it predicts as c; ``loss[t, g]`` float64, its mean soft-max cross-entropy over split g (every
        row's loss clamped to ``-log(1e-15)`` as the reference clips the probabilities).  The prediction is ``Classification``'s:
        ``argmax(clip(softmax(outputs)))``.  The ``(pop, D, classes)`` outputs are never stored, nothing synchronises with the host,
        and the result is bit-identical from run to run.

        ``labels``: ``(D,)`` int, or float holding integers (checked here, one host sync; pass int labels to avoid it).  ``groups``:
        None (every row in split 0), a ``(D,)`` bool (``False`` -> 0, ``True`` -> 1) or a ``(D,)`` int tensor with ``n_groups`` splits
        (default 2 for bool; required for int, at most 8).  A row whose group lies outside ``[0, n_groups)`` or whose label lies outside
        ``[0, output_len)`` is looked at in no output: a tree may be NaN there.  A row WITH a split where an output is NaN or the largest
        output is infinite makes ``loss[t, g]`` of that split NaN; an empty split gives NaN; a malformed tree predicts class 0 with loss
        NaN.  ``ValueError`` for a single-output forest, more than 16 outputs, a shape or a dtype."""
        dev = self.batch_node_value.device
        if not 2 <= self.output_len <= 16:
            raise ValueError(f"class_stats works on forests with 2 to 16 outputs (one per class), but output_len is {self.output_len}")
        inputs, labels = check_tensor(inputs, dev), check_tensor(labels, dev)
        n = inputs.shape[0]
        if inputs.dim() != 2 or inputs.shape != (n, self.input_len) or n == 0:
            raise ValueError(f"inputs shape should be (D, {self.input_len}) with D > 0, but got {tuple(inputs.shape)}")
        if labels.shape != (n,):
            raise ValueError(f"labels shape should be ({n},), but got {tuple(labels.shape)}")
        if labels.dtype == torch.bool or labels.is_complex():
            raise ValueError(f"labels should be an int tensor or a float tensor of integers, but got {labels.dtype}")
        if labels.is_floating_point():
            if not bool(torch.all(labels == torch.round(labels))):
                raise ValueError("labels should hold integers: a label like 1.5 names no class")
            labels = labels.clamp(-1.0, float(self.output_len))   # (out of range stays out of range, whatever the cast does beyond int32)
        else:
            labels = labels.clamp(-1, self.output_len)
        if groups is None:
            if n_groups not in (None, 1):
                raise ValueError(f"n_groups should be 1 (or None) without groups, but got {n_groups}")
            n_groups = 1
        else:
            groups = check_tensor(groups, dev)
            if groups.shape != (n,) or groups.is_floating_point() or groups.is_complex():
                raise ValueError(f"groups should be a ({n},) bool or int tensor, but got {groups.dtype}{tuple(groups.shape)}")
            if groups.dtype == torch.bool:
                n_groups = 2 if n_groups is None else n_groups
            elif n_groups is None:
                raise ValueError("n_groups is required with int groups")
            else:
                groups = groups.clamp(-1, 8)
            if not 1 <= int(n_groups) <= 8:
                raise ValueError(f"n_groups should be in [1, 8], but got {n_groups}")
            groups = groups.to(torch.int32).contiguous()
        return tuple(torch.ops.evogp_hip.tree_batch_class_stats(*self._shape(inputs), *self._tensors(), inputs.contiguous().to(torch.float32),
                                                                labels.to(torch.int32).contiguous(), groups, int(n_groups)))

    def _sr_data(self, inputs: Tensor, labels: Tensor):
        """the dataset as the kernels take it: on the forest's device, shapes checked, contiguous float32"""
        inputs, labels = check_tensor(inputs, self.batch_node_value.device), check_tensor(labels, self.batch_node_value.device)
        n = inputs.shape[0]
        assert inputs.shape == (n, self.input_len), (
            f"inputs shape should be ({n}, {self.input_len}), but got {inputs.shape}")
        assert labels.shape == (n, self.output_len), (
            f"outputs shape should be ({n}, {self.output_len}), but got {labels.shape}")
        return inputs.contiguous().to(torch.float32), labels.contiguous().to(torch.float32)

    def _shape(self, inputs: Tensor):
        """the five integers every dataset op starts with: (pop_size, data rows, max_tree_len, input_len, output_len)"""
        return self.pop_size, inputs.shape[0], self.max_tree_len, self.input_len, self.output_len

    def _single_output(self, what: str, error=AssertionError):
        """the one guard of the single-output methods; ``error``: the type the method is documented to raise"""
        if self.output_len != 1:
            raise error(f"{what} works on single-output trees only, but output_len is {self.output_len}")

    def SR_fitness(self, inputs: Tensor, labels: Tensor, use_MSE: bool = True, execute_mode: str = "auto") -> Tensor:
        """Mean squared / absolute error of every tree over the dataset: (pop,), positive."""
        inputs, labels = self._sr_data(inputs, labels)
        assert execute_mode in _SR_MODES, f"execute_mode should be one of {list(_SR_MODES)}, but got {execute_mode}"
        mask = self.func_mask
        if inputs.is_cuda and mask:
            # what this object knows beyond the tensors: the function set of the trees (the descriptors they came from)
            return torch.ops.evogp_hip.tree_SR_fitness_masked(*self._shape(inputs), use_MSE, *self._tensors(), inputs, labels,
                                                              _SR_MODES[execute_mode], mask)
        return torch.ops.evogp_cuda.tree_SR_fitness(*self._shape(inputs), use_MSE, *self._tensors(), inputs, labels,
                                                    _SR_MODES[execute_mode])

    def SR_case_errors(self, inputs: Tensor, labels: Tensor, use_MSE: bool = True) -> Tensor:
        """Per-case errors ``(pop, D)``: entry ``[t, d]`` is the squared (``use_MSE``) or absolute error of tree t on row d, averaged
        over the outputs, in float32 (NaN stays NaN).  The predictions are ``batch_forward``'s, bit for bit.  The tensor is the transposed
        view of a case-major ``(D, pop)`` one (strides ``(1, pop)``): one case across many trees is contiguous, which is how lexicase
        selection reads it (csrc/lexicase.hip).  Its mean over the rows is what ``SR_fitness`` returns, up to the fitness path's order
        of summation."""
        inputs, labels = self._sr_data(inputs, labels)
        return torch.ops.evogp_hip.tree_SR_case_errors(*self._shape(inputs), use_MSE, *self._tensors(), inputs, labels).t()

    def _tuning_loss(self, what: str, inputs: Tensor, use_MSE: bool, weights, loss, param):
        """the loss the constants are tuned under: None when ``weights``, ``loss`` and ``param`` are all None (the unweighted ops run,
        as ever), else ``(weights, kind, param)`` as the weighted ops take them -- ``weights`` a contiguous float32 ``(D,)`` tensor on
        the forest's device or None, ``kind`` the integer of ``LOSS_KINDS``.  ``ValueError`` for what the rules of ``SR_gradient`` exclude"""
        if weights is None and loss is None and param is None:
            return None
        self._single_output(f"{what} with weights, loss or param", ValueError)
        if loss is None:
            loss = "mse" if use_MSE else "mae"
        elif not use_MSE:
            raise ValueError(f"{what}: loss={loss!r} says which error is minimised, so use_MSE must be left True")
        param = check_loss(loss, param)
        if weights is not None:
            n = inputs.shape[0]
            if not isinstance(weights, Tensor) or not weights.dtype.is_floating_point or weights.shape != (n,):
                raise ValueError(f"weights should be a ({n},) floating-point tensor, but got "
                                 f"{(tuple(weights.shape), weights.dtype) if isinstance(weights, Tensor) else weights!r}")
            weights = weights.detach().to(self.batch_node_value.device).contiguous().to(torch.float32)
        return weights, LOSS_KINDS[loss], 0.0 if param is None else param

    def SR_gradient(self, inputs: Tensor, labels: Tensor, use_MSE: bool = True, weights: Optional[Tensor] = None,
                    loss: Optional[str] = None, param: Optional[float] = None):
        """``(loss, grad)``: ``loss`` (pop,) is what ``SR_fitness`` returns, ``grad`` (pop, max_tree_len) is d loss / d value at every
        constant node and exactly 0 elsewhere (one reverse-mode HIP pass, csrc/sr_grad.hip).  Malformed trees: NaN loss, zero row.

        ``weights`` (a ``(D,)`` floating tensor), ``loss`` and ``param`` (those of ``SR_weighted_loss``; single-output forests): loss
        and gradient of ``sum_d w_d rho(tree(x_d) - y_d) / sum_d w_d`` instead -- the loss ``SR_weighted_loss`` scores by, on the rows
        it scores.  ``weights`` alone means ``"mse"``, or ``"mae"`` with ``use_MSE=False``; ``loss`` with ``use_MSE=False`` is a
        ``ValueError``.  A row of weight 0 is not looked at; the loss is NaN and the row zero also where a row WITH weight has a
        non-finite prediction, and for every tree when ``weights`` holds a negative or non-finite entry or sums to 0 (decided on the
        device).  With all three left at None the call is the unweighted one, unchanged."""
        inputs, labels = self._sr_data(inputs, labels)
        own = self._tuning_loss("SR_gradient", inputs, use_MSE, weights, loss, param)
        if own is None:
            return torch.ops.evogp_hip.tree_SR_gradient(*self._shape(inputs), use_MSE, *self._tensors(), inputs, labels)
        return torch.ops.evogp_hip.tree_SR_weighted_gradient(*self._shape(inputs), *self._tensors(), inputs, labels, *own)

    def SR_normal_equations(self, inputs: Tensor, labels: Tensor, weights: Optional[Tensor] = None):
        """``(loss, A, b, const_index)`` of the Gauss-Newton model of the MSE loss in each tree's OPTIMISED constants: its first
        ``min(nc, K)`` CONST nodes in prefix order, ``K = LM_MAX_CONSTS = 8`` (further constants are held fixed).  With ``J`` the per-row
        Jacobian of the prediction in those constants and ``r = pred - y``: ``A = J^T J / D`` (pop, K, K), symmetric; ``b = J^T r / D``
        (pop, K), half the gradient of the loss; ``loss`` (pop,) is ``SR_gradient``'s; ``const_index`` (pop, K) int64 is the node position
        of each optimised constant, -1 where the tree has fewer.  Rows and columns of absent constants are exactly 0.  Malformed
        trees: NaN loss, zero ``A`` and ``b``.  One HIP pass (csrc/sr_lm.hip); single-output forests only.

        ``weights`` (a ``(D,)`` floating tensor): the model of the WEIGHTED MSE, ``A = sum w J^T J / sum w``, ``b = sum w J^T r / sum w``,
        ``loss`` that of ``SR_gradient(weights=weights)`` bit for bit, under its rules for rows of weight 0 and unusable weights."""
        self._single_output("SR_normal_equations", ValueError if weights is not None else AssertionError)
        inputs, labels = self._sr_data(inputs, labels)
        value, ntype, size = self._tensors()
        if weights is None:
            loss, normal = torch.ops.evogp_hip.tree_SR_normal_eq(*self._shape(inputs), value, ntype, size, inputs, labels)
        else:
            w = self._tuning_loss("SR_normal_equations", inputs, True, weights, None, None)[0]
            loss, normal = torch.ops.evogp_hip.tree_SR_weighted_normal_eq(*self._shape(inputs), value, ntype, size, inputs, labels, w)
        K = LM_MAX_CONSTS
        T = K * (K + 1) // 2
        A, b = _symmetric(normal[:, :T], K), normal[:, T:].clone()
        L = self.max_tree_len
        pos = torch.arange(L, device=value.device)[None, :]
        is_c = (ntype == NType.CONST) & (pos < size[:, :1].clamp(0, L))
        first = torch.where(is_c, pos, L).sort(dim=1).values[:, :K]
        const_index = torch.where(first < L, first, -1)
        if L < K:
            const_index = torch.nn.functional.pad(const_index, (0, K - L), value=-1)
        return loss, A, b, const_index

    # ---- structural duplicates ---------------------------------------------------------------
    def structure_hash(self) -> Tensor:
        """(pop,) int64: the bits of a 64-bit hash of every tree's live prefix (node values by bit pattern, node types, length;
        include/evogp_hip.h evogp_hip_tree_hash).  Equal trees have equal hashes; a row whose length is out of range has hash 0."""
        return torch.ops.evogp_hip.tree_hash(*self._tensors())

    def duplicate_classes(self):
        """``(class_id, is_first)``: ``class_id`` (pop,) int32 is the smallest index of a tree equal to tree t -- same length and, over
        the live prefix, the same value bits, type words and subtree sizes (so -0.0 differs from 0.0 and tail words do not count); a
        row whose length is out of range is a class of its own.  ``is_first`` (pop,) bool marks the representatives
        (``class_id[t] == t``).  Exact: hashes only choose which rows are compared.  No host synchronisation."""
        value, ntype, size = self._tensors()
        class_id = torch.ops.evogp_hip.tree_classes(value, ntype, size, torch.ops.evogp_hip.tree_hash(value, ntype, size))
        return class_id, class_id == torch.arange(self.pop_size, dtype=torch.int32, device=class_id.device)

    def unique(self):
        """``(forest, inverse, counts)``, shaped like ``torch.unique``: the representatives of ``duplicate_classes`` in ascending index
        order as a Forest, ``inverse`` (pop,) int64 with ``forest[inverse[t]]`` equal to tree t on its live prefix, and ``counts``
        (int64) the number of trees per representative.  ONE host synchronisation (the number of representatives sizes the result)."""
        return self._unique(*self.duplicate_classes())

    def _unique(self, class_id: Tensor, is_rep: Tensor):
        rank = torch.cumsum(is_rep.to(torch.int64), 0) - 1
        inverse = rank[class_id.to(torch.int64)]
        reps = torch.nonzero(is_rep).squeeze(1)   # (the host sync)
        return self[reps], inverse, torch.bincount(inverse, minlength=reps.numel())

    def _first_rows_only(self):
        """``(forest, class_id)``: this forest with every row that is not the first of its class made an EMPTY tree (length 0; the
        subtree-size tensor is the only one copied), which every tape kernel classifies as malformed and leaves at once"""
        class_id, is_first = self.duplicate_classes()
        value, ntype, size = self._tensors()
        size = size.clone()
        size[:, 0] = torch.where(is_first, size[:, 0], torch.zeros_like(size[:, 0]))
        return Forest(self.input_len, self.output_len, value, ntype, size, func_mask=self.func_mask), class_id.to(torch.int64)

    def _once_per_class(self, dedup: bool):
        """``(forest, gather)`` for a dataset pass that honours ``dedup``: the forest to run the pass on and the function that hands
        every row of a result its own entry -- ``_first_rows_only`` and ``t -> t[class_id]``, or this forest and the identity"""
        if not dedup:
            return self, lambda t: t
        firsts, class_id = self._first_rows_only()
        return firsts, lambda t: t[class_id]

    def optimize_constants(self, inputs: Tensor, labels: Tensor, steps: int = 10, step_size: float = 0.1, use_MSE: bool = True,
                           method: str = "descent", damping: float = 1e-3, dedup: bool = False, weights: Optional[Tensor] = None,
                           loss: Optional[str] = None, param: Optional[float] = None):
        """``(forest, loss)``: ``steps`` iterations of a per-tree optimisation of the constants, all on the device with no host
        synchronisation (2 launches per step).  Returns a new Forest (this one is untouched) whose trees differ from these only in
        constant values, and the loss of each returned tree.  No tree's loss rises.

        ``method="descent"``: gradient descent ("bold driver": a step of length h along -grad / |grad|, h starting at ``step_size``, is
        kept only if it lowers the tree's loss, and h then doubles; otherwise h halves).  ``method="lm"`` (MSE, single-output forests):
        Levenberg-Marquardt on the tree's first 8 constants in prefix order (further constants keep their values): the step solves
        ``(A + lambda diag A) delta = -b`` on the normal equations of ``SR_normal_equations`` and is kept only if it lowers the loss;
        lambda starts at ``damping``, falls tenfold after a kept step and rises tenfold after a rejected one.  A model that is linear
        in its constants is solved in one to three steps.

        ``dedup=True``: the same result, bit for bit, with the dataset passes run once per DISTINCT tree (``duplicate_classes``): the
        launches see the other rows as empty trees, and every row then takes the tuned constants and the loss of its class's first
        row.  No host synchronisation is added.

        ``weights``, ``loss``, ``param`` (those of ``SR_gradient``; single-output forests): the loss that is minimised, and returned,
        is ``sum_d w_d rho(tree(x_d) - y_d) / sum_d w_d`` -- sample weights, a robust loss, or a 0/1 row that keeps held-out rows away
        from the tuner (a row of weight 0 is not looked at).  ``method="lm"`` takes weights and no loss but ``"mse"``.  A tree whose loss
        is NaN (``SR_gradient`` says when) keeps its constants.  With all three left at None the call is the unweighted one."""
        assert steps >= 0, f"steps should be >= 0, but got {steps}"
        if method not in ("descent", "lm"):
            raise ValueError(f"method should be 'descent' or 'lm', but got {method!r}")
        if method == "lm" and loss not in (None, "mse"):
            raise ValueError(f"method='lm' minimises the (weighted) mean squared error, but got loss={loss!r}")
        if method == "lm":
            if not use_MSE:
                raise ValueError("method='lm' minimises the mean squared error: use_MSE must be True")
            self._single_output("method='lm'", ValueError)
        inputs, labels = self._sr_data(inputs, labels)
        own = self._tuning_loss("optimize_constants", inputs, use_MSE, weights, loss, param)
        source, gather = self._once_per_class(dedup)
        shape, hip = self._shape(inputs), torch.ops.evogp_hip
        if method == "lm":   # the model is the packed normal equations, the per-tree scalar is lambda
            if own is None:
                evaluate = lambda *tree: hip.tree_SR_normal_eq(*shape, *tree, inputs, labels)
            else:
                evaluate = lambda *tree: hip.tree_SR_weighted_normal_eq(*shape, *tree, inputs, labels, own[0])
            value, loss = source._tune(steps, damping, evaluate, hip.tree_SR_lm_step)
        else:                # the model is the gradient, the per-tree scalar is the step length
            if own is None:
                evaluate = lambda *tree: hip.tree_SR_gradient(*shape, use_MSE, *tree, inputs, labels)
            else:
                evaluate = lambda *tree: hip.tree_SR_weighted_gradient(*shape, *tree, inputs, labels, *own)
            value, loss = source._tune(steps, step_size, evaluate, lambda phase, *rest: hip.tree_SR_const_step(phase, self.output_len, *rest))
        if dedup:   # constants live in the prefix, which the rows of a class share; every row keeps its own tail words
            live = torch.arange(self.max_tree_len, device=value.device)[None, :] < self.batch_subtree_size[:, :1]
            value = torch.where(live, gather(value), value)
        forest = Forest(self.input_len, self.output_len, value, self.batch_node_type.clone(), self.batch_subtree_size.clone(),
                        func_mask=self.func_mask)
        return forest, gather(loss)

    def _tune(self, steps: int, start: float, evaluate, propose):
        """``(value, loss)``: the accept/reject loop of both optimisers on a copy of the node values.  ``evaluate(value, ntype, size)``
        is the dataset pass, ``(loss, model)``; ``propose(phase, value, ntype, size, cand, loss, model, loss_c, model_c, scalar)`` is
        the step op: phase 2 writes the first candidate, phase 3 accepts or rejects one and writes the next, phase 1 only accepts or
        rejects.  ``scalar`` (pop,) starts at ``start``."""
        value, ntype, size = self._tensors()
        value = value.clone()
        loss, model = evaluate(value, ntype, size)
        if steps > 0:
            cand = torch.empty_like(value)
            scalar = torch.full((self.pop_size,), float(start), dtype=torch.float32, device=value.device)
            propose(2, value, ntype, size, cand, loss, model, loss, model, scalar)
            for k in range(steps):
                loss_c, model_c = evaluate(cand, ntype, size)
                propose(3 if k + 1 < steps else 1, value, ntype, size, cand, loss, model, loss_c, model_c, scalar)
        return value, loss

    # ---- semantic duplicates -------------------------------------------------------------------
    def _semantic_rows(self, what: str, inputs: Tensor) -> Tensor:
        self._single_output(what, ValueError)
        inputs = check_tensor(inputs, self.batch_node_value.device)
        if inputs.dim() != 2 or inputs.shape[0] < 1 or inputs.shape[1] != self.input_len:
            raise ValueError(f"inputs shape should be (D, {self.input_len}) with D >= 1, but got {tuple(inputs.shape)}")
        return inputs.contiguous().to(torch.float32)

    def semantic_hash(self, inputs: Tensor) -> Tensor:
        """(pop,) int64: the bits of a 64-bit signature of every tree's float32 predictions on the rows of ``inputs`` ``(D, input_len)``
        -- ``batch_forward``'s bits with -0.0 taken as +0.0 and every NaN as one (csrc/sr_semantic.hip, include/evogp_hip.h
        evogp_hip_sr_semantic_hash).  Trees that predict the same on every row have equal signatures; a malformed row has 0.  The
        predictions are never stored.  Deterministic, no host synchronisation; single-output forests (``ValueError`` otherwise)."""
        inputs = self._semantic_rows("semantic_hash", inputs)
        return torch.ops.evogp_hip.tree_SR_semantic_hash(*self._shape(inputs), *self._tensors(), inputs)

    def semantic_classes(self, inputs: Tensor, keep: str = "first"):
        """``(class_id, is_representative)``: two well-formed trees are in one class when their predictions on ``inputs`` agree on every
        row (``+0.0 == -0.0``, NaN equals NaN, everything else by bits), whatever they look like: ``x0 + x1`` and ``x1 + x0``,
        ``x0 * 1`` and ``x0``, any two trees that are NaN everywhere.  A malformed row is a class of its own.  ``class_id`` (pop,) int32
        names the representative of tree t's class, ``is_representative`` (pop,) bool marks the representatives.  ``keep="first"``: the
        member of smallest index; ``keep="smallest"``: the member with the fewest nodes, ties to the smallest index.  Exact: the
        signatures of ``semantic_hash`` only choose which trees are compared.  No host synchronisation."""
        if keep not in ("first", "smallest"):
            raise ValueError(f"keep should be 'first' or 'smallest', but got {keep!r}")
        inputs = self._semantic_rows("semantic_classes", inputs)
        shape, tensors = self._shape(inputs), self._tensors()
        sig = torch.ops.evogp_hip.tree_SR_semantic_hash(*shape, *tensors, inputs)
        class_id = torch.ops.evogp_hip.tree_SR_semantic_classes(*shape, *tensors, inputs, sig)
        index = torch.arange(self.pop_size, dtype=torch.int64, device=class_id.device)
        if keep == "smallest":
            # per first-index class the minimum of size * pop + index: integers, exact, and the order of the scatter does not matter
            first = class_id.to(torch.int64)
            word = tensors[2][:, 0].to(torch.int64).clamp(0, self.max_tree_len) * self.pop_size + index
            best = torch.full_like(word, torch.iinfo(torch.int64).max).scatter_reduce(0, first, word, "amin", include_self=True)
            class_id = (best[first] % self.pop_size).to(torch.int32)
        return class_id, class_id.to(torch.int64) == index

    def semantic_unique(self, inputs: Tensor, keep: str = "first"):
        """``(forest, inverse, counts)``, shaped like ``unique``: the representatives of ``semantic_classes(inputs, keep)`` in ascending
        index order as a Forest, ``inverse`` (pop,) int64 with ``forest[inverse[t]]`` predicting what tree t predicts on every row, and
        ``counts`` (int64) the number of trees per representative.  ONE host synchronisation."""
        return self._unique(*self.semantic_classes(inputs, keep))

    # ---- pairwise semantic moments -------------------------------------------------------------
    def SR_pair_moments(self, inputs: Tensor, labels: Optional[Tensor], first: Tensor, candidates: Tensor, mates: Optional["Forest"] = None):
        """``(own, moments)``: how far apart pairs of trees are on a dataset, and what combining them gives (csrc/sr_pair.hip,
        include/evogp_hip.h evogp_hip_sr_pair_moments).  Event e pairs tree ``first[e]`` of this forest with the trees
        ``candidates[e, m]`` of ``mates`` (a single-output Forest of the same ``input_len``, any ``max_tree_len``; None: this forest),
        ``M <= 16``.  With ``r_t = (double)p_t - (double)y`` over the float32 predictions of ``batch_forward`` (``labels=None``: y = 0):
        ``own[e] = sum r_a^2`` float64 ``(E,)``, ``moments[e, m] = (sum r_b^2, sum r_a r_b, sum (p_a - p_b)^2)`` float64 ``(E, M, 3)``.
        ``candidates`` of shape ``(E,)`` is read as ``(E, 1)`` and ``moments`` then comes back as ``(E, 3)``.  A malformed tree, a tree
        with a prediction that is not finite, or an index outside its forest is unusable: an unusable first tree makes ``own[e]`` and
        ``moments[e]`` NaN, an unusable candidate its three words.  The words of a pair depend on its two trees and the dataset alone,
        bit for bit.  No (pop, D) array, no host synchronisation; ``ValueError`` for a multi-output forest on either side, another
        ``input_len``, ``M`` outside 1 .. 16 or a shape mismatch, before anything is launched."""
        inputs = self._semantic_rows("SR_pair_moments", inputs)
        other = self if mates is None else mates
        if not isinstance(other, Forest) or other.output_len != 1 or other.input_len != self.input_len:
            raise ValueError(f"SR_pair_moments: mates should be a single-output Forest with {self.input_len} inputs, but got "
                             f"{type(other).__name__} with {getattr(other, 'input_len', '?')} inputs and {getattr(other, 'output_len', '?')} outputs")
        device = self.batch_node_value.device
        if labels is not None:
            labels = check_tensor(labels, device)
            if labels.dim() == 2 and labels.shape[1] == 1:
                labels = labels[:, 0]
            if labels.shape != (inputs.shape[0],):
                raise ValueError(f"labels shape should be ({inputs.shape[0]},) or ({inputs.shape[0]}, 1), but got {tuple(labels.shape)}")
            labels = labels.contiguous().to(torch.float32)
        first, candidates = (check_tensor(t, device) for t in (first, candidates))
        for name, t in (("first", first), ("candidates", candidates)):
            if t.dtype.is_floating_point or t.dtype == torch.bool:
                raise ValueError(f"{name} should hold integers, but got {t.dtype}")
        if first.dim() != 1:
            raise ValueError(f"first shape should be (E,), but got {tuple(first.shape)}")
        flat = candidates.dim() == 1
        if flat:
            candidates = candidates[:, None]
        if candidates.dim() != 2 or candidates.shape[0] != first.shape[0]:
            raise ValueError(f"candidates shape should be ({first.shape[0]},) or ({first.shape[0]}, M), but got {tuple(candidates.shape)}")
        if not 1 <= candidates.shape[1] <= PAIR_MAX_CANDIDATES:
            raise ValueError(f"SR_pair_moments takes 1 to {PAIR_MAX_CANDIDATES} candidates per event, but got {candidates.shape[1]}")
        own, moments = torch.ops.evogp_hip.tree_SR_pair_moments(*self._tensors(), *other._tensors(), inputs, labels,
                                                                first.to(torch.int32).contiguous(), candidates.to(torch.int32).contiguous())
        return own, (moments[:, 0] if flat else moments)

    def semantic_distance(self, inputs: Tensor, first: Tensor, second: Tensor, mates: Optional["Forest"] = None) -> Tensor:
        """(E,) float64: the Euclidean distance between the float32 prediction vectors of tree ``first[e]`` of this forest and tree
        ``second[e]`` of ``mates`` (None: this forest) on the rows of ``inputs``: ``sqrt(SR_pair_moments(...)[1][:, 2])``.  NaN where
        either tree is unusable.  No host synchronisation."""
        second = check_tensor(second, self.batch_node_value.device)
        if second.dim() != 1:
            raise ValueError(f"second shape should be (E,), but got {tuple(second.shape)}")
        return torch.sqrt(self.SR_pair_moments(inputs, None, first, second, mates)[1][:, 2])

    # ---- subtree signatures and the population-built library ------------------------------------
    def SR_subtree_signatures(self, inputs: Tensor) -> Tensor:
        """(pop, max_tree_len) int64: ``semantic_hash``'s signature of EVERY SUBTREE on the rows of ``inputs`` ``(D, input_len)``.  Entry
        ``[t, i]`` is the word ``semantic_hash`` gives the row that holds the nodes ``[i, i + size[t, i])`` alone, so column 0 is
        ``semantic_hash(inputs)`` and two subtrees anywhere in the forest that take the same values on every row carry one word.  0 on
        the tail of a row and on malformed trees.  One forward walk per tree (csrc/sr_subtree_sig.hip); deterministic, no host
        synchronisation; single-output forests (``ValueError`` otherwise)."""
        inputs = self._semantic_rows("SR_subtree_signatures", inputs)
        return torch.ops.evogp_hip.tree_SR_subtree_signatures(*self._shape(inputs), *self._tensors(), inputs)

    def subtree_library(self, inputs: Tensor, k: int = BACKPROP_MAX_LIBRARY, min_size: int = 1, max_size: Optional[int] = None,
                        sig: Optional[Tensor] = None):
        """``(library, counts, tree, node)``: the semantically distinct subtrees of this forest on ``inputs``, the most frequent first.
        The subtrees of ``min_size <= size <= max_size`` nodes (``max_size=None``: any) fall into classes of equal signature
        (``SR_subtree_signatures``); a class is represented by its member of fewest nodes (ties: the smallest tree index, then node
        index), and the classes are ordered by (members descending, representative ascending).  ``library`` is a Forest of the first
        ``m = min(k, classes)`` representatives at this forest's ``max_tree_len``: row j holds the nodes ``[node[j], node[j] + size)`` of
        tree ``tree[j]`` word for word from position 0, zeros behind them, and carries this forest's ``func_mask``.  ``counts`` (m,) int32:
        the members per class; ``tree``, ``node`` (m,) int64.  Signatures alone decide a class: a collision of two 64-bit words merges two
        semantics and costs one member, so compute the library's semantics from ``library`` itself.  ONE host synchronisation (to read
        m); ``ValueError`` for a multi-output forest, ``k`` outside 1 .. 1024 or sizes with ``1 <= min_size <= max_size`` violated.
        ``sig``: ``SR_subtree_signatures(inputs)`` when the caller already has it (``remove_introns`` takes the same), None to compute it."""
        inputs = self._semantic_rows("subtree_library", inputs)
        L = self.max_tree_len
        max_size = L if max_size is None else max_size
        for name, v in (("k", k), ("min_size", min_size), ("max_size", max_size)):
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"{name} should be an integer, but got {v!r}")
        if not 1 <= k <= BACKPROP_MAX_LIBRARY:
            raise ValueError(f"k should be in [1, {BACKPROP_MAX_LIBRARY}], but got {k}")
        if min_size < 1 or max_size < min_size:
            raise ValueError(f"sizes should satisfy 1 <= min_size <= max_size, but got min_size {min_size} and max_size {max_size}")
        if self.pop_size * L >= 2 ** 31:
            raise ValueError(f"subtree_library takes forests of fewer than 2^31 words, but got {self.pop_size} x {L}")
        value, ntype, size = self._tensors()
        if sig is None:
            sig = torch.ops.evogp_hip.tree_SR_subtree_signatures(*self._shape(inputs), value, ntype, size, inputs)
        elif not isinstance(sig, Tensor) or sig.dtype != torch.int64 or tuple(sig.shape) != (self.pop_size, L):
            raise ValueError(f"sig should be the int64 ({self.pop_size}, {L}) tensor of SR_subtree_signatures")
        member, counts, n_classes = torch.ops.evogp_hip.subtree_library_select(sig, size, min_size, min(max_size, L), k)
        m = min(k, int(n_classes.item()))   # (the host sync)
        flat = member[:m].to(torch.int64)
        tree, node = flat // L, flat % L
        cols = torch.arange(L, device=value.device)[None, :]
        live = cols < size[tree, node].to(torch.int64)[:, None]
        src = (node[:, None] + cols).clamp(max=L - 1)
        rows = tuple(torch.where(live, a[tree[:, None], src], torch.zeros((), dtype=a.dtype, device=a.device)) for a in (value, ntype, size))
        return Forest(self.input_len, 1, *rows, func_mask=self.func_mask), counts[:m], tree, node

    # ---- exact semantic intron removal -----------------------------------------------------------
    def SR_subtree_introns(self, inputs: Tensor, sig: Optional[Tensor] = None) -> Tensor:
        """(pop, max_tree_len) int16 ``rep``: ``rep[t, i]`` is the descendant of node i whose subtree takes the value of the subtree at i
        on EVERY row of ``inputs`` ``(D, input_len)`` -- equal float32 bit patterns, or both NaN; ``+0.0`` and ``-0.0`` are different -- or
        i itself: the node computes nothing (``x + 0``, ``1 * x``, ``max(x, x)``, ``neg(neg(x))``, ``IF(c, a, a)``, ``(x * 2) / 2``, ...).
        Among the equal descendants the signatures name the one of fewest nodes (then least index); the tape then verifies that one on
        every row, so ``rep`` never names an unequal node, whatever ``sig`` holds.  ``sig``: ``SR_subtree_signatures(inputs)`` when the
        caller already has it (the library refresh computes it too), None to compute it here.  i on the tail and on malformed rows.
        Two walks per tree with ``sig=None``, one otherwise (csrc/sr_introns.hip); deterministic, no host synchronisation;
        single-output forests (``ValueError`` otherwise)."""
        inputs = self._semantic_rows("SR_subtree_introns", inputs)
        shape, tensors = self._shape(inputs), self._tensors()
        if sig is None:
            sig = torch.ops.evogp_hip.tree_SR_subtree_signatures(*shape, *tensors, inputs)
        elif not isinstance(sig, Tensor) or sig.dtype != torch.int64 or tuple(sig.shape) != (self.pop_size, self.max_tree_len):
            raise ValueError(f"sig should be the int64 ({self.pop_size}, {self.max_tree_len}) tensor of SR_subtree_signatures")
        return torch.ops.evogp_hip.tree_SR_subtree_introns(*shape, *tensors, inputs, sig.contiguous())

    def remove_introns(self, inputs: Tensor, sig: Optional[Tensor] = None, dedup: bool = False):
        """``(forest, removed)``: every tree without its semantic introns on ``inputs`` -- from the root down, a node becomes
        ``SR_subtree_introns``' ``rep`` of it -- and the number of nodes each tree lost (int32 ``(pop,)``).  The new tree's prediction has,
        on every row of ``inputs``, the bit pattern of the old one's (or both are NaN): every loss on these rows is unchanged.  A new
        Forest with this forest's ``func_mask`` (this one is untouched), zero tails, malformed rows copied.  Removing the introns of the
        result returns it unchanged unless a candidate that the verdict refused (``-0.0`` against ``+0.0``, a collision) was itself
        dropped by the rewrite: the node then meets its next candidate in a second pass.  ``sig`` as in ``SR_subtree_introns``.  No host synchronisation.

        ``dedup=True``: the same result, bit for bit, with the dataset passes run once per DISTINCT tree (``duplicate_classes``): the
        other rows enter them as empty trees and take the ``rep`` of their class's first row before the rewrite, which runs on every
        row.  A ``sig`` given with ``dedup=True`` is read on the first rows alone."""
        source, gather = self._once_per_class(dedup)
        rep = gather(source.SR_subtree_introns(inputs, sig))
        value, ntype, size, removed = torch.ops.evogp_hip.tree_remove_introns(*self._tensors(), rep.contiguous())
        # (a rewritten tree's functions are a subset of the old tree's)
        return Forest(self.input_len, self.output_len, value, ntype, size, func_mask=self.func_mask), removed

    def SR_subtree_errors(self, inputs: Tensor, labels: Tensor, use_MSE: bool = True):
        """``(node_err, node_const)``, both (pop, max_tree_len): ``node_err[t, i]`` is the loss the subtree rooted at node i of tree t
        would have as a model of its own (what ``SR_fitness`` returns for it as a row of its own; ``node_err[:, 0]`` is the tree's
        loss), ``node_const[t, i]`` is the value of that subtree when it has one and the same float32 bit pattern on every row of
        ``inputs`` and NaN otherwise (a NaN is never "constant").  Tail entries and malformed trees are NaN.  One forward pass per
        tree over every row (csrc/sr_subtree.hip); single-output forests only."""
        self._single_output("SR_subtree_errors")
        inputs, labels = self._sr_data(inputs, labels)
        return torch.ops.evogp_hip.tree_SR_subtree_errors(*self._shape(inputs), use_MSE, *self._tensors(), inputs, labels)

    def simplify(self, inputs: Tensor, labels: Tensor, use_MSE: bool = True, hoist: bool = True, fold_constants: bool = True,
                 dedup: bool = False, introns: bool = False):
        """``(forest, loss)``: every tree rewritten into a tree that is no larger and, on this dataset, no worse, in two launches with
        no host synchronisation.  ``hoist``: the tree becomes its subtree of least finite error (then least size, then least index),
        so a tree that is NaN as a whole but has a finite subtree is rescued.  ``fold_constants``: every function node whose subtree
        takes one finite float32 value on every row becomes a CONST node of that value (the outermost such node wins); the rewritten
        tree computes bit-identical values on every row of ``inputs``.  Returns a new Forest (this one is untouched) and the loss of
        each returned tree (``node_err`` at the chosen root).  Simplifying the result again returns it unchanged.

        ``dedup=True``: the same result, bit for bit, with the pass over the dataset run once per DISTINCT tree
        (``duplicate_classes``): the other rows enter it as empty trees and take the subtree errors of their class's first row before
        the rewrite, which runs on every row.  No host synchronisation is added.

        ``introns=True``: the forest after hoist and fold then goes through ``remove_introns(inputs)``: nodes that take the value of one
        of their descendants on every row leave.  The predictions keep their bits, so the returned loss is the one above."""
        self._single_output("simplify")
        inputs, labels = self._sr_data(inputs, labels)
        value, ntype, size = self._tensors()
        source, gather = self._once_per_class(dedup)
        node_err, node_const = torch.ops.evogp_hip.tree_SR_subtree_errors(*self._shape(inputs), use_MSE, *source._tensors(), inputs, labels)
        value, ntype, size, _, loss = torch.ops.evogp_hip.tree_prune(self.output_len, bool(hoist), bool(fold_constants), value, ntype, size,
                                                                     gather(node_err), gather(node_const))
        # (a rewritten tree's functions are a subset of the old tree's)
        forest = Forest(self.input_len, self.output_len, value, ntype, size, func_mask=self.func_mask)
        if introns:
            forest = forest.remove_introns(inputs, dedup=dedup)[0]
        return forest, loss

    # ---- linear scaling ------------------------------------------------------------------------
    def SR_scaled_fitness(self, inputs: Tensor, labels: Tensor, dedup: bool = False):
        """``(loss, slope, intercept)``, each (pop,) float32: the mean squared error of ``intercept + slope * tree(x)`` with the
        least-squares coefficients of every tree (linear scaling, Keijzer 2003), from three float64 sums per tree taken inside the
        evaluation kernel (csrc/sr_scale.hip): the ``(pop, D)`` predictions are never stored.  A tree that is constant over the rows
        (decided exactly, on the minimum and maximum prediction) gets slope 0, intercept mean(y) and the variance of the labels; a
        malformed tree or one with a non-finite prediction gets NaN in all three.  Deterministic from run to run, no host
        synchronisation; single-output forests, MSE only.

        ``dedup=True``: the same bits with the pass run once per DISTINCT tree (``duplicate_classes``), the other rows entering it
        as empty trees and taking the result of their class's first row."""
        self._single_output("SR_scaled_fitness")
        inputs, labels = self._sr_data(inputs, labels)
        source, gather = self._once_per_class(dedup)
        loss, coef = torch.ops.evogp_hip.tree_SR_linear_scaling(*self._shape(inputs), *source._tensors(), inputs, labels)
        loss, coef = gather(loss), gather(coef)
        return loss, coef[:, 1], coef[:, 0]

    def apply_scaling(self, slope: Tensor, intercept: Tensor, grow: bool = False):
        """``(forest, applied)``: every tree T rewritten as ``ADD(MUL(T, slope), intercept)`` -- four more nodes -- so that the tree
        itself computes the scaled model (``fl(fl(T * slope) + intercept)`` in float32).  ``applied`` (pop,) bool is False for the rows
        left as they were: the wrapped tree does not fit the row, a coefficient is not finite, or the tree is malformed.
        ``grow=True``: the result has ``max_tree_len = min(L + 4, 1024)``, so every finite tree of a forest with ``L <= 1020`` fits.
        One launch, no host synchronisation; single-output forests only."""
        self._single_output("apply_scaling")
        dev = self.batch_node_value.device
        slope, intercept = check_tensor(slope, dev), check_tensor(intercept, dev)
        assert slope.shape == (self.pop_size,) and intercept.shape == (self.pop_size,), (
            f"slope and intercept shapes should be ({self.pop_size}, ), but got {tuple(slope.shape)} and {tuple(intercept.shape)}")
        coef = torch.stack([intercept.to(torch.float32), slope.to(torch.float32)], dim=1).contiguous()
        out_len = min(self.max_tree_len + 4, _utils.MAX_STACK) if grow else self.max_tree_len
        value, ntype, size, applied = torch.ops.evogp_hip.tree_wrap_linear(out_len, *self._tensors(), coef)
        mask = self.func_mask
        return (Forest(self.input_len, self.output_len, value, ntype, size, func_mask=(mask | _WRAP_FUNCS) if mask else 0),
                applied.to(torch.bool))

    # ---- weighted, robust and held-out losses -----------------------------------------------------
    def _weight_rows(self, inputs: Tensor, labels: Tensor, weights: Optional[Tensor]):
        """``(inputs, labels, weights, flat)`` as the weighted passes take them: float32 ``(D, input_len)``, ``(D, 1)`` and ``(K, D)`` or
        None on the forest's device; ``flat``: no weights or one ``(D,)`` row, the result has no column axis.  ``ValueError`` for a shape
        or a dtype"""
        dev = self.batch_node_value.device
        inputs, labels = check_tensor(inputs, dev), check_tensor(labels, dev)
        n = inputs.shape[0]
        if inputs.shape != (n, self.input_len):
            raise ValueError(f"inputs shape should be ({n}, {self.input_len}), but got {tuple(inputs.shape)}")
        if labels.shape != (n, 1):
            raise ValueError(f"labels shape should be ({n}, 1), but got {tuple(labels.shape)}")
        inputs, labels = inputs.contiguous().to(torch.float32), labels.contiguous().to(torch.float32)
        flat = True
        if weights is not None:
            weights = check_tensor(weights, dev)
            flat = weights.dim() == 1
            if not weights.dtype.is_floating_point:
                raise ValueError(f"weights should be a floating-point tensor, but got {weights.dtype}")
            if weights.dim() not in (1, 2) or weights.shape[-1] != n or (weights.dim() == 2 and not 1 <= weights.shape[0] <= WLOSS_MAX_WEIGHTS):
                raise ValueError(f"weights shape should be ({n},) or (K, {n}) with 1 <= K <= {WLOSS_MAX_WEIGHTS}, but got {tuple(weights.shape)}")
            weights = weights.reshape(-1, n).contiguous().to(torch.float32)
        return inputs, labels, weights, flat

    def SR_weighted_loss(self, inputs: Tensor, labels: Tensor, weights: Optional[Tensor] = None, loss: str = "mse",
                         param: Optional[float] = None, dedup: bool = False) -> Tensor:
        """``(sum_d W[k, d] * rho(tree(x_d) - y_d)) / sum_d W[k, d]`` of every tree, float32, taken inside the evaluation kernel in one
        pass (csrc/sr_wloss.hip): the ``(pop, D)`` predictions are never stored.  ``weights``: None (every weight 1) or ``(D,)`` gives
        ``(pop,)``; ``(K, D)`` with ``1 <= K <= 8`` gives ``(pop, K)``, one column per weight row -- sample weights, a training and a
        validation row of 0/1 masks, K folds -- for one interpretation of the trees.  ``loss``: ``"mse"``, ``"mae"``, ``"huber"``
        (``param`` = delta > 0), ``"pinball"`` (``param`` = tau in (0, 1): the fit sits at the tau-quantile) or ``"logcosh"``; rho is
        evaluated in float64 on the float32 predictions of ``batch_forward``.

        A row with weight exactly 0 is not looked at in that column: the tree may be NaN or infinite there.  A column is NaN where a
        row WITH weight has a non-finite prediction or the tree is malformed, and for every tree when its weight row holds a negative
        or non-finite weight or sums to 0 (decided on the device: include/evogp_hip.h has the rules).  A column depends on its own
        weight row only.  Deterministic from run to run, no host synchronisation; single-output forests.

        ``dedup=True``: the same bits with the pass run once per DISTINCT tree (``duplicate_classes``)."""
        self._single_output("SR_weighted_loss", ValueError)
        param = check_loss(loss, param)
        inputs, labels, weights, flat = self._weight_rows(inputs, labels, weights)
        source, gather = self._once_per_class(dedup)
        out = gather(torch.ops.evogp_hip.tree_SR_weighted_loss(*self._shape(inputs), *source._tensors(), inputs, labels, weights,
                                                               LOSS_KINDS[loss], 0.0 if param is None else param))
        return out[:, 0] if flat else out

    # ---- linear scaling under sample weights, scored on held-out rows ------------------------------
    def SR_weighted_scaled_fitness(self, inputs: Tensor, labels: Tensor, weights: Optional[Tensor] = None, dedup: bool = False):
        """``(loss, slope, intercept)``: linear scaling (``SR_scaled_fitness``) fitted under sample weights and scored on up to 8
        weight rows in ONE interpretation of the trees (csrc/sr_wscale.hip); the ``(pop, D)`` predictions are never stored.
        ``weights``: None (every weight 1) or ``(D,)`` gives a ``(pop,)`` loss; ``(K, D)`` with ``1 <= K <= 8`` gives ``(pop, K)``.
        **Row 0 is the fit row**: ``intercept + slope * tree(x)`` is the weighted least-squares fit on it, in closed form, float64.
        Every row k, row 0 included, is then scored with those coefficients:
        ``loss[:, k] = sum_d W[k, d] (intercept + slope * tree(x_d) - y_d)^2 / sum_d W[k, d]`` -- a training row and a validation row
        of 0/1 masks give the held-out error of the model fitted WITHOUT the held-out rows.  ``slope`` and ``intercept`` are ``(pop,)``.

        A tree that is constant over the rows row 0 weights (decided exactly, on the minimum and maximum prediction), or that has one
        such row only, gets slope 0 and the weighted mean of the labels.  A data row with weight exactly 0 in a weight row is not looked
        at there: the tree may be NaN or infinite on it.  Column k is NaN where a data row WITH weight in row k has a non-finite
        prediction; if that is row 0, so are the coefficients and every column.  A malformed tree is NaN everywhere.  A weight row with
        a negative or non-finite weight or a sum of 0 gives NaN: everywhere when it is row 0, in its own column otherwise (decided on
        the device: include/evogp_hip.h has the rules).  Multiplying a weight row by a power of two changes no bit.  A column depends on
        row 0 and its own row only.  Deterministic from run to run, no host synchronisation; single-output forests, squared error.

        ``dedup=True``: the same bits with the pass run once per DISTINCT tree (``duplicate_classes``)."""
        self._single_output("SR_weighted_scaled_fitness", ValueError)
        inputs, labels, weights, flat = self._weight_rows(inputs, labels, weights)
        source, gather = self._once_per_class(dedup)
        loss, coef = torch.ops.evogp_hip.tree_SR_weighted_scaling(*self._shape(inputs), *source._tensors(), inputs, labels, weights)
        loss, coef = gather(loss), gather(coef)
        return (loss[:, 0] if flat else loss), coef[:, 1], coef[:, 0]

    # ---- multi-gene fitness ----------------------------------------------------------------------
    def _gene_data(self, what: str, inputs: Tensor, labels: Tensor):
        if not 1 <= self.output_len <= GENES_MAX:
            raise ValueError(f"{what} works on forests of 1 .. {GENES_MAX} outputs, but output_len is {self.output_len}")
        inputs, labels = check_tensor(inputs, self.batch_node_value.device), check_tensor(labels, self.batch_node_value.device)
        n = inputs.shape[0]
        if inputs.shape != (n, self.input_len):
            raise ValueError(f"inputs shape should be ({n}, {self.input_len}), but got {tuple(inputs.shape)}")
        if labels.shape not in ((n,), (n, 1)):
            raise ValueError(f"{what} fits ONE label column: labels shape should be ({n},) or ({n}, 1), but got {tuple(labels.shape)}")
        return inputs.contiguous().to(torch.float32), labels.contiguous().to(torch.float32)

    def SR_gene_fitness(self, inputs: Tensor, labels: Tensor, dedup: bool = False):
        """``(loss (pop,), coef (pop, 1 + G))``, float32: multi-gene regression (GPTIPS; Arnaldo et al. 2014).  The ``G = output_len``
        outputs of a tree are features ``g_1 .. g_G`` and the model is ``coef[0] + sum_j coef[1 + j] * g_j(x)`` with the least-squares
        coefficients of every tree; ``loss`` is its mean squared error on ONE label column, ``(D,)`` or ``(D, 1)``.  The float64
        co-moments are taken inside the evaluation kernel in one pass (csrc/sr_genes.hip): the ``(pop, D, G)`` outputs are never
        stored.  A gene that is constant over the rows, or collinear with the genes in front of it up to float32 rounding (LDL^T
        pivot below 2^-30 of its variance), gets weight exactly 0; a malformed tree or one with a non-finite gene value gets NaN
        throughout (include/evogp_hip.h has the full definition).  ``1 <= G <= 8``.  Deterministic, no host synchronisation.

        ``dedup=True``: the same bits with the pass run once per DISTINCT tree (``duplicate_classes``)."""
        inputs, labels = self._gene_data("SR_gene_fitness", inputs, labels)
        source, gather = self._once_per_class(dedup)
        loss, coef = torch.ops.evogp_hip.tree_SR_gene_fitness(*self._shape(inputs), *source._tensors(), inputs, labels)
        return gather(loss), gather(coef)

    def SR_gene_moments(self, inputs: Tensor, labels: Tensor):
        """``(mean (pop, G), cov (pop, G, G), cov_y (pop, G))``, float64: the moments ``SR_gene_fitness`` solves from -- the mean of
        every gene, the covariance of the genes (the kernel's upper triangle, mirrored) and their covariance with the labels, all
        with divisor D.  A malformed tree has zeros."""
        inputs, labels = self._gene_data("SR_gene_moments", inputs, labels)
        _, _, m = torch.ops.evogp_hip.tree_SR_gene_moments(*self._shape(inputs), *self._tensors(), inputs, labels)
        G = self.output_len
        T = G * (G + 1) // 2
        return m[:, :G], _symmetric(m[:, G:G + T], G), m[:, G + T:]

    def gene_predict(self, inputs: Tensor, coef: Tensor) -> Tensor:
        """``(pop, D)`` float32: the multi-gene model ``coef[:, 0] + batch_forward(inputs) @ coef[:, 1:]`` in float32 torch.  This is
        the path that MATERIALISES the ``(pop, D, G)`` outputs: use it for a handful of trees, not for a population."""
        coef = check_tensor(coef, self.batch_node_value.device)
        if coef.shape != (self.pop_size, 1 + self.output_len):
            raise ValueError(f"coef shape should be ({self.pop_size}, {1 + self.output_len}), but got {tuple(coef.shape)}")
        coef = coef.to(torch.float32)
        genes = self.batch_forward(inputs)   # (pop, D, G)
        return coef[:, :1] + torch.einsum("pdg,pg->pd", genes, coef[:, 1:])

    # ---- interval arithmetic --------------------------------------------------------------------
    def _box(self, lower, upper):
        """the box as two float32 ``(input_len,)`` tensors on the forest's device, checked on the host"""
        dev = self.batch_node_value.device
        lower, upper = box_side(lower, self.input_len), box_side(upper, self.input_len)
        for name, b in (("lower", lower), ("upper", upper)):
            if b.shape[0] != self.input_len:
                raise ValueError(f"{name} should hold {self.input_len} bounds, but got {b.shape[0]}")
        if not bool(torch.isfinite(lower).all() and torch.isfinite(upper).all()):
            raise ValueError("the bounds of the box must be finite")
        if bool((lower > upper).any()):
            raise ValueError("lower must not exceed upper")
        return lower.contiguous().to(dev), upper.contiguous().to(dev)

    def SR_intervals(self, lower, upper):
        """``(lo, hi, flags)``, each (pop, max_tree_len): for every node of every tree a float32 interval and a flag byte that bound
        the float32 value its subtree takes on ANY input of the box ``lower[v] <= x[v] <= upper[v]`` -- not only on the rows of a
        dataset (interval arithmetic, Keijzer 2003; csrc/sr_interval.hip, one lane per tree, no dataset, no host synchronisation
        beyond the check of the bounds).  ``flags`` bit 0 (1): the value may be a NaN; bit 1 (2): the row is malformed (all its live
        nodes then hold NaN bounds).  Words past a tree's length are 0.  ``lower`` / ``upper``: floats or ``(input_len,)`` tensors,
        finite, ``lower <= upper`` (``ValueError`` otherwise); single-output forests only."""
        self._single_output("SR_intervals", ValueError)
        return torch.ops.evogp_hip.tree_intervals(*self._tensors(), *self._box(lower, upper))

    def safe_mask(self, lower, upper, max_abs: float = float("inf")) -> Tensor:
        """(pop,) bool: the tree is defined and bounded on the whole box -- its root can not be a NaN, both root bounds are finite and
        neither exceeds ``max_abs`` in magnitude (``SR_intervals``)"""
        return _root_safe(*self.SR_intervals(lower, upper), max_abs)

    # ---- derivative bounds --------------------------------------------------------------------
    def _wrt(self, wrt):
        """the requested variables as a host list of ints, checked"""
        if wrt is None:
            return list(range(self.input_len))
        idx = [wrt] if isinstance(wrt, int) else [int(v) for v in torch.as_tensor(wrt).reshape(-1).tolist()]
        if not idx:
            raise ValueError("wrt must name at least one variable")
        for v in idx:
            if not 0 <= v < self.input_len:
                raise ValueError(f"wrt holds variable {v}, but the trees have variables 0 .. {self.input_len - 1}")
        return idx

    def _derivative_op(self, what: str, lower, upper, idx):
        self._single_output(what, ValueError)
        lower, upper = self._box(lower, upper)
        wrt = torch.tensor(idx, dtype=torch.int32).to(self.batch_node_value.device)
        return torch.ops.evogp_hip.tree_derivative_intervals(*self._tensors(), lower, upper, wrt)

    def SR_derivative_intervals(self, lower, upper, wrt=None):
        """``(dlo, dhi, dflags)``, each (K, pop, max_tree_len): for every node of every tree and every variable ``wrt[k]`` (default: all
        of them; a repeated index gives equal slices) a float32 interval that bounds the partial derivative of its subtree in that
        variable at every real input of the box ``lower[v] <= x[v] <= upper[v]`` where the subtree is defined and differentiable
        (interval arithmetic over forward-mode derivatives, Kronberger et al. 2022; csrc/sr_deriv.hip, one lane per (tree, variable),
        no dataset, no host synchronisation beyond the checks).  ``dflags`` bit 0 (1): the subtree may be discontinuous in the
        variable; bit 1 (2): the row is malformed (NaN bounds); bit 2 (4): the variable occurs in a branch that can be taken (a
        subtree without it has exactly [0, 0]).  Where bit 0 is clear and the subtree is safe (``SR_intervals``), ``dlo >= 0`` proves
        it nondecreasing and ``dhi <= 0`` nonincreasing.  The box is checked as in ``SR_intervals``; ``ValueError`` for an index
        outside [0, input_len), an empty ``wrt`` or a multi-output forest."""
        return tuple(self._derivative_op("SR_derivative_intervals", lower, upper, self._wrt(wrt))[3:])

    def monotone_mask(self, lower, upper, constraints, max_abs: float = float("inf")) -> Tensor:
        """(pop,) bool: the tree is safe on the box (``safe_mask``'s rule on the enclosure of its real value) and obeys every
        constraint of ``{variable: +1 | -1 | (dmin, dmax)}``: the bounds of its partial derivative in that variable lie within
        [0, +inf], [-inf, 0] or [dmin, dmax] and it is known to be continuous in it.  One call of the op."""
        idx, want, _ = parse_monotonic(constraints)
        vlo, vhi, vfl, dlo, dhi, dfl = self._derivative_op("monotone_mask", lower, upper, self._wrt(idx))
        ok = _root_safe(vlo, vhi, vfl, max_abs)
        for k, (dmin, dmax) in enumerate(want):
            ok = ok & ((dfl[k, :, 0] & 3) == 0) & (dlo[k, :, 0] >= dmin) & (dhi[k, :, 0] <= dmax)
        return ok

    # ---- input gradients on the data ----------------------------------------------------------------
    def _xgrad_wrt(self, what: str, wrt, extra=()):
        """the requested variables of the input-gradient ops as a host list: ``_wrt``'s checks, then the variables of ``extra`` that
        ``wrt`` lacks appended, distinct, at most ``XGRAD_MAX_VARS``"""
        self._single_output(what, ValueError)
        if wrt is None and self.input_len > XGRAD_MAX_VARS:
            raise ValueError(f"{what}: wrt=None asks for all {self.input_len} variables, but one call takes at most {XGRAD_MAX_VARS}: "
                             "name the variables in wrt")
        idx = self._wrt(wrt)
        if len(set(idx)) != len(idx):
            raise ValueError(f"{what}: wrt names a variable twice: {idx}")
        if extra:
            idx = idx + [v for v in self._wrt(list(extra)) if v not in idx]
        if len(idx) > XGRAD_MAX_VARS:
            raise ValueError(f"{what}: {len(idx)} variables are requested, but one call takes at most {XGRAD_MAX_VARS}")
        return idx

    def SR_input_gradients(self, inputs: Tensor, wrt=None):
        """``(pred, grad)``: ``pred`` (pop, D) the prediction of every tree on every row of ``inputs`` (D, input_len), ``grad`` (pop, D, V)
        its partial derivative in variable ``wrt[k]`` at that row -- reverse-mode differentiation on the value tape (csrc/sr_xgrad.hip,
        one HIP pass), by the rules of the constant gradient.  ``grad`` is a permuted view of the kernel's (V, pop, D) array.  A
        variable the tree does not hold has exactly 0; a malformed tree NaN everywhere.  A derivative may be NaN where the prediction
        is finite (``0 * NaN`` under a branch that was not taken).  ``wrt``: an int or a list of distinct variables, at most
        ``XGRAD_MAX_VARS`` = 8; None means every variable and needs ``input_len <= 8`` (``ValueError`` otherwise, as for an index out
        of range, a repeated index or a multi-output forest)."""
        idx = self._xgrad_wrt("SR_input_gradients", wrt)
        inputs = check_tensor(inputs, self.batch_node_value.device)
        assert inputs.dim() == 2 and inputs.shape[1] == self.input_len, (
            f"inputs shape[1] should be {self.input_len}, but got {tuple(inputs.shape)}")
        pred, dpred = torch.ops.evogp_hip.tree_SR_input_gradient(*self._tensors(), inputs.contiguous().to(torch.float32), idx)
        return pred, dpred.permute(1, 2, 0)

    def SR_derivative_loss(self, inputs: Tensor, labels: Tensor, dlabels: Optional[Tensor] = None, wrt=None, bounds=None):
        """``(loss, violations)`` without a (pop, D) array (csrc/sr_xgrad.hip, one HIP pass, no host synchronisation): ``loss`` (pop, 1 + V)
        float32 -- column 0 the mean squared error of the prediction against ``labels`` (D, 1), column 1 + k the mean squared error of
        d tree / d x_wrt[k] against ``dlabels[:, k]`` (``dlabels`` (D, V); None: zeros, the column is then the mean squared sensitivity
        to the variable); ``violations`` (pop, V) int32 -- the rows on which that derivative is outside its range in ``bounds`` =
        ``{variable: +1 | -1 | (dmin, dmax)}`` (``parse_monotonic``) or is NaN; a variable without a bound counts its NaN rows only.
        Variables of ``bounds`` that ``wrt`` lacks are appended to it; the columns follow that order (``dlabels`` then needs a column
        for each).  A column is NaN when a row term is not finite; a malformed tree has NaN columns and ``D`` violations.  Sums are
        float64 in a fixed order: bit-identical from run to run.  ``ValueError`` as for ``SR_input_gradients``."""
        variables, ranges, _ = parse_monotonic(bounds or {})
        idx = self._xgrad_wrt("SR_derivative_loss", wrt, variables)
        inputs, labels = self._sr_data(inputs, labels)
        dev, V = self.batch_node_value.device, len(idx)
        if dlabels is not None:
            dlabels = check_tensor(dlabels, dev)
            if dlabels.shape != (inputs.shape[0], V):
                raise ValueError(f"dlabels should have shape ({inputs.shape[0]}, {V}): one column per requested variable {idx}, "
                                 f"but got {tuple(dlabels.shape)}")
            dlabels = dlabels.contiguous().to(torch.float32)
        dmin = dmax = None
        if variables:
            lo, hi = [float("-inf")] * V, [float("inf")] * V
            for v, (a, b) in zip(variables, ranges):
                lo[idx.index(v)], hi[idx.index(v)] = a, b
            dmin, dmax = torch.tensor(lo, dtype=torch.float32).to(dev), torch.tensor(hi, dtype=torch.float32).to(dev)
        return torch.ops.evogp_hip.tree_SR_derivative_loss(*self._tensors(), inputs, labels, dlabels, idx, dmin, dmax)

    # ---- semantic backpropagation --------------------------------------------------------------------
    def _backprop_args(self, what: str, inputs: Tensor, labels: Tensor, positions: Tensor):
        """the dataset and the positions as the two ops take them; ``ValueError`` for a multi-output forest or positions of another
        shape or a non-integer dtype (their RANGE is the kernel's to report: status 2, no host synchronisation)"""
        self._single_output(what, ValueError)
        inputs, labels = self._sr_data(inputs, labels)
        positions = check_tensor(positions, self.batch_node_value.device)
        if tuple(positions.shape) != (self.pop_size,):
            raise ValueError(f"{what}: positions should have shape ({self.pop_size},), but got {tuple(positions.shape)}")
        if positions.dtype.is_floating_point or positions.dtype == torch.bool:
            raise ValueError(f"{what}: positions should be integers, but got {positions.dtype}")
        return inputs, labels, positions.contiguous().to(torch.int32)

    def SR_desired_semantics(self, inputs: Tensor, labels: Tensor, positions: Tensor):
        """``(desired, state, status)``: semantic backpropagation (Pawlak, Wieloch & Krawiec 2015; csrc/sr_backprop.hip, one HIP pass, no
        host synchronisation).  ``desired`` (pop, D) float32 is the value the subtree at node ``positions[t]`` of tree t would have to
        return on row d for the whole tree to return ``labels[d]``: the tree inverted from its root down to that node, one float32
        operation per function on the way (DESIGN.md 3.24 has the table).  ``state`` (pop, D) uint8: 0 REQUIRED (``desired`` holds the
        value), 1 FREE (any value reproduces the label: ``0 * x``, the branch an IF does not take), 2 IMPOSSIBLE (no value does);
        ``desired`` is NaN where the state is not 0.  ``status`` (pop,) int32: 0 ok, 1 malformed row, 2 position outside the tree, 3
        BLOCKED (a function on the path has no inverse here: sin, pow, a comparison, a loose variant, an IF's condition); with a status
        other than 0 every row is IMPOSSIBLE.  ``ValueError`` for a multi-output forest or ``positions`` that is not (pop,) integers."""
        inputs, labels, positions = self._backprop_args("SR_desired_semantics", inputs, labels, positions)
        return torch.ops.evogp_hip.tree_SR_desired(*self._tensors(), inputs, labels, positions)

    def SR_backprop_match(self, inputs: Tensor, labels: Tensor, positions: Tensor, library):
        """``(best, dist, const, const_dist, counts, status)``: the desired values of ``SR_desired_semantics`` matched against a library
        of subtrees in the same HIP pass, without a (pop, D) array and without a host synchronisation.  ``library``: a (K, D) float32
        tensor of semantics, or a single-output Forest of K trees whose semantics are ``library.batch_forward(inputs)``; 1 <= K <=
        ``BACKPROP_MAX_LIBRARY`` = 1024.  ``dist`` (pop, K) float64: the squared distance of member k to the desired values over the
        REQUIRED rows (+inf where the member is not finite on one of them); ``best`` (pop,) int32 the nearest member, the smallest
        index on ties, -1 when ``status`` is not 0, no row is REQUIRED or no member is finite; ``const`` (pop,) float32 and
        ``const_dist`` (pop,) float64 the best constant (the mean of the desired values) and its distance; ``counts`` (pop, 3) int32
        the REQUIRED, FREE and IMPOSSIBLE rows.  ``ValueError`` as for ``SR_desired_semantics``, and for a library of another shape."""
        inputs, labels, positions = self._backprop_args("SR_backprop_match", inputs, labels, positions)
        library = self._library_semantics("SR_backprop_match", library, inputs)
        return torch.ops.evogp_hip.tree_SR_backprop_match(*self._tensors(), inputs, labels, positions, library)

    def _library_semantics(self, what: str, library, inputs: Tensor) -> Tensor:
        """the (K, D) float32 semantics a match op takes, from a tensor or from a library Forest"""
        if isinstance(library, Forest):
            if library.input_len != self.input_len or library.output_len != 1:
                raise ValueError(f"{what}: the library forest should have {self.input_len} inputs and one output, but has "
                                 f"{library.input_len} and {library.output_len}")
            library = library.batch_forward(inputs)[:, :, 0]
        library = check_tensor(library, self.batch_node_value.device)
        if library.dim() != 2 or library.shape[1] != inputs.shape[0] or not 1 <= library.shape[0] <= BACKPROP_MAX_LIBRARY:
            raise ValueError(f"{what}: library should have shape (K, {inputs.shape[0]}) with 1 <= K <= {BACKPROP_MAX_LIBRARY}, "
                             f"but got {tuple(library.shape)}")
        return library.contiguous().to(torch.float32)

    # ---- approximately geometric semantic crossover: the target is the midpoint of two parents ----
    def _midpoint_args(self, what: str, inputs: Tensor, positions: Tensor, mates, mate_index):
        """the datapoints, the positions, the mates and the mate index as the two ops take them; the RANGE of ``mate_index`` is the
        kernel's to report (status 4, no host synchronisation)"""
        self._single_output(what, ValueError)
        if not isinstance(mates, Forest) or mates.output_len != 1:
            raise ValueError(f"{what}: mates should be a single-output Forest")
        if mates.input_len != self.input_len or mates.max_tree_len != self.max_tree_len:
            raise ValueError(f"{what}: mates should have input_len {self.input_len} and max_tree_len {self.max_tree_len}, but have "
                             f"{mates.input_len} and {mates.max_tree_len}")
        dev = self.batch_node_value.device
        inputs = check_tensor(inputs, dev)
        assert inputs.dim() == 2 and inputs.shape[1] == self.input_len, f"inputs shape should be (datapoints, {self.input_len}), but got {tuple(inputs.shape)}"
        positions = check_tensor(positions, dev)
        if tuple(positions.shape) != (self.pop_size,):
            raise ValueError(f"{what}: positions should have shape ({self.pop_size},), but got {tuple(positions.shape)}")
        if positions.dtype.is_floating_point or positions.dtype == torch.bool:
            raise ValueError(f"{what}: positions should be integers, but got {positions.dtype}")
        if mate_index is None:
            if mates.pop_size != self.pop_size:
                raise ValueError(f"{what}: without a mate_index the mates should have {self.pop_size} trees, but have {mates.pop_size}")
            mate_index = torch.arange(self.pop_size, dtype=torch.int32, device=dev)
        else:
            mate_index = check_tensor(mate_index, dev)
            if tuple(mate_index.shape) != (self.pop_size,) or mate_index.dtype.is_floating_point or mate_index.dtype == torch.bool:
                raise ValueError(f"{what}: mate_index should be ({self.pop_size},) integers, but got {tuple(mate_index.shape)} {mate_index.dtype}")
        return (inputs.contiguous().to(torch.float32), positions.contiguous().to(torch.int32), mates._tensors(),
                mate_index.contiguous().to(torch.int32))

    def SR_midpoint_semantics(self, inputs: Tensor, positions: Tensor, mates: "Forest", mate_index: Optional[Tensor] = None):
        """``(desired, state, status)`` as ``SR_desired_semantics``, with the labels replaced by a MATE (approximately geometric semantic
        crossover, Pawlak, Wieloch & Krawiec 2015; csrc/sr_backprop.hip; one HIP pass, no host synchronisation, no
        labels).  Tree t is paired with tree ``mate_index[t]`` of ``mates`` -- a single-output Forest of the same ``input_len`` and
        ``max_tree_len``; ``None``: with tree t, and then ``mates.pop_size == pop_size``.  On row d the root target is the midpoint
        ``0.5 * T_t(x_d) + 0.5 * T_mate(x_d)`` in float32: REQUIRED where it is finite, IMPOSSIBLE at every position where it is not.
        So at ``positions[t] == 0`` the desired values are the midpoints.  ``status`` gains 4: the mate index is outside the mates, or
        the mate's row is malformed (decided after 1 and 2, before 3).  ``ValueError`` for a multi-output forest on either side, another
        ``input_len`` or ``max_tree_len``, ``positions`` or ``mate_index`` that is not (pop,) integers."""
        inputs, positions, mate_rows, mate_index = self._midpoint_args("SR_midpoint_semantics", inputs, positions, mates, mate_index)
        return torch.ops.evogp_hip.tree_SR_desired_mid(*self._tensors(), *mate_rows, inputs, positions, mate_index)

    def SR_midpoint_match(self, inputs: Tensor, positions: Tensor, mates: "Forest", library, mate_index: Optional[Tensor] = None):
        """``(best, dist, const, const_dist, counts, status)`` as ``SR_backprop_match``, for the desired values of
        ``SR_midpoint_semantics``: the library member nearest to what the subtree at ``positions[t]`` would have to return for tree t
        to land on the midpoint between itself and its mate.  Same HIP pass, no (pop, D) array, no host synchronisation.
        ``ValueError`` as for ``SR_midpoint_semantics``, and for a bad library as in ``SR_backprop_match``."""
        inputs, positions, mate_rows, mate_index = self._midpoint_args("SR_midpoint_match", inputs, positions, mates, mate_index)
        library = self._library_semantics("SR_midpoint_match", library, inputs)
        return torch.ops.evogp_hip.tree_SR_agx_match(*self._tensors(), *mate_rows, inputs, positions, mate_index, library)

    # ---- dimensional analysis --------------------------------------------------------------------
    def SR_dimensions(self, input_units, label_units=None):
        """``(units, flags, violations)``: dimensional analysis of every tree (csrc/sr_dims.hip, one lane per tree, no dataset, no host
        synchronisation beyond the conversion of the units).  ``input_units``: ``(input_len, K)`` exponents of the K base dimensions
        (1 .. 8) for every input -- ints, floats or ``Fraction``s, each a multiple of 1/25200; ``label_units``: ``(K,)``, or None to leave
        the root free.  A constant may carry whatever unit makes its tree consistent.  ``violations`` (pop,) int32: 0 iff the constants
        can be given units under which every operation is consistent and the root has ``label_units`` (always sound; complete but for
        trees with a ``pow`` whose base is free, such as a product with a constant), otherwise the number of violating nodes, -1 for a malformed row.
        ``units`` (pop, max_tree_len, K) int32: the unit of every node as numerators over 25200 -- of a consistent tree under one
        consistent assignment, ``tree.utils.str_unit`` prints a row; ``flags`` (pop, max_tree_len) uint8: 1 = the node is free,
        2 = violation, 4 = malformed row, 8 = the root's unit is not the label's.  ``ValueError`` for an exponent that is no multiple
        of 1/25200 or beyond 2^24 / 25200 in magnitude, a wrong shape, or a multi-output forest."""
        self._single_output("SR_dimensions", ValueError)
        var, label, check_root = check_units(input_units, label_units, self.input_len)   # int numerators over 25200
        dev = self.batch_node_value.device
        return torch.ops.evogp_hip.tree_dimensions(*self._tensors(), torch.tensor(var, dtype=torch.int32).to(dev),
                                                   torch.tensor(label, dtype=torch.int32).to(dev), check_root)

    def dimension_mask(self, input_units, label_units=None) -> Tensor:
        """(pop,) bool: the tree is dimensionally consistent (``SR_dimensions``: ``violations == 0``)"""
        return self.SR_dimensions(input_units, label_units)[2] == 0

    # ---- structural constraints -----------------------------------------------------------------
    def SR_structure(self, complexity_of=None, nested_constraints=None, operand_constraints=None, max_depth=None, max_complexity=None):
        """``(complexity, height, depth, nest, flags, violations)``: the structural pass over every tree (csrc/sr_structure.hip, one lane
        per tree, no dataset, no host synchronisation beyond the conversion of the tables).  The three dictionaries are
        ``tree.utils.parse_structure``'s: ``complexity_of={"sin": 3}`` the cost of one node (1 where not given),
        ``nested_constraints={"sin": {"sin": 0, "cos": 0}}`` at most ``limit`` inner nodes on any path below an outer node (R rules,
        one per pair, at most 8), ``operand_constraints={"pow": (-1, 1)}`` the largest complexity of each operand.  ``max_depth``: the
        largest number of nodes on a path from the root to a leaf (a single leaf has 1), ``max_complexity``: the largest complexity of
        the tree; None for no limit.  ``complexity`` (pop, max_tree_len) int32: the summed cost of every subtree (with unit costs its
        size); ``height`` int16: nodes on the longest path down from the node; ``depth`` int16: edges up to the root; ``nest`` (pop,
        max_tree_len, R) uint8: the inner nodes of rule r on the fullest path from the node down, the node included, saturating at
        255; ``flags`` uint8: 1 = a nesting rule fails at this node, 2 = an operand of this node is too complex, 4 = malformed row,
        8 = too deep (node 0), 16 = too complex (node 0); ``violations`` (pop,) int32: the nodes with flag 1 or 2, plus one each for
        8 and 16; 0 = the tree passes, -1 = malformed row.  ``ValueError`` for what ``parse_structure`` refuses, a limit that is no
        int >= 0, or a multi-output forest."""
        self._single_output("SR_structure", ValueError)
        return self._structure_op(parse_structure(complexity_of, nested_constraints, operand_constraints), max_depth, max_complexity)

    def _structure_op(self, tables, max_depth=None, max_complexity=None):
        """the op under ``parse_structure``'s tables"""
        limits = []
        for name, m in (("max_depth", max_depth), ("max_complexity", max_complexity)):
            if m is not None and (isinstance(m, bool) or not isinstance(m, (int, np.integer)) or not 0 <= int(m) < 2 ** 31):
                raise ValueError(f"{name} should be None or an int >= 0, but got {m!r}")
            limits.append(-1 if m is None else int(m))
        cost, operand_limit, rules = tables
        dev = self.batch_node_value.device

        def words(x, shape):   # (a set that holds symbol 31 is a negative int32 word)
            return torch.tensor([v - (1 << 32) if v >= 1 << 31 else v for v in x], dtype=torch.int32).reshape(shape).to(dev)

        return torch.ops.evogp_hip.tree_structure(
            *self._tensors(), words(cost, (32,)), words([l for row in operand_limit for l in row], (32, 3)),
            words([r[0] for r in rules], (len(rules),)), words([r[1] for r in rules], (len(rules),)),
            words([r[2] for r in rules], (len(rules),)), *limits)

    def structure_mask(self, complexity_of=None, nested_constraints=None, operand_constraints=None, max_depth=None,
                       max_complexity=None) -> Tensor:
        """(pop,) bool: the tree obeys every structural constraint (``SR_structure``: ``violations == 0``)"""
        return self.SR_structure(complexity_of, nested_constraints, operand_constraints, max_depth, max_complexity)[5] == 0

    def complexity(self, complexity_of=None) -> Tensor:
        """(pop,) int32: the weighted complexity of every tree (``SR_structure``: ``complexity[:, 0]``; 0 for a malformed row).  With
        ``complexity_of=None`` the tree size."""
        return self.SR_structure(complexity_of)[0][:, 0]

    # ---- genetic operators --------------------------------------------------------------------
    def mutate(self, replace_pos: Tensor, new_sub_forest: "Forest") -> "Forest":
        """Replace the subtree at replace_pos[n] of tree n by the whole tree new_sub_forest[n]."""
        replace_pos = check_tensor(replace_pos, self.batch_node_value.device)
        assert replace_pos.shape == (self.pop_size,), (
            f"replace_pos shape should be ({self.pop_size}, ), but got {replace_pos.shape}")
        for attr in ("pop_size", "input_len", "output_len", "max_tree_len"):
            assert getattr(self, attr) == getattr(new_sub_forest, attr), (
                f"{attr} should be {getattr(self, attr)}, but got {getattr(new_sub_forest, attr)}")
        value, ntype, size = torch.ops.evogp_cuda.tree_mutate(
            self.pop_size, self.max_tree_len, *self._tensors(), replace_pos.contiguous().to(torch.int32),
            *new_sub_forest._tensors())
        return Forest(self.input_len, self.output_len, value, ntype, size, func_mask=Forest.join_masks(self.func_mask, new_sub_forest.func_mask))

    def crossover(self, left_indices: Tensor, right_indices: Tensor, left_pos: Tensor, right_pos: Tensor) -> "Forest":
        """out[n] = self[left_indices[n]] with subtree left_pos[n] replaced by subtree right_pos[n] of
        self[right_indices[n]]."""
        idx = [check_tensor(t, self.batch_node_value.device).contiguous().to(torch.int32) for t in (left_indices, right_indices, left_pos, right_pos)]
        n = idx[0].shape[0]
        for name, t in zip(("left_indices", "right_indices", "left_pos", "right_pos"), idx):
            assert t.shape == (n,), f"{name} shape should be ({n}, ), but got {t.shape}"
        value, ntype, size = torch.ops.evogp_cuda.tree_crossover(self.pop_size, n, self.max_tree_len,
                                                                 *self._tensors(), *idx)
        return Forest(self.input_len, self.output_len, value, ntype, size, func_mask=self.func_mask)

    # ---- container protocol -------------------------------------------------------------------
    def __getitem__(self, index):
        if isinstance(index, int) or (hasattr(index, "shape") and tuple(index.shape) == ()):
            return Tree(self.input_len, self.output_len, self.batch_node_value[index], self.batch_node_type[index],
                        self.batch_subtree_size[index])
        if isinstance(index, (slice, Tensor, np.ndarray)):
            return Forest(self.input_len, self.output_len, self.batch_node_value[index],
                          self.batch_node_type[index], self.batch_subtree_size[index], func_mask=self.func_mask)
        raise Exception(f"Do not support index type {type(index)}")

    def __setitem__(self, index, value):
        if isinstance(index, int):
            assert isinstance(value, Tree), f"value should be Tree when index is int, but got {type(value)}"
            self.batch_node_value[index] = value.node_value
            self.batch_node_type[index] = value.node_type
            self.batch_subtree_size[index] = value.subtree_size
        elif isinstance(index, (slice, Tensor, np.ndarray)):
            assert isinstance(value, Forest), f"value should be Forest when index is slice, but got {type(value)}"
            joined = Forest.join_masks(self.func_mask, value.func_mask)
            self.batch_node_value[index] = value.batch_node_value
            self.batch_node_type[index] = value.batch_node_type
            self.batch_subtree_size[index] = value.batch_subtree_size
            self._func_mask = (joined, self._forest_key()) if joined else None
        else:
            raise NotImplementedError

    def __iter__(self):
        for i in range(self.pop_size):
            yield self[i]

    def __len__(self):
        return self.pop_size

    def __add__(self, other):
        assert other.input_len == self.input_len and other.output_len == self.output_len
        if isinstance(other, Forest):
            parts = (other.batch_node_value, other.batch_node_type, other.batch_subtree_size)
        elif isinstance(other, Tree):
            parts = (other.node_value.unsqueeze(0), other.node_type.unsqueeze(0), other.subtree_size.unsqueeze(0))
        else:
            raise NotImplementedError
        return Forest(self.input_len, self.output_len,
                      torch.cat([self.batch_node_value, parts[0]], dim=0),
                      torch.cat([self.batch_node_type, parts[1]], dim=0),
                      torch.cat([self.batch_subtree_size, parts[2]], dim=0),
                      func_mask=Forest.join_masks(self.func_mask, other.func_mask) if isinstance(other, Forest) else 0)

    def __radd__(self, other):
        return self.__add__(other)

    def __str__(self):
        lines = [f"Forest(pop size: {self.pop_size})", "["]
        lines += [f"  {tree}, " for tree in self]
        lines.append("]")
        return "\n".join(lines)

    __repr__ = __str__

    # ---- pickling (numpy round trip, forest.py:476-499) ----------------------------------------
    def __getstate__(self):
        return {
            "input_len": self.input_len,
            "output_len": self.output_len,
            "batch_node_value": self.batch_node_value.cpu().numpy(),
            "batch_node_type": self.batch_node_type.cpu().numpy(),
            "batch_subtree_size": self.batch_subtree_size.cpu().numpy(),
        }

    def __setstate__(self, state):
        dev = _utils.default_device()
        self.input_len = state["input_len"]
        self.output_len = state["output_len"]
        self.pop_size, self.max_tree_len = state["batch_node_value"].shape
        self.batch_node_value = torch.from_numpy(state["batch_node_value"]).to(dev)
        self.batch_node_type = torch.from_numpy(state["batch_node_type"]).to(dev)
        self.batch_subtree_size = torch.from_numpy(state["batch_subtree_size"]).to(dev)
