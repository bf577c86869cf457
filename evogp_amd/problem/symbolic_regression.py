"""SymbolicRegression — fitness = minus the mean squared/absolute error of every tree over a
dataset (src/evogp/problem/symbolic_regression.py:9-96).  ``execute_mode`` keeps the reference's
strings; every kernel mode maps onto the one fused HIP kernel, ``"torch"`` evaluates with
``Forest.batch_forward`` (the non-replicating batch op) and reduces in torch."""
from __future__ import annotations

from fractions import Fraction
from typing import Callable, Optional

import torch
from torch import Tensor

from ..tree import Forest, default_device
from ..tree.forest import check_loss
from ..tree.utils import DIM_DEN, box_side, check_units, parse_monotonic, parse_structure
from .base import BaseProblem

_MODES = ["torch", "hybrid parallel", "data parallel", "tree parallel", "auto"]


class SymbolicRegression(BaseProblem):
    def __init__(self, datapoints: Optional[Tensor] = None, labels: Optional[Tensor] = None,
                 func: Optional[Callable] = None, num_inputs: Optional[int] = None, num_data: Optional[int] = 100,
                 lower_bounds=-1, upper_bounds=1, execute_mode: str = "auto", const_opt_steps: int = 0,
                 const_step_size: float = 0.1, simplify_every: int = 0, const_opt_method: str = "descent",
                 dedup: bool = False, linear_scaling: bool = False, interval_check: bool = False, input_bounds="data",
                 input_margin: float = 0.0, monotonic=None, multigene: bool = False, input_units=None, label_units=None,
                 dimension_penalty: Optional[float] = None, semantic_dedup: bool = False, semantic_keep: str = "smallest",
                 max_depth: Optional[int] = None, max_complexity: Optional[int] = None, complexity_of=None, nested_constraints=None,
                 operand_constraints=None, structure_penalty: Optional[float] = None, loss: Optional[str] = None,
                 loss_param: Optional[float] = None, sample_weights: Optional[Tensor] = None,
                 validation_mask: Optional[Tensor] = None, const_opt_loss: Optional[str] = None,
                 scaling_loss: Optional[str] = None, derivative_labels: Optional[Tensor] = None, derivative_wrt=None,
                 derivative_weight=1.0, sampled_monotonic=None, intron_removal_every: int = 0):
        """``const_opt_steps`` > 0 (no counterpart in the reference): ``optimize`` tunes every tree's constants by that many steps of
        ``Forest.optimize_constants``, and StandardPipeline scores the optimised forest (Lamarckian).  ``const_opt_method``:
        ``"descent"`` (gradient descent with steps of ``const_step_size``) or ``"lm"`` (Levenberg-Marquardt; MSE, single-output).
        ``simplify_every`` = k > 0 (single-output problems): every k-th call of ``optimize`` first rewrites the forest with
        ``Forest.simplify`` (best subtree hoisted, row-constant subtrees folded), so the smaller trees are the ones scored and bred.
        ``dedup``: both run their dataset passes once per distinct tree (``Forest.duplicate_classes``); the results are the same.
        ``linear_scaling`` (Keijzer 2003; MSE, single-output problems): a tree T is scored by the error of ``a + b * T(x)`` with the
        least-squares ``a, b`` (``Forest.SR_scaled_fitness``, which honours ``dedup``), so evolution searches for the shape and the
        closed form supplies scale and offset; ``scaled(forest)`` returns the trees with their coefficients written in, and
        StandardPipeline reports its best tree that way.  ``optimize`` is untouched: simplification and constant tuning run first.
        ``interval_check`` (Keijzer 2003; single-output problems): a tree that interval arithmetic cannot show to be defined and finite
        on the whole box of admissible inputs (``Forest.safe_mask``) gets NaN from ``evaluate`` and -inf from ``scores``, whatever
        loss it has on the rows; the others keep their values bit for bit.  The box is fixed at construction: ``input_bounds="data"``
        takes the per-column minimum and maximum of ``datapoints``, each side moved outward by ``input_margin`` times the column's
        range; or pass a ``(lower, upper)`` pair of floats or ``(num_inputs,)`` tensors.
        ``monotonic`` (shape constraints, Kronberger et al. 2022; single-output problems): ``{variable: +1 | -1 | (dmin, dmax)}``.  A
        tree passes when it is safe on the box (``monotonic`` implies the check of ``interval_check``, on the same box) and interval
        arithmetic over its partial derivatives proves it nondecreasing (+1) or nonincreasing (-1) in the variable, or its derivative
        within [dmin, dmax], on the whole box (``Forest.monotone_mask``); the others get NaN / -inf as above.  With
        ``linear_scaling`` the constraint is on the tree's shape and the fitted slope may flip it, so under a +-1 constraint
        ``scaled_fitness`` gives a NaN loss to a tree whose slope is negative; a (dmin, dmax) pair bounds the unscaled tree.
        ``multigene`` (GPTIPS; Arnaldo et al. 2014; MSE, labels of shape ``(D, 1)``): the ``G = output_len`` outputs of a tree, 1 .. 8 of
        them, are features and the tree is scored by the error of ``b0 + sum_j w_j g_j(x)`` with the least-squares coefficients
        (``Forest.SR_gene_fitness``, which honours ``dedup``); ``gene_model(forest)`` returns the losses and the coefficients, and
        StandardPipeline keeps those of its best tree in ``best_coef``.  It contains linear scaling, and the single-output passes do not
        apply to it: ``ValueError`` together with ``linear_scaling``, ``const_opt_steps`` > 0, ``simplify_every`` > 0,
        ``interval_check`` or ``monotonic``, and from ``evaluate`` / ``scores`` with ``use_MSE=False``.
        ``input_units`` (dimensional analysis; labels of shape ``(D, 1)``): ``(num_inputs, K)`` exponents of K base dimensions for every
        input, ``label_units`` ``(K,)`` those of the target or None to leave the root free (``Forest.SR_dimensions``; a constant may carry
        any unit).  ``dimension_penalty=None``: a tree that cannot be made dimensionally consistent gets NaN from ``evaluate`` and -inf
        from ``scores`` (on top of the box masks where those are on), the others keep their values bit for bit; ``dimension_penalty=p``
        with ``p >= 0``: its fitness falls by ``p`` times the number of violating nodes instead (a malformed row still gets NaN / -inf).
        With ``linear_scaling`` the root is not held to ``label_units``: slope and intercept are free constants that carry whatever
        unit converts the tree's; violations inside the tree still count.  ``ValueError`` with ``multigene``, and for ``label_units`` or
        ``dimension_penalty`` without ``input_units``.
        ``semantic_dedup`` (single-output problems): trees that predict the same value on every datapoint are one candidate
        (``Forest.semantic_classes``: ``x0 + x1`` and ``x1 + x0``, ``x0 * 1`` and ``x0``, every tree that is NaN on all rows).  A tree
        that is not the representative of its class gets NaN from ``evaluate`` and -inf from ``scores``; every representative keeps
        its value bit for bit, so each behaviour competes once -- under ``semantic_keep="smallest"`` as its smallest tree, under
        ``"first"`` as its first.  ``semantic_classes(forest)`` returns the classes, also with ``semantic_dedup=False``.  With
        ``linear_scaling`` the UNSCALED predictions are compared: trees that are equal only up to an affine map (``x0`` and
        ``2 * x0 + 1``, which linear scaling scores alike) are NOT merged.  ``ValueError`` with ``multigene``.
        ``max_depth``, ``max_complexity``, ``nested_constraints``, ``operand_constraints`` (structural constraints; single-output
        problems): the limits of ``Forest.SR_structure`` -- the nodes on the longest path from the root to a leaf, the summed cost of
        the tree's nodes under ``complexity_of={name: cost}`` (1 where not given), ``{"sin": {"sin": 0, "cos": 0}}`` no sine or cosine
        inside a sine, ``{"pow": (-1, 1)}`` an exponent of complexity 1 at most.  They are parsed and checked here.
        ``structure_penalty=None``: a tree that breaks a limit gets NaN from ``evaluate`` and -inf from ``scores`` (on top of the other
        masks), the others keep their values bit for bit; ``structure_penalty=p`` with ``p >= 0``: its fitness falls by ``p`` times the
        number of violations instead (a malformed row still gets NaN / -inf).  ``structure(forest)`` and ``structure_mask(forest)``
        return the pass and who obeys; ``complexity(forest)`` the (pop,) complexity under ``complexity_of``, with or without a limit --
        the signature ``NSGA2Selection(complexity=, max_complexity=)`` takes.  ``ValueError`` with ``multigene``, and for
        ``structure_penalty`` without one of the four limits.
        ``loss``, ``loss_param``, ``sample_weights``, ``validation_mask`` (labels of shape ``(D, 1)``; with all four left at None
        nothing changes): the loss behind ``evaluate`` / ``scores`` becomes ``Forest.SR_weighted_loss`` -- ``loss`` one of ``"mse"``,
        ``"mae"``, ``"huber"`` (``loss_param`` = delta), ``"pinball"`` (``loss_param`` = tau) or ``"logcosh"`` (None: what ``use_MSE``
        says), every row weighted by ``sample_weights`` ``(D,)`` (non-negative, finite, not all 0).  ``validation_mask`` ``(D,)`` bool
        holds rows out: the same pass scores every tree twice, on the rows where the mask is False -- the loss that is evolved, masked
        and penalised as before -- and on the rows where it is True, kept on the device as ``last_validation_loss``;
        ``validation_scores(forest)`` returns the latter as scores, and StandardPipeline tracks ``best_validation_tree`` with it.  A
        tree need not be defined on a row it is not scored on.  ``ValueError`` together with ``linear_scaling`` (unless
        ``scaling_loss="problem"``, below), ``multigene`` or
        ``simplify_every`` > 0 (those passes minimise the unweighted MSE / MAE), together with ``const_opt_steps`` > 0 unless
        ``const_opt_loss="problem"``, and from ``evaluate`` / ``scores`` with ``use_MSE=False`` while ``loss`` is set.
        ``const_opt_loss``: None (constant tuning minimises the unweighted MSE / MAE, as ever) or ``"problem"``: ``optimize`` tunes
        under the problem's own loss -- ``loss`` and ``loss_param`` (MSE when only weights or a mask are given), on the training weight
        row: ``sample_weights`` with the held-out rows at 0, which the tuner therefore never reads (``Forest.optimize_constants(weights=,
        loss=, param=)``).  ``const_opt_method="lm"`` takes no ``loss`` but ``"mse"`` there (``ValueError``); a problem with none of
        the four loss options tunes as under None.
        ``scaling_loss`` (needs ``linear_scaling``; mirrors ``const_opt_loss``): None (every ``ValueError`` above stays) or
        ``"problem"``: linear scaling works under the problem's ``sample_weights`` and ``validation_mask``
        (``Forest.SR_weighted_scaled_fitness``, one pass).  Slope and intercept are fitted on the training weight row --
        ``sample_weights`` with the held-out rows at 0 -- and ``scaled_fitness``, ``scaled``, ``evaluate`` and ``scores`` state the
        error of that model on that row; ``last_validation_loss`` and ``validation_scores`` state the error of THE SAME model on the
        held-out rows, which the fit never read.  A closed form exists for the squared error only: ``loss`` other than None or
        ``"mse"`` raises ``ValueError``.  The sign check of ``monotonic``, the masks and penalties, ``dedup`` and
        ``const_opt_loss="problem"`` work on top of it; a problem with none of the four loss options scales as under None.
        ``derivative_labels``, ``derivative_wrt``, ``derivative_weight`` (derivative-informed fitness; labels of shape ``(D, 1)``):
        ``derivative_labels`` ``(D, V)`` holds measured or known values of d y / d x_v on the datapoints for the variables
        ``derivative_wrt`` (an int or a list of V distinct variables, at most 8; None: every variable, in order).  ``evaluate`` /
        ``scores`` then return ``-(loss_0 + sum_k weight_k * loss_k)`` with the columns of ``Forest.SR_derivative_loss``: the mean
        squared error of the prediction and of each partial derivative, in one pass (``execute_mode`` plays no part in it);
        ``derivative_weight`` is a float or a ``(V,)`` sequence, finite and >= 0.  ``derivative_loss(forest)`` returns the raw columns.
        ``ValueError`` together with ``linear_scaling``, ``multigene``, ``loss`` / ``loss_param`` / ``sample_weights`` /
        ``validation_mask``, ``const_opt_steps`` > 0 or ``simplify_every`` > 0 (those closed forms and tuners do not know the
        derivative columns), and from ``evaluate`` / ``scores`` with ``use_MSE=False``.
        ``sampled_monotonic`` (sampled shape constraints; single-output problems): ``{variable: +1 | -1 | (dmin, dmax)}`` as for
        ``monotonic``, but held on the ROWS of the dataset instead of proven on a box: a tree whose partial derivative in the variable
        leaves its range, or is NaN, on any datapoint gets NaN from ``evaluate`` and -inf from ``scores`` (the optimistic companion
        of ``monotonic``; the two may be combined).  Alone it only masks: the fitness of the other trees is the plain one, bit for
        bit.  Its variables are appended to ``derivative_wrt`` where that lacks them (they carry no label and no weight).

        ``intron_removal_every`` = k > 0 (single-output problems): every k-th call of ``optimize`` first takes the semantic introns out
        of the forest (``Forest.remove_introns`` on the datapoints: nodes that take the value of one of their own descendants on every
        row, ``x + 0``, ``max(x, x)``, ``neg(neg(x))``, ...), before ``simplify_every`` and the constant tuning.  No prediction changes
        on any row of ``datapoints``, so it goes with every loss, weights, ``validation_mask``, ``linear_scaling`` and the constraints;
        ``ValueError`` for labels of more than one column and together with ``multigene`` (the pass works on single-output trees)."""
        assert execute_mode in _MODES, f"execute_mode should be one of {_MODES}, but got {execute_mode}"
        assert const_opt_steps >= 0, f"const_opt_steps should be >= 0, but got {const_opt_steps}"
        self.execute_mode = execute_mode
        self.const_opt_steps = int(const_opt_steps)
        self.const_step_size = float(const_step_size)
        assert const_opt_method in ("descent", "lm"), f"const_opt_method should be 'descent' or 'lm', but got {const_opt_method}"
        self.const_opt_method = const_opt_method
        assert simplify_every >= 0, f"simplify_every should be >= 0, but got {simplify_every}"
        self.simplify_every = int(simplify_every)
        self.dedup = bool(dedup)
        self._optimize_calls = 0
        if isinstance(intron_removal_every, bool) or not isinstance(intron_removal_every, int) or intron_removal_every < 0:
            raise ValueError(f"intron_removal_every should be a non-negative integer, but got {intron_removal_every!r}")
        self.intron_removal_every, self._intron_calls = intron_removal_every, 0
        self.linear_scaling = bool(linear_scaling)
        if datapoints is not None and labels is not None:
            self.datapoints, self.labels = datapoints, labels
        else:
            assert func is not None and num_inputs is not None, (
                "func and num_inputs, must be provided when datapoints and labels are not provided")
            self.datapoints, self.labels = self.generate_data(func, num_inputs, num_data, lower_bounds, upper_bounds)
        # the checks fire in this order: scaling, interval, monotonic, multigene, units, semantic_keep, semantic_dedup, structure,
        # then the loss options: combinations, label shape, loss and loss_param, sample_weights, validation_mask
        if self.linear_scaling:
            self._one_label_column("linear_scaling")
        self.interval_check = bool(interval_check)
        if self.interval_check:
            self._one_label_column("interval_check")
        self.monotonic, self._sign_constrained = None, False
        if monotonic is not None:
            self._one_label_column("monotonic")
            variables, bounds, signs = parse_monotonic(monotonic, self.datapoints.shape[1])
            self.monotonic = {v: s if s else b for v, b, s in zip(variables, bounds, signs)}   # +1 | -1 | (dmin, dmax), normalised
            self._sign_constrained = any(signs)
        self._box_check = self.interval_check or self.monotonic is not None
        if self._box_check:
            self.input_lower, self.input_upper = self._input_box(input_bounds, float(input_margin))
        self.multigene = bool(multigene)
        if self.intron_removal_every > 0:
            self._one_label_column("intron_removal_every")
            if self.multigene:
                raise ValueError("multigene cannot be combined with intron_removal_every > 0: that pass works on single-output trees")
        if self.multigene:
            self._one_label_column("multigene", "fits one label column, (D, 1)")
            for name, on in (("linear_scaling", self.linear_scaling), ("const_opt_steps > 0", self.const_opt_steps > 0),
                             ("simplify_every > 0", self.simplify_every > 0), ("interval_check", self.interval_check),
                             ("monotonic", self.monotonic is not None)):
                if on:
                    raise ValueError(f"multigene cannot be combined with {name}: that pass works on single-output trees")
        self.input_units, self.label_units, self.dimension_penalty = None, None, None
        if input_units is None:
            if label_units is not None or dimension_penalty is not None:
                raise ValueError("label_units and dimension_penalty need input_units")
        else:
            if self.multigene:
                raise ValueError("multigene cannot be combined with input_units: dimensional analysis works on single-output trees")
            self._one_label_column("input_units")
            if dimension_penalty is not None:
                if isinstance(dimension_penalty, bool) or not float(dimension_penalty) >= 0.0:
                    raise ValueError(f"dimension_penalty should be None or a float >= 0, but got {dimension_penalty!r}")
                self.dimension_penalty = float(dimension_penalty)
            # checked here, on the host, so that a wrong shape or exponent fails at construction; kept as exact Fractions
            var, label, has_label = check_units(input_units, label_units, self.datapoints.shape[1])
            self.input_units = [[Fraction(n, DIM_DEN) for n in row] for row in var]
            self.label_units = [Fraction(n, DIM_DEN) for n in label] if has_label else None
        self.semantic_dedup = bool(semantic_dedup)
        if semantic_keep not in ("first", "smallest"):
            raise ValueError(f"semantic_keep should be 'first' or 'smallest', but got {semantic_keep!r}")
        self.semantic_keep = semantic_keep
        if self.semantic_dedup:
            if self.multigene:
                raise ValueError("multigene cannot be combined with semantic_dedup: semantic classes compare single-output trees")
            self._one_label_column("semantic_dedup")
        self.max_depth, self.max_complexity, self.structure_penalty = None, None, None
        self._structural = any(o is not None for o in (max_depth, max_complexity, nested_constraints, operand_constraints))
        if self._structural or complexity_of is not None:
            if self.multigene:
                raise ValueError("multigene cannot be combined with structural constraints: that pass works on single-output trees")
            self._one_label_column("structural constraints")
        if structure_penalty is not None:
            if not self._structural:
                raise ValueError("structure_penalty needs max_depth, max_complexity, nested_constraints or operand_constraints")
            if isinstance(structure_penalty, bool) or not float(structure_penalty) >= 0.0:
                raise ValueError(f"structure_penalty should be None or a float >= 0, but got {structure_penalty!r}")
            self.structure_penalty = float(structure_penalty)
        for name, m in (("max_depth", max_depth), ("max_complexity", max_complexity)):
            if m is not None:
                if isinstance(m, bool) or not isinstance(m, int) or not 0 <= m < 2 ** 31:
                    raise ValueError(f"{name} should be None or an int >= 0, but got {m!r}")
                setattr(self, name, m)
        # parsed here, on the host, so that an unknown name or a limit out of range fails at construction
        self._structure_tables = parse_structure(complexity_of, nested_constraints, operand_constraints)
        self._cost_tables = (self._structure_tables[0], parse_structure()[1], [])   # complexity(): the costs, no limits
        self._constrained = self._box_check or self.input_units is not None or self.semantic_dedup or self._structural
        self.loss, self.loss_param, self.sample_weights, self.validation_mask = loss, loss_param, None, None
        self.last_validation_loss = None   # (pop,): the loss on the held-out rows, of the forest scored last
        self._loss_weights = None          # (K, D) float32 on the data's device: what SR_weighted_loss is called with
        self._own_loss = any(o is not None for o in (loss, loss_param, sample_weights, validation_mask))
        if const_opt_loss not in (None, "problem"):
            raise ValueError(f"const_opt_loss should be None or 'problem', but got {const_opt_loss!r}")
        self.const_opt_loss = const_opt_loss
        if scaling_loss not in (None, "problem"):
            raise ValueError(f"scaling_loss should be None or 'problem', but got {scaling_loss!r}")
        if scaling_loss == "problem" and not self.linear_scaling:
            raise ValueError("scaling_loss='problem' needs linear_scaling=True")
        self.scaling_loss = scaling_loss
        self._scaling_own = scaling_loss == "problem" and self._own_loss   # linear scaling under the problem's weight rows
        if self._scaling_own and loss not in (None, "mse"):
            raise ValueError(f"linear scaling has a closed form for the squared error only, but the problem's loss is {loss!r}")
        if self._own_loss:
            if const_opt_loss == "problem" and self.const_opt_method == "lm" and loss not in (None, "mse"):
                raise ValueError(f"const_opt_method='lm' minimises the (weighted) mean squared error, but the problem's loss is {loss!r}")
            for name, on in (("linear_scaling", self.linear_scaling and not self._scaling_own), ("multigene", self.multigene),
                             ("const_opt_steps > 0", self.const_opt_steps > 0 and const_opt_loss != "problem"),
                             ("simplify_every > 0", self.simplify_every > 0)):
                if on:
                    raise ValueError(f"loss, loss_param, sample_weights and validation_mask cannot be combined with {name}: "
                                     "that pass minimises the unweighted mean squared / absolute error")
            self._one_label_column("loss, loss_param, sample_weights and validation_mask", "work on one label column, (D, 1)")
            if loss is None and loss_param is not None:
                raise ValueError(f"loss_param needs a loss, but got loss_param={loss_param!r} alone")
            if loss is not None:
                self.loss_param = check_loss(loss, loss_param)
            dev, D = self.datapoints.device, self.datapoints.shape[0]
            w = None
            if sample_weights is not None:
                if not isinstance(sample_weights, Tensor) or sample_weights.shape != (D,) or not sample_weights.dtype.is_floating_point:
                    raise ValueError(f"sample_weights should be a ({D},) floating-point tensor, but got "
                                     f"{tuple(sample_weights.shape) if isinstance(sample_weights, Tensor) else sample_weights!r}")
                w = sample_weights.detach().to(dev).to(torch.float32)
                if not bool((torch.isfinite(w) & (w >= 0)).all()) or not float(w.sum()) > 0.0:   # (the one host synchronisation)
                    raise ValueError("sample_weights should be finite, non-negative and not all 0")
                self.sample_weights = w
            if validation_mask is not None:
                if not isinstance(validation_mask, Tensor) or validation_mask.shape != (D,) or validation_mask.dtype != torch.bool:
                    raise ValueError(f"validation_mask should be a ({D},) bool tensor, but got "
                                     f"{(tuple(validation_mask.shape), validation_mask.dtype) if isinstance(validation_mask, Tensor) else validation_mask!r}")
                m = validation_mask.detach().to(dev)
                held = int(m.sum())
                if held == 0 or held == D:
                    raise ValueError(f"validation_mask should hold some rows out and leave some in, but {held} of {D} are True")
                self.validation_mask = m
                ones = torch.ones(D, dtype=torch.float32, device=dev) if w is None else w
                self._loss_weights = torch.stack([ones * (~m), ones * m]).contiguous()   # training rows, validation rows
            elif w is not None:
                self._loss_weights = w[None, :].contiguous()

        self._init_derivatives(derivative_labels, derivative_wrt, derivative_weight, sampled_monotonic)

    def _init_derivatives(self, derivative_labels, derivative_wrt, derivative_weight, sampled_monotonic):
        """the derivative options, checked on the host: ``_deriv_wrt`` (the variables of one ``SR_derivative_loss`` call),
        ``derivative_labels`` (D, V) padded with a zero column per appended variable, ``derivative_weight`` (n labelled,) float64"""
        self.derivative_labels, self.derivative_weight, self.sampled_monotonic = None, None, None
        self._deriv_wrt, self._deriv_labelled, self._deriv_pending = [], 0, None
        if derivative_labels is None and sampled_monotonic is None:
            if derivative_wrt is not None:
                raise ValueError("derivative_wrt needs derivative_labels")
            return
        num_inputs, D = self.datapoints.shape[1], self.datapoints.shape[0]
        wrt = []
        if derivative_labels is not None:
            for name, on in (("linear_scaling", self.linear_scaling), ("multigene", self.multigene),
                             ("loss, loss_param, sample_weights or validation_mask", self._own_loss),
                             ("const_opt_steps > 0", self.const_opt_steps > 0), ("simplify_every > 0", self.simplify_every > 0)):
                if on:
                    raise ValueError(f"derivative_labels cannot be combined with {name}: that pass does not know the derivative columns")
            self._one_label_column("derivative_labels", "works on one label column, (D, 1)")
            if derivative_wrt is None:
                if num_inputs > 8:
                    raise ValueError(f"derivative_wrt=None asks for all {num_inputs} variables, but at most 8 are supported: name them")
                wrt = list(range(num_inputs))
            else:
                wrt = [derivative_wrt] if isinstance(derivative_wrt, int) else [int(v) for v in derivative_wrt]
            if not wrt or len(set(wrt)) != len(wrt) or not all(0 <= v < num_inputs for v in wrt):
                raise ValueError(f"derivative_wrt should name distinct variables in 0 .. {num_inputs - 1}, but got {wrt}")
            if not isinstance(derivative_labels, Tensor) or derivative_labels.shape != (D, len(wrt)) or not derivative_labels.dtype.is_floating_point:
                raise ValueError(f"derivative_labels should be a ({D}, {len(wrt)}) floating-point tensor: one column per variable of "
                                 f"derivative_wrt, but got {tuple(derivative_labels.shape) if isinstance(derivative_labels, Tensor) else derivative_labels!r}")
            lam = torch.as_tensor(derivative_weight, dtype=torch.float64).reshape(-1)
            if lam.numel() == 1:
                lam = lam.expand(len(wrt)).clone()
            if lam.shape != (len(wrt),) or not bool((torch.isfinite(lam) & (lam >= 0)).all()):
                raise ValueError(f"derivative_weight should be a float or ({len(wrt)},) floats, finite and >= 0, but got {derivative_weight!r}")
            self.derivative_weight = lam
        elif derivative_wrt is not None:
            raise ValueError("derivative_wrt needs derivative_labels")
        self._deriv_labelled = len(wrt)
        if sampled_monotonic is not None:
            if self.multigene:
                raise ValueError("multigene cannot be combined with sampled_monotonic: that pass works on single-output trees")
            self._one_label_column("sampled_monotonic")
            variables, bounds, signs = parse_monotonic(sampled_monotonic, num_inputs)
            self.sampled_monotonic = {v: s if s else b for v, b, s in zip(variables, bounds, signs)}
            wrt = wrt + [v for v in variables if v not in wrt]
            self._constrained = True
        if len(wrt) > 8:
            raise ValueError(f"derivative_wrt and sampled_monotonic name {len(wrt)} variables together, but at most 8 are supported")
        self._deriv_wrt = wrt
        if derivative_labels is not None:
            dl = derivative_labels.detach().to(self.datapoints.device).to(torch.float32)
            pad = dl.new_zeros((D, len(wrt) - self._deriv_labelled))
            self.derivative_labels = torch.cat([dl, pad], dim=1).contiguous()

    def derivative_loss(self, forest: Forest):
        """``(loss (pop, 1 + V), violations (pop, V))``: ``Forest.SR_derivative_loss`` on this problem's data, derivative labels and
        ``sampled_monotonic`` bounds, over the variables ``derivative_wrt`` followed by those only ``sampled_monotonic`` names (their
        label is 0).  The raw columns: no weight, no mask"""
        if not self._deriv_wrt:
            raise ValueError("this problem has neither derivative_labels nor sampled_monotonic")
        return forest.SR_derivative_loss(self.datapoints, self.labels, self.derivative_labels, self._deriv_wrt, self.sampled_monotonic)

    def _one_label_column(self, feature: str, claim: str = "works on single-output problems only"):
        if self.labels.dim() != 2 or self.labels.shape[1] != 1:
            raise ValueError(f"{feature} {claim}, but the labels have shape {tuple(self.labels.shape)}")

    def _input_box(self, input_bounds, margin: float):
        """the box of admissible inputs as two float32 ``(num_inputs,)`` tensors"""
        if isinstance(input_bounds, str):
            if input_bounds != "data":
                raise ValueError(f"input_bounds should be 'data' or a (lower, upper) pair, but got {input_bounds!r}")
            x = self.datapoints.detach().to(torch.float32)
            lower, upper = x.min(dim=0).values, x.max(dim=0).values
        else:
            lower, upper = (box_side(b, self.datapoints.shape[1]) for b in input_bounds)
        if margin != 0.0:
            pad = margin * (upper - lower)
            lower, upper = lower - pad, upper + pad
        return lower.cpu(), upper.cpu()   # (Forest.SR_intervals checks the bounds on the host)

    def safe_mask(self, forest: Forest) -> Tensor:
        """(pop,) bool: ``Forest.safe_mask`` on this problem's box"""
        return forest.safe_mask(self.input_lower, self.input_upper)

    def monotone_mask(self, forest: Forest) -> Tensor:
        """(pop,) bool: ``Forest.monotone_mask`` on this problem's box with its ``monotonic`` constraints"""
        if self.monotonic is None:
            raise ValueError("this problem has no monotonic constraints")
        return forest.monotone_mask(self.input_lower, self.input_upper, self.monotonic)

    def dimensions(self, forest: Forest):
        """``(units, flags, violations)``: ``Forest.SR_dimensions`` under this problem's ``input_units`` and ``label_units`` (the
        root is left free under ``linear_scaling``)"""
        if self.input_units is None:
            raise ValueError("this problem has no input_units")
        return forest.SR_dimensions(self.input_units, None if self.linear_scaling else self.label_units)

    def dimension_mask(self, forest: Forest) -> Tensor:
        """(pop,) bool: the tree is dimensionally consistent under this problem's units (``dimensions``: ``violations == 0``)"""
        return self.dimensions(forest)[2] == 0

    def structure(self, forest: Forest):
        """``(complexity, height, depth, nest, flags, violations)``: ``Forest.SR_structure`` under this problem's structural options"""
        if not self._structural:
            raise ValueError("this problem has no structural constraints")
        forest._single_output("structure", ValueError)
        return forest._structure_op(self._structure_tables, self.max_depth, self.max_complexity)

    def structure_mask(self, forest: Forest) -> Tensor:
        """(pop,) bool: the tree obeys this problem's structural constraints (``structure``: ``violations == 0``)"""
        return self.structure(forest)[5] == 0

    def complexity(self, forest: Forest) -> Tensor:
        """(pop,) int32: the complexity of every tree under this problem's ``complexity_of`` (the tree size without it; 0 for a
        malformed row).  The signature ``NSGA2Selection(complexity=)`` takes."""
        forest._single_output("complexity", ValueError)
        return forest._structure_op(self._cost_tables)[0][:, 0]

    def semantic_classes(self, forest: Forest, keep: Optional[str] = None):
        """``(class_id, is_representative)``: ``Forest.semantic_classes`` on this problem's datapoints; ``keep``: None takes the
        problem's ``semantic_keep``.  The signature ``GeneticProgramming(duplicate_classes=)`` takes."""
        return forest.semantic_classes(self.datapoints, self.semantic_keep if keep is None else keep)

    def _masked(self, forest: Forest, fitness: Tensor, fill: float) -> Tensor:
        mask = None
        if self.semantic_dedup:
            mask = self.semantic_classes(forest)[1].to(fitness.device)
        if self._box_check:
            box = self.safe_mask(forest) if self.monotonic is None else self.monotone_mask(forest)   # (the latter holds the former)
            box = box.to(fitness.device)
            mask = box if mask is None else mask & box
        if self.sampled_monotonic is not None:   # (the pass the fitness came from, when derivative_labels is on: one launch for both)
            cols = [self._deriv_wrt.index(v) for v in self.sampled_monotonic]
            pending, self._deriv_pending = self._deriv_pending, None   # what _loss has just computed for this very forest
            viol = pending[1] if pending is not None and pending[0] is forest else self.derivative_loss(forest)[1]
            obeys = (viol[:, cols] == 0).all(1).to(fitness.device)
            mask = obeys if mask is None else mask & obeys
        counted = []   # (violations, penalty) of the passes that count violations
        if self.input_units is not None:
            counted.append((self.dimensions(forest)[2], self.dimension_penalty))
        if self._structural:
            counted.append((self.structure(forest)[5], self.structure_penalty))
        for viol, penalty in counted:
            viol = viol.to(fitness.device)
            if penalty is None:
                ok = viol == 0
            else:   # (a malformed row, -1, is treated as in the hard case)
                ok = viol >= 0
                fitness = torch.where(viol > 0, fitness - penalty * viol.to(fitness.dtype), fitness)
            mask = ok if mask is None else mask & ok
        return torch.where(mask, fitness, torch.full_like(fitness, fill))

    @staticmethod
    def generate_data(func, num_inputs, num_data, lower_bounds, upper_bounds):
        dev = default_device()

        def as_bound(b):
            if isinstance(b, (int, float)):
                return torch.full((num_inputs,), float(b), device=dev)
            return torch.as_tensor(b, dtype=torch.float32, device=dev)

        lo, hi = as_bound(lower_bounds)[None, :], as_bound(upper_bounds)[None, :]
        inputs = torch.rand(num_data, num_inputs, device=dev) * (hi - lo) + lo
        outputs = torch.vmap(func)(inputs)
        if outputs.dim() == 1:
            outputs = outputs[:, None]
        return inputs, outputs

    def scaled_fitness(self, forest: Forest, dedup: Optional[bool] = None):
        """``(loss, slope, intercept)`` of every tree under linear scaling on this problem's data: ``Forest.SR_scaled_fitness``, or
        under ``execute_mode="torch"`` the same definition from ``batch_forward``'s predictions in float64 torch.  ``dedup``: None takes
        the problem's setting.  Under ``scaling_loss="problem"``: ``Forest.SR_weighted_scaled_fitness`` (or its torch twin) on this
        problem's weight rows -- the loss and the coefficients of the training row; the validation column of the same pass goes to
        ``last_validation_loss``"""
        if self._scaling_own:
            return self._weighted_scaled_fitness(forest, dedup)
        if self.execute_mode != "torch":
            return self._slope_checked(*forest.SR_scaled_fitness(self.datapoints, self.labels,
                                                                 dedup=self.dedup if dedup is None else bool(dedup)))
        p = forest.batch_forward(self.datapoints)[:, :, 0]   # (pop, D) float32
        D = p.shape[1]
        y = self.labels.to(p.device)[:, 0].to(torch.float64)
        ybar = y.mean()
        v = y - ybar
        syy = (v * v).sum()
        pd = p.to(torch.float64)
        mean = pd.sum(1) / D
        var = (pd * pd).sum(1) / D - mean * mean
        cov = (pd * v[None, :]).sum(1) / D
        flat = (p.min(1).values == p.max(1).values) | (var <= 0) | (D == 1)
        b = torch.where(flat, torch.zeros_like(var), cov / var)
        a = torch.where(flat, ybar.expand_as(var), ybar - b * mean)
        loss = torch.where(flat, (syy / D).expand_as(var), torch.clamp(syy / D - b * cov, min=0.0))
        loss, a, b = loss.to(torch.float32), a.to(torch.float32), b.to(torch.float32)
        bad = ~torch.isfinite(p).all(1) | ~torch.isfinite(a) | ~torch.isfinite(b)
        nan = torch.full_like(loss, float("nan"))
        return self._slope_checked(torch.where(bad, nan, loss), torch.where(bad, nan, b), torch.where(bad, nan, a))

    def _weighted_scaled_fitness(self, forest: Forest, dedup: Optional[bool], keep_validation: bool = True):
        W = self._loss_weights
        if self.execute_mode != "torch":
            loss, slope, intercept = forest.SR_weighted_scaled_fitness(self.datapoints, self.labels, W,
                                                                       dedup=self.dedup if dedup is None else bool(dedup))
        else:
            loss, slope, intercept = self._weighted_scaling_torch(forest.batch_forward(self.datapoints)[:, :, 0], W)
        if W is None:
            return self._slope_checked(loss, slope, intercept)
        if self.validation_mask is not None and keep_validation:
            self.last_validation_loss = loss[:, 1]
        return self._slope_checked(loss[:, 0].contiguous(), slope, intercept)

    def _weighted_scaling_torch(self, p: Tensor, W: Optional[Tensor]):
        """the definition of ``Forest.SR_weighted_scaled_fitness`` (include/evogp_hip.h evogp_hip_sr_weighted_scaling) on the
        ``(pop, D)`` float32 predictions in two-pass float64 torch: ``(loss (pop, K) or (pop,) without W, slope, intercept)``"""
        dev, f64 = p.device, torch.float64
        y = self.labels.to(dev)[:, 0].to(f64)
        Wd = torch.ones(1, p.shape[1], dtype=f64, device=dev) if W is None else W.to(dev).to(f64)
        zero = torch.zeros((), dtype=f64, device=dev)
        on = Wd != 0                                                    # (K, D): a row without weight is not looked at
        wsum = Wd.sum(1)
        usable = (torch.isfinite(Wd) & (Wd >= 0)).all(1) & (wsum != 0)
        ybar0 = (Wd[0] * y).sum() / wsum[0]
        v = y - ybar0
        vbar = (Wd * v[None, :]).sum(1) / wsum                          # (K,)
        dv = v[None, :] - vbar[:, None]                                 # (K, D)
        V = (Wd * dv * dv).sum(1)
        pd = p.to(f64)
        pz = torch.where(on[None, :, :], pd[:, None, :], zero)          # (pop, K, D)
        m = (Wd[None] * pz).sum(2) / wsum[None, :]                      # (pop, K)
        dp = torch.where(on[None, :, :], pd[:, None, :] - m[:, :, None], zero)
        M = (Wd[None] * dp * dp).sum(2)
        c = (Wd[None] * dp * dv[None]).sum(2)
        inf = torch.full((), float("inf"), dtype=p.dtype, device=dev)
        mn = torch.where(on[0][None, :], p, inf).min(1).values
        mx = torch.where(on[0][None, :], p, -inf).max(1).values
        flat = (mn == mx) | (M[:, 0] <= 0) | (on[0].sum() == 1)
        b = torch.where(flat, zero, c[:, 0] / M[:, 0])
        a = torch.where(flat, ybar0 + vbar[0], ybar0 + vbar[0] - b * m[:, 0])
        delta = b[:, None] * (m - m[:, :1]) - (vbar - vbar[0])[None, :]
        num = b[:, None] ** 2 * M - 2.0 * b[:, None] * c + V[None, :] + wsum[None, :] * delta * delta
        num[:, 0] = V[0] - b * c[:, 0]
        loss = (torch.where(num < 0, zero, num) / wsum[None, :]).to(torch.float32)
        af, bf = a.to(torch.float32), b.to(torch.float32)
        bad = (on[None, :, :] & ~torch.isfinite(p)[:, None, :]).any(2)  # (pop, K)
        dead = bad[:, 0] | ~usable[0] | ~torch.isfinite(af) | ~torch.isfinite(bf)
        nan = float("nan")
        loss = torch.where(dead[:, None] | bad | ~usable[None, :], torch.full_like(loss, nan), loss)
        af, bf = torch.where(dead, torch.full_like(af, nan), af), torch.where(dead, torch.full_like(bf, nan), bf)
        return (loss[:, 0] if W is None else loss), bf, af

    def _slope_checked(self, loss: Tensor, slope: Tensor, intercept: Tensor):
        """under a +-1 ``monotonic`` constraint a negative slope turns the proven direction round: such a tree fails (NaN loss)"""
        if self._sign_constrained:
            loss = torch.where(slope < 0, torch.full_like(loss, float("nan")), loss)
        return loss, slope, intercept

    def scaled(self, forest: Forest, dedup: Optional[bool] = None) -> Forest:
        """``forest`` with every tree T rewritten as ``intercept + slope * T`` for its own least-squares coefficients on this problem's
        data (``Forest.apply_scaling`` with ``grow=True``: rows four words longer, at most 1024); under ``scaling_loss="problem"`` the
        coefficients fitted on the training weight row (``last_validation_loss`` is left as it is)"""
        if self._scaling_own:
            _, slope, intercept = self._weighted_scaled_fitness(forest, dedup, keep_validation=False)
        else:
            _, slope, intercept = self.scaled_fitness(forest, dedup)
        return forest.apply_scaling(slope, intercept, grow=True)[0]

    def _check_scaling(self, use_MSE: bool):
        if not use_MSE:
            raise ValueError(f"{'multigene' if self.multigene else 'linear_scaling'} minimises the mean squared error: use_MSE must be True")

    def gene_model(self, forest: Forest, dedup: Optional[bool] = None):
        """``(loss (pop,), coef (pop, 1 + G))`` of every tree as a multi-gene model on this problem's data: ``Forest.SR_gene_fitness``,
        or under ``execute_mode="torch"`` the same definition from ``batch_forward``'s outputs in float64 torch (which materialises
        them).  ``dedup``: None takes the problem's setting"""
        if self.execute_mode != "torch":
            return forest.SR_gene_fitness(self.datapoints, self.labels, dedup=self.dedup if dedup is None else bool(dedup))
        g32 = forest.batch_forward(self.datapoints)   # (pop, D, G) float32
        pop, D, G = g32.shape
        g = g32.to(torch.float64)
        y = self.labels.to(g.device)[:, 0].to(torch.float64)
        ybar = y.mean()
        v = y - ybar
        syy_D = (v * v).sum() / D
        m = g.mean(1)
        gc = g - m[:, None, :]
        C = torch.einsum("pdi,pdj->pij", gc, gc) / D
        c = torch.einsum("pdi,d->pi", gc, v) / D
        var = torch.diagonal(C, dim1=1, dim2=2)
        flat = (g32.min(1).values == g32.max(1).values) | (var <= 0) | (D == 1)
        # the LDL^T of the definition, gene by gene over the whole population: a dropped gene keeps an identity row
        Lm = torch.zeros_like(C)
        dd = torch.ones_like(m)
        kept = torch.zeros_like(flat)
        for j in range(G):
            dj = var[:, j].clone()
            for k in range(j):
                a = C[:, k, j].clone()
                for q in range(k):
                    a = a - Lm[:, j, q] * Lm[:, k, q] * dd[:, q]
                l = torch.where(kept[:, k], a / dd[:, k], torch.zeros_like(a))
                Lm[:, j, k] = l
                dj = dj - l * l * dd[:, k]
            kept[:, j] = ~flat[:, j] & (dj > 2.0 ** -30 * var[:, j])
            dd[:, j] = torch.where(kept[:, j], dj, torch.ones_like(dj))
            Lm[:, j, :j] = torch.where(kept[:, j, None], Lm[:, j, :j], torch.zeros_like(Lm[:, j, :j]))
        w = torch.where(kept, c, torch.zeros_like(c))
        for j in range(G):
            for k in range(j):
                w[:, j] = w[:, j] - Lm[:, j, k] * w[:, k]
        w = w / dd
        for j in range(G - 1, -1, -1):
            for i in range(j + 1, G):
                w[:, j] = w[:, j] - Lm[:, i, j] * w[:, i]
        w = torch.where(kept, w, torch.zeros_like(w))
        b0 = ybar - (w * m).sum(1)
        loss = torch.clamp(syy_D - (w * c).sum(1), min=0.0)
        coef = torch.cat([b0[:, None], w], dim=1).to(torch.float32)
        bad = ~torch.isfinite(g32).all(2).all(1) | ~torch.isfinite(coef).all(1)
        nan = float("nan")
        return (torch.where(bad, torch.full_like(loss, nan), loss).to(torch.float32),
                torch.where(bad[:, None], torch.full_like(coef, nan), coef))

    def weighted_loss(self, forest: Forest, loss: str, dedup: Optional[bool] = None) -> Tensor:
        """``Forest.SR_weighted_loss`` on this problem's data with its ``loss_param`` and weight rows -- ``(pop,)``, or ``(pop, 2)``
        under a ``validation_mask``: training rows, validation rows -- or under ``execute_mode="torch"`` the same definition from
        ``batch_forward``'s predictions in float64 torch (which materialises them)"""
        W = self._loss_weights
        if self.execute_mode != "torch":
            return forest.SR_weighted_loss(self.datapoints, self.labels, W if W is None or W.shape[0] > 1 else W[0], loss,
                                           self.loss_param, dedup=self.dedup if dedup is None else bool(dedup))
        p = forest.batch_forward(self.datapoints)[:, :, 0]   # (pop, D) float32
        r = p.to(torch.float64) - self.labels.to(p.device)[:, 0].to(torch.float64)[None, :]
        a, prm = r.abs(), self.loss_param
        if loss == "mse":
            rho = r * r
        elif loss == "mae":
            rho = a
        elif loss == "huber":
            rho = torch.where(a <= prm, r * r * 0.5, prm * (a - prm * 0.5))
        elif loss == "pinball":
            rho = torch.where(-r >= 0, prm * -r, (prm - 1.0) * -r)
        else:
            rho = a + torch.log1p(torch.exp(-2.0 * a)) - 0.6931471805599453
        Wd = torch.ones(1, p.shape[1], dtype=torch.float64, device=p.device) if W is None else W.to(p.device).to(torch.float64)
        on = (Wd != 0)[None, :, :]   # a row without weight is not looked at
        s = torch.where(on, Wd[None, :, :] * rho[:, None, :], torch.zeros((), dtype=torch.float64, device=p.device)).sum(2)
        bad = (on & ~torch.isfinite(p)[:, None, :]).any(2)
        wsum = Wd.sum(1)
        usable = (torch.isfinite(Wd) & (Wd >= 0)).all(1) & (wsum != 0)
        out = torch.where(bad | ~usable[None, :], torch.full_like(s, float("nan")), s / wsum[None, :]).to(torch.float32)
        return out[:, 0] if W is None or W.shape[0] == 1 else out

    def validation_scores(self, forest: Forest, scores: Optional[Tensor] = None) -> Tensor:
        """(pop,): minus the loss of every tree on the rows ``validation_mask`` holds out, -inf where it is NaN and wherever the
        tree's training score is -inf (a tree that fails a constraint is no candidate on any rows).  ``scores``: None scores the
        forest here; or what ``scores(forest)`` has just returned, and the validation column of that same pass is taken."""
        if self.validation_mask is None:
            raise ValueError("this problem has no validation_mask")
        train = self.scores(forest) if scores is None else scores
        held = self.last_validation_loss.to(train.device)
        out = torch.where(torch.isnan(held), torch.full_like(held, float("-inf")), -held)
        return torch.where(train == float("-inf"), torch.full_like(out, float("-inf")), out)

    def _loss(self, forest: Forest, use_MSE: bool):
        """``(loss, on_device)``: the positive loss of every tree under this problem's model, and whether a HIP pass over a device
        forest computed it (``scores`` then finishes it in one launch)"""
        on_device = self.execute_mode != "torch" and forest.batch_node_value.is_cuda
        if self.derivative_labels is not None:
            if not use_MSE:
                raise ValueError("derivative_labels minimises squared errors: use_MSE must be True")
            cols, viol = self.derivative_loss(forest)
            self._deriv_pending = (forest, viol) if self.sampled_monotonic is not None else None   # (_masked takes it: one pass for both)
            lam = self.derivative_weight.to(cols.device).to(cols.dtype)
            return cols[:, 0] + (cols[:, 1:1 + self._deriv_labelled] * lam[None, :]).sum(1), on_device
        if self._scaling_own:
            self._check_scaling(use_MSE)
            return self.scaled_fitness(forest)[0], on_device
        if self._own_loss:
            if self.loss is not None and not use_MSE:
                raise ValueError(f"this problem's loss is {self.loss!r}: use_MSE must be left True")
            out = self.weighted_loss(forest, self.loss or ("mse" if use_MSE else "mae"))
            if self.validation_mask is None:
                return out, on_device
            self.last_validation_loss = out[:, 1]
            return out[:, 0].contiguous(), on_device
        if self.multigene or self.linear_scaling:
            self._check_scaling(use_MSE)
            return (self.gene_model(forest) if self.multigene else self.scaled_fitness(forest))[0], on_device
        if self.execute_mode == "torch":
            pred = forest.batch_forward(self.datapoints)  # (pop, D, out)
            err = pred - self.labels[None, :, :]
            # mean over datapoints AND outputs, as the reference's torch mode (symbolic_regression.py:76-80)
            return torch.mean(err**2 if use_MSE else err.abs(), dim=(1, 2)), False
        return forest.SR_fitness(self.datapoints, self.labels, use_MSE, self.execute_mode), on_device

    def evaluate(self, forest: Forest, use_MSE: bool = True) -> Tensor:
        fitness = -self._loss(forest, use_MSE)[0]
        return self._masked(forest, fitness, float("nan")) if self._constrained else fitness

    def scores(self, forest: Forest, use_MSE: bool = True) -> Tensor:
        """``evaluate`` with the NaN entries already at -inf (what StandardPipeline.step makes of them, pipeline/standard.py:41-43):
        on the device the sign and the scrub are ONE launch behind the fitness pass instead of four torch launches"""
        loss, on_device = self._loss(forest, use_MSE)
        if on_device:
            fitness = torch.ops.evogp_hip.fitness_scores(loss, True)
        else:
            fitness = torch.where(torch.isnan(loss), torch.full_like(loss, float("-inf")), -loss)
        return self._masked(forest, fitness, float("-inf")) if self._constrained else fitness

    def optimize(self, forest: Forest, use_MSE: bool = True) -> Forest:
        """``forest`` simplified (``Forest.simplify``, on every ``simplify_every``-th call) and then with its constants tuned by
        ``const_opt_steps`` steps of ``Forest.optimize_constants`` on this dataset (the forest itself when both are 0).  In front of
        both, on every ``intron_removal_every``-th call, the forest without its semantic introns (``Forest.remove_introns``)."""
        if self.intron_removal_every > 0:
            self._intron_calls += 1
            if self._intron_calls % self.intron_removal_every == 0:
                forest = forest.remove_introns(self.datapoints, dedup=self.dedup)[0]
        if self.simplify_every > 0:
            self._optimize_calls += 1
            if self._optimize_calls % self.simplify_every == 0:
                forest = forest.simplify(self.datapoints, self.labels, use_MSE, dedup=self.dedup)[0]
        if self.const_opt_steps <= 0:
            return forest
        own = {}
        if self.const_opt_loss == "problem" and self._own_loss:   # the loss the trees are scored by, on the rows they are scored on
            W = self._loss_weights
            own = dict(weights=None if W is None else W[0], loss=self.loss, param=self.loss_param)   # (no loss: what use_MSE says)
        return forest.optimize_constants(self.datapoints, self.labels, self.const_opt_steps, self.const_step_size, use_MSE,
                                         method=self.const_opt_method, dedup=self.dedup, **own)[0]

    @property
    def problem_dim(self):
        return self.datapoints.shape[1]

    @property
    def solution_dim(self):
        return self.labels.shape[1]
