"""DynamicalSystem — system identification and forecasting (no counterpart in the reference): the tree is the law of motion,
``x_{t+1} = f(x_t, u_t)``, ``dx/dt = f(x, u)`` or a NARX forecaster, and it is scored by its FREE-RUN trajectory: fed its own output for
``T`` steps and compared with the measured series, in ONE kernel for the whole population (``Forest.SR_simulation_loss``,
csrc/sr_simulate.hip).  A one-step fit (``SymbolicRegression``) looks fine and then drifts or blows up in simulation;
this fitness is the simulation.

``evaluate`` returns ``-sum_s loss_s / state_scale_s``: the per-state mean squared errors, each in units of that state's scale (default:
the variance of ``target`` over trajectories and steps, so that a state measured in volts and one in millivolts weigh the same).  Larger
is better, as everywhere; a tree whose simulation dies (a state that is not finite) or that is malformed scores ``-inf``."""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from ..tree import Forest
from .base import BaseProblem


def simulation_fitness(loss: Tensor, state_scale: Tensor) -> Tensor:
    """``-sum_s loss[:, s] / state_scale[s]`` as float32; NaN (a dead trajectory, a malformed tree) scores ``-inf``"""
    score = -(loss / state_scale.to(loss.dtype)).sum(1)
    return torch.where(torch.isnan(score), torch.full_like(score, float("-inf")), score).to(torch.float32)


class DynamicalSystem(BaseProblem):
    """``x0`` ``(B, S)``, ``u`` ``(B, T, U)`` or None, ``target`` ``(B, T, S)`` (``(B, T)`` for ``scheme="narx"``), ``scheme`` one of
    ``"map"``, ``"euler"``, ``"rk4"``, ``"narx"``, ``dt`` the step; ``state_scale``: ``(S,)`` positive scales (one for ``"narx"``), default
    the per-state variance of ``target`` (1 where that is 0).  The forest has ``input_len = S + U`` and ``output_len = S`` (1 for narx)."""

    def __init__(self, x0: Tensor, u: Optional[Tensor], target: Tensor, scheme: str = "euler", dt: float = 1.0, state_scale=None,
                 const_opt_steps: int = 0):
        """``const_opt_steps`` > 0: ``optimize`` -- which ``StandardPipeline`` calls in front of every evaluation -- tunes every tree's
        constants by that many Levenberg-Marquardt steps under this fitness (``optimize_constants``); the tuned forest is scored and bred"""
        assert const_opt_steps >= 0, f"const_opt_steps should be >= 0, but got {const_opt_steps}"
        self.const_opt_steps = int(const_opt_steps)
        self.x0, self.u, self.target, self.scheme, self.dt = x0, u, target, scheme, float(dt)
        if x0.dim() != 2 or target.dim() != (2 if scheme == "narx" else 3) or target.shape[0] != x0.shape[0]:
            raise ValueError(f"x0 should be (B, S) and target (B, T{'' if scheme == 'narx' else ', S'}), but got {tuple(x0.shape)} and {tuple(target.shape)}")
        cols = target.reshape(-1, 1 if scheme == "narx" else target.shape[-1]).to(torch.float64)
        if state_scale is None:
            var = cols.var(0, unbiased=False)
            state_scale = torch.where(var > 0, var, torch.ones_like(var))
        state_scale = torch.as_tensor(state_scale, dtype=torch.float64, device=target.device).reshape(-1)
        if state_scale.shape[0] != cols.shape[1] or not bool((state_scale > 0).all()):
            raise ValueError(f"state_scale should hold {cols.shape[1]} positive scales, but got {state_scale.tolist()}")
        self.state_scale = state_scale

    @staticmethod
    def from_series(series: Tensor, inputs: Optional[Tensor], window: int, stride: int = 1, scheme: str = "euler", dt: float = 1.0,
                    state_scale=None, lags: int = 1, const_opt_steps: int = 0) -> "DynamicalSystem":
        """Multiple shooting: ONE long recording ``series`` ``(N, S)`` (``(N,)`` for narx) with its inputs ``(N, U)`` or None is cut into
        overlapping windows of ``window`` steps, one every ``stride`` samples; each window starts a trajectory from the measured state
        and is compared with the ``window`` samples that follow.  (The windows are also what fills the 64 lanes of the kernel's tiles.)
        narx: the start state is the last ``lags`` samples, newest first.  ``u[:, t]`` is the input at the sample the step starts from."""
        narx = scheme == "narx"
        if series.dim() != (1 if narx else 2):
            raise ValueError(f"series should be {'(N,)' if narx else '(N, S)'}, but got {tuple(series.shape)}")
        first = lags - 1 if narx else 0
        n = series.shape[0]
        if window < 1 or stride < 1 or lags < 1 or first + window >= n:
            raise ValueError(f"a window of {window} steps (stride {stride}, lags {lags}) does not fit a series of {n} samples")
        starts = torch.arange(first, n - window, stride, device=series.device)
        steps = starts[:, None] + torch.arange(window, device=series.device)[None, :]
        if narx:
            x0 = series[starts[:, None] - torch.arange(lags, device=series.device)[None, :]]
        else:
            x0 = series[starts]
        target = series[steps + 1]
        u = None if inputs is None else inputs[steps]
        return DynamicalSystem(x0.contiguous(), u, target.contiguous(), scheme, dt, state_scale, const_opt_steps=const_opt_steps)

    def losses(self, forest: Forest) -> Tensor:
        """``(pop, S)`` float64: the per-state free-run mean squared errors, NaN where the simulation died"""
        return forest.SR_simulation_loss(self.x0, self.u, self.target, self.scheme, self.dt)

    def evaluate(self, forest: Forest) -> Tensor:
        return simulation_fitness(self.losses(forest), self.state_scale)

    def optimize_constants(self, forest: Forest, steps: int = 3, damping: float = 1e-3):
        """``(forest, loss)``: ``Forest.optimize_simulation_constants`` on this problem's data with ``state_weight = 1 / state_scale``, so
        the loss that is lowered, float32 ``(pop,)``, is minus ``evaluate``'s fitness (NaN where that is ``-inf``)"""
        return forest.optimize_simulation_constants(self.x0, self.u, self.target, self.scheme, self.dt, steps, damping,
                                                    (1.0 / self.state_scale).to(torch.float32))

    def optimize(self, forest: Forest) -> Forest:
        """the forest with its constants tuned by ``const_opt_steps`` steps (the forest itself when that is 0)"""
        return forest if self.const_opt_steps <= 0 else self.optimize_constants(forest, self.const_opt_steps)[0]

    @property
    def problem_dim(self):
        return self.x0.shape[1] + (0 if self.u is None else self.u.shape[2])

    @property
    def solution_dim(self):
        return 1 if self.scheme == "narx" else self.x0.shape[1]
