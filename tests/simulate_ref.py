"""TEST-ONLY: the definition of the simulation ops (include/evogp_hip.h, evogp_hip_sr_simulate) restated in numpy float32, on top of ANY
evaluator of one input row per tree -- ``Forest.forward`` on the device (tests/test_gpu_simulate.py), the C oracle's ``evaluate`` on the
CPU (tests/test_simulate_ref.py).  The evaluator is called once per (trajectory, step, stage): nothing here knows the kernel.

``f(rows)``: float32 ``(pop, S + U)`` -> ``(pop, S)`` (``(pop, 1)`` for narx).  Every operation is one numpy float32 operation: rounded separately."""
import numpy as np

F = np.float32


def step(f, x, u, scheme, dt):
    """one step of every tree: x float32 (pop, S), u float32 (U,) -> x+ float32 (pop, S)"""
    dt = F(dt)
    rows = lambda s: np.concatenate([s, np.broadcast_to(u, (len(s), len(u)))], 1).astype(F)  # noqa: E731
    with np.errstate(all="ignore"):
        if scheme == "map":
            return f(rows(x))
        if scheme == "euler":
            return x + dt * f(rows(x))
        if scheme == "narx":
            return np.concatenate([f(rows(x))[:, :1], x[:, :-1]], 1)
        h2, h6 = F(dt * F(0.5)), F(dt / F(6))
        k1 = f(rows(x))
        k2 = f(rows(x + h2 * k1))
        k3 = f(rows(x + h2 * k2))
        k4 = f(rows(x + dt * k3))
        return x + h6 * (((k1 + F(2) * k2) + F(2) * k3) + k4)


def simulate(f, pop, x0, u, scheme, dt, malformed=None):
    """states float32 (pop, B, T, S): x0 (B, S), u (B, T, U).  A trajectory dies at the first step whose new state has a component that is
    not finite: NaN from that step on.  ``malformed`` bool (pop,): those trees are NaN everywhere."""
    B, S = x0.shape
    T = u.shape[1]
    out = np.full((pop, B, T, S), np.nan, F)
    for b in range(B):
        x = np.broadcast_to(x0[b], (pop, S)).astype(F)
        alive = np.ones(pop, bool) if malformed is None else ~malformed
        for t in range(T):
            x = step(f, x, u[b, t], scheme, dt).astype(F)
            alive &= np.isfinite(x).all(1)
            out[alive, b, t] = x[alive]
    return out


def loss(states, target, narx=False):
    """longdouble (pop, S) ((pop, 1) for narx): the mean of (x - target)^2 over b and t; NaN for a tree with a NaN state"""
    x = states[..., :1] if narx else states
    y = target[..., None] if narx else target
    d = x.astype(np.longdouble) - y.astype(np.longdouble)[None]
    with np.errstate(all="ignore"):
        out = (d * d).sum((1, 2)) / np.longdouble(states.shape[1] * states.shape[2])
    out[np.isnan(states).any((1, 2, 3))] = np.nan
    return out
