"""CPU: the restated definition of the simulation ops (tests/simulate_ref.py) against a truth that does not descend from the kernel -- the
same scheme in float64 numpy on the same float32 constants -- with the C oracle's evaluator in place of ``Forest.forward``;
tests/test_gpu_simulate.py then ties the kernel to the restatement bit for bit."""
import os
import sys

import numpy as np
import pytest

import evogp_amd  # noqa: F401  (defines the schemas)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simulate_ref as SIM  # noqa: E402
import simulate_tables  # noqa: E402,F401  (the ops' rows of the invariance and binding tables exist in every collection)
from helpers import the_oracle  # noqa: E402
from semantic_cases import X0, plant  # noqa: E402

T, DT = 17, np.float32(0.1)
# roundings of one step of the pinned formula, the tree's own value counted as one:
#   map     f                                                                                   1
#   euler   f, dt * f, x + .                                                                    3
#   rk4     k1; (h * k, x + ., f) for k2, k3, k4 = 9; 2 * k2, + , 2 * k3, +, + k4 = 5; h6 * ., x + . = 2      17
ROUNDINGS = {"map": 1, "euler": 3, "rk4": 17}


def _truth64(scheme, x):
    """one step of the scheme in float64 on the float32 constants: the law is 0.9 x (map) or -x"""
    c, dt = np.float64(np.float32(0.9)), np.float64(DT)
    h2, h6 = np.float64(np.float32(DT * np.float32(0.5))), np.float64(np.float32(DT / np.float32(6)))
    if scheme == "map":
        return c * x
    if scheme == "euler":
        return x + dt * -x
    k1 = -x
    k2 = -(x + h2 * k1)
    k3 = -(x + h2 * k2)
    k4 = -(x + dt * k3)
    return x + h6 * (((k1 + 2 * k2) + 2 * k3) + k4)


@pytest.mark.parametrize("scheme", ["map", "euler", "rk4"])
def test_restatement_against_float64_on_contractive_linear_laws(scheme):
    """allowed: ROUNDINGS[scheme] * (t + 1) * 2^-24 relative after step t (the count above; the laws contract, so no error of an
    earlier step grows).  Worst measured error / bound: map 0.75, euler 0.19, rk4 0.042."""
    f = [np.zeros((1, 8), np.float32), np.zeros((1, 8), np.int16), np.zeros((1, 8), np.int16)]
    plant(*f, 0, ("mul", ("c", np.float32(0.9)), X0) if scheme == "map" else ("neg", X0))
    oracle = the_oracle()
    x0 = np.random.default_rng(5).uniform(0.5, 1.5, (7, 1)).astype(np.float32)
    got = SIM.simulate(lambda rows: oracle.evaluate(*f, rows, 1), 1, x0, np.zeros((7, T, 0), np.float32), scheme, DT)[0, :, :, 0]
    x, worst = x0[:, 0].astype(np.float64), 0.0
    for t in range(T):
        x = _truth64(scheme, x)
        ratio = np.abs(got[:, t] - x) / (ROUNDINGS[scheme] * (t + 1) * 2.0 ** -24 * np.abs(x))
        worst = max(worst, float(ratio.max()))
        assert (ratio <= 1).all(), (scheme, t, ratio.max())
    print(f"{scheme}: worst error / bound {worst:.3g}")
