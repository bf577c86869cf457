"""TEST-ONLY: the two planted problems of tuning under the problem's own loss, shared by the CPU suite (tests/test_wtune_host.py, on the
float64 reference behind the CPU stand-in ops) and the GPU suite (tests/test_gpu_wtune.py, on the device): held-out rows that must not
reach the tuner, and outliers that a robust loss must resist.  The model is c1 * x0 + c2 with (c1, c2) = (2.5, 0.7), started at (1, 1),
on D = 96 rows; a forest of POP copies goes through StandardPipeline.step, whose best tree carries the tuned constants."""
import math

import numpy as np
import torch

import sr_grad_ref as R

D, POP, GP_LEN = 96, 8, 32
TARGET = np.array([2.5, 0.7])
BOUND = 1e-3   # |c - c*|: the bound of test_planted_linear_problem_in_five_steps (tests/test_gpu_sr_lm.py)

# The float64 reference (weighted_grad_ref.lm_optimize on the training rows, started at (1, 1)) first meets BOUND after
# HELD_OUT_REFERENCE_STEPS steps (tests/test_wtune_host.py::test_reference_step_count checks this number); the code under test gets
# half as many again for accept / reject decisions that fall the other way in fp32: the rule above test_planted_sine_problem.
HELD_OUT_REFERENCE_STEPS = 2
HELD_OUT_STEPS = math.ceil(1.5 * HELD_OUT_REFERENCE_STEPS)
ROBUST_STEPS = 40   # descent steps of the robust comparison: the same number under both losses


def planted_arrays(pop=POP):
    value = np.zeros((pop, GP_LEN), np.float32)
    type_ = np.zeros((pop, GP_LEN), np.int16)
    size = np.zeros((pop, GP_LEN), np.int16)
    value[:, :5] = [R.F_ADD, R.F_MUL, 1.0, 0, 1.0]
    type_[:, :5] = [R.T_BFUNC, R.T_BFUNC, R.T_CONST, R.T_VAR, R.T_CONST]
    size[:, :5] = [5, 3, 1, 1, 1]
    return value, type_, size


def _rows():
    rng = np.random.default_rng(20261020)
    X = rng.uniform(-1, 1, (D, 1)).astype(np.float32)
    return rng, X, (TARGET[0] * X + TARGET[1]).astype(np.float32)


def held_out_data():
    """``(X, y, mask)``: one third of the rows held out (every third row), their labels moved by +100"""
    _, X, y = _rows()
    mask = np.arange(D) % 3 == 1
    y[mask] += 100.0
    return X, y, mask


def robust_data():
    """``(X, y)``: 5 % of the labels (5 of 96) moved by +50"""
    rng, X, y = _rows()
    y[rng.choice(D, 5, replace=False)] += 50.0
    return X, y


def tuned_constants(device, X, y, **problem):
    """(c1, c2) of the best tree after ONE StandardPipeline.step on a forest of copies of the planted tree under
    ``SymbolicRegression(datapoints=X, labels=y, **problem)``"""
    from evogp_amd.algorithm import DefaultCrossover, DefaultMutation, DefaultSelection, GeneticProgramming
    from evogp_amd.pipeline import StandardPipeline
    from evogp_amd.problem import SymbolicRegression
    from evogp_amd.tree import Forest, GenerateDescriptor

    d = GenerateDescriptor(max_tree_len=GP_LEN, input_len=1, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=3,
                           const_samples=[-1, 0.5, 1])
    forest = Forest(1, 1, *(torch.from_numpy(a).to(device) for a in planted_arrays()))
    problem = {k: v.to(device) if isinstance(v, torch.Tensor) else v for k, v in problem.items()}
    prob = SymbolicRegression(datapoints=torch.from_numpy(X).to(device), labels=torch.from_numpy(y).to(device), **problem)
    algo = GeneticProgramming(forest, DefaultCrossover(), DefaultMutation(0.2, d), DefaultSelection(0.3, 2))
    pipe = StandardPipeline(algo, prob, generation_limit=1, is_show_details=False)
    pipe.step()
    c = pipe.best_tree.node_value.detach().cpu().numpy()
    return np.array([c[2], c[4]], np.float64)


def distance(c):
    return float(np.max(np.abs(np.asarray(c, np.float64) - TARGET)))
