"""evogp_amd.problem — fitness evaluation front ends (reference: src/evogp/problem/)."""
from .base import BaseProblem
from .symbolic_regression import SymbolicRegression
from .classification import Classification
from .transformation import Transformation
from .custom_loss import CustomLoss
from .rank_fitness import RankFitness
from .niching import NichedFitness
from .dynamics import DynamicalSystem
from .rollout import LinearTrackingEnv, PendulumEnv, RolloutProblem

__all__ = ["BaseProblem", "DynamicalSystem", "SymbolicRegression", "Classification", "Transformation", "CustomLoss", "RankFitness", "NichedFitness", "RolloutProblem", "LinearTrackingEnv", "PendulumEnv"]
