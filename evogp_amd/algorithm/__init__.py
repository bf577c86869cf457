"""evogp_amd.algorithm — genetic operators (reference: src/evogp/algorithm/): the default set, the rank / roulette /
tournament / truncation selections, epsilon-lexicase selection over per-case errors and NSGA-II selection on (error, complexity) (no counterpart in
the reference), the diversity and leaf-biased crossovers, the structural and point mutations, the semantic-backpropagation mutation
and the approximately geometric semantic crossover over one shared library, and semantic mate selection over pairwise moments (no
counterpart in the reference)."""
from .selection import (BaseSelection, BaseSelector, DefaultSelection, LexicaseSelection, NSGA2Selection, RankSelection, RankSelector, RouletteSelection,
                        RouletteSelector, TournamentSelection, TournamentSelector, TruncationSelection, TruncationSelector, lexicase_epsilon)
from .crossover import ApproxGeometricCrossover, BaseCrossover, CombinedDefaultCrossover, DefaultCrossover, DiversityCrossover, LeafBiasedCrossover, SemanticMateCrossover
from .mutation import (BaseMutation, CombinedDefaultMutation, CombinedMutation, DefaultMutation, DeleteMutation, HoistMutation, InsertMutation,
                       MultiConstMutation, MultiPointMutation, SemanticBackpropMutation, SingleConstMutation, SinglePointMutation)
from .semantic_library import SemanticLibrary
from .semantic_mate import SemanticMate
from .genetic_programming import GeneticProgramming, ParetoFront

__all__ = ["BaseSelection", "DefaultSelection", "RankSelection", "RouletteSelection", "TournamentSelection",
           "TruncationSelection", "LexicaseSelection", "lexicase_epsilon", "NSGA2Selection", "BaseSelector", "RankSelector", "RouletteSelector", "TournamentSelector",
           "TruncationSelector", "BaseCrossover", "DefaultCrossover", "DiversityCrossover", "LeafBiasedCrossover", "BaseMutation",
           "DefaultMutation", "HoistMutation", "InsertMutation", "DeleteMutation", "SinglePointMutation",
           "MultiPointMutation", "SingleConstMutation", "MultiConstMutation", "CombinedMutation", "CombinedDefaultCrossover",
           "CombinedDefaultMutation", "SemanticBackpropMutation", "ApproxGeometricCrossover", "SemanticLibrary", "SemanticMate", "SemanticMateCrossover", "GeneticProgramming",
           "ParetoFront"]
