"""StandardPipeline — evaluate, track the best tree, evolve; stop on a fitness target, a time limit
or a generation limit (src/evogp/pipeline/standard.py:11-106)."""
from __future__ import annotations

import time

import torch

from ..algorithm import GeneticProgramming
from ..problem import BaseProblem


class BasePipeline:
    def step(self):
        raise NotImplementedError

    def run(self):
        raise NotImplementedError


class StandardPipeline(BasePipeline):
    def __init__(self, algorithm: GeneticProgramming, problem: BaseProblem, fitness_target: float = None,
                 generation_limit: int = 100, time_limit: int = None, is_show_details: bool = True,
                 valid_fitness_boundry: float = 1e8, validation_patience: int = None):
        """``validation_patience`` (a problem with a ``validation_mask`` only): ``run`` stops after that many consecutive generations
        without a new best validation fitness and returns ``best_validation_tree``, not ``best_tree``"""
        self.algorithm = algorithm
        self.problem = problem
        self.fitness_target = fitness_target
        self.generation_limit = generation_limit
        self.time_limit = time_limit
        self.is_show_details = is_show_details
        self.valid_fitness_boundry = valid_fitness_boundry
        self.best_tree = None
        self.best_fitness = float("-inf")
        self.best_coef = None   # a multigene problem: the (1 + G,) coefficients of best_tree's model, on the host
        self.fitness = None
        if validation_patience is not None:
            if getattr(problem, "validation_mask", None) is None:
                raise ValueError("validation_patience needs a problem with a validation_mask")
            if isinstance(validation_patience, bool) or not isinstance(validation_patience, int) or validation_patience < 1:
                raise ValueError(f"validation_patience should be None or an int >= 1, but got {validation_patience!r}")
        self.validation_patience = validation_patience
        if getattr(problem, "validation_mask", None) is not None:
            # the tree with the highest score on the held-out rows among the trees whose training score is finite (the smaller index
            # wins a tie), and the generations since it last changed
            self.best_validation_tree = None
            self.best_validation_fitness = float("-inf")
            self.validation_stale = 0

    def step(self):
        """One generation.  Same result as the reference's loop (standard.py:41-52), but nothing waits on the device
        before the whole generation is enqueued: the NaN scrub is a select instead of a boolean-mask assignment (which
        hides a host sync), and the fitness vector is brought to the host AFTER ``algorithm.step`` has queued the
        selection / breeding kernels, so the copy overlaps them instead of idling the GPU."""
        # Lamarckian constant tuning / simplification: the optimised trees are scored and bred
        if (getattr(self.problem, "const_opt_steps", 0) > 0 or getattr(self.problem, "simplify_every", 0) > 0
                or getattr(self.problem, "intron_removal_every", 0) > 0):
            self.algorithm.forest = self.problem.optimize(self.algorithm.forest)
        forest = self.algorithm.forest  # step() builds a new forest; the best tree comes from this one
        scores = getattr(self.problem, "scores", None)
        if scores is not None:   # (a problem that hands over the scrubbed fitness itself: SymbolicRegression, one launch)
            fitness = scores(forest)
        else:
            fitness = self.problem.evaluate(forest)
            fitness = torch.where(torch.isnan(fitness), torch.full_like(fitness, float("-inf")), fitness)  # standard.py:43
        self.algorithm.step(fitness)
        if getattr(self.problem, "validation_mask", None) is not None:
            held = self.problem.validation_scores(forest, fitness).cpu()   # (the validation column of the pass behind `fitness`)
            top = held.max()
            self.validation_stale += 1
            if top > self.best_validation_fitness:
                self.best_validation_fitness = top
                first = int(torch.nonzero(held == top)[0])
                if getattr(self.problem, "linear_scaling", False):
                    # as best_tree below: the model whose held-out error is stated, the tree with its TRAIN-fitted coefficients written in
                    self.best_validation_tree = self.problem.scaled(forest[first:first + 1], dedup=False)[0]
                else:
                    self.best_validation_tree = forest[first]
                self.validation_stale = 0
        host = fitness.cpu()
        best = int(torch.argmax(host))
        if host[best] > self.best_fitness:
            self.best_fitness = host[best]
            if getattr(self.problem, "linear_scaling", False):
                # the reported tree is the model whose error the fitness states: the tree with its slope and intercept written in
                self.best_tree = self.problem.scaled(forest[best:best + 1], dedup=False)[0]   # (one tree: nothing to deduplicate)
            elif getattr(self.problem, "multigene", False):
                # the weights cannot be written into the tree (an OUT node hands its operand on, not its result): they go next to it
                self.best_tree = forest[best]
                self.best_coef = self.problem.gene_model(forest[best:best + 1], dedup=False)[1][0].cpu()
            else:
                self.best_tree = forest[best]
        return host

    def run(self):
        start = time.time()
        generation = 0
        while True:
            tic = time.time()
            self.fitness = self.step()
            if self.is_show_details:
                self.show_details(tic, generation, self.fitness)
            if self.fitness_target is not None and self.best_fitness >= self.fitness_target:
                print(f"stopped: best fitness {float(self.best_fitness):.6g} reached the target {self.fitness_target}")
                break
            if self.time_limit is not None and time.time() - start > self.time_limit:
                print(f"stopped: {self.time_limit} s time limit")
                break
            if self.validation_patience is not None and self.validation_stale >= self.validation_patience:
                print(f"stopped: no better validation fitness than {float(self.best_validation_fitness):.6g} "
                      f"for {self.validation_patience} generations")
                break
            generation += 1
            if generation >= self.generation_limit:
                print(f"stopped: {self.generation_limit} generations")
                break
        return self.best_tree if self.validation_patience is None else self.best_validation_tree

    def show_details(self, tic, generation, fitness):
        b = self.valid_fitness_boundry
        valid = fitness[(fitness < b) & (fitness > -b)]
        ms = (time.time() - tic) * 1000
        line = f"gen {generation:4d}  {ms:8.2f} ms  {len(valid)} of {len(fitness)} finite"
        if len(valid):
            line += (f"  best {float(valid.max()):.4f}  mean {float(valid.mean()):.4f} +- {float(valid.std(unbiased=False)):.4f}"
                     f"  worst {float(valid.min()):.4f}")
        print(line)
