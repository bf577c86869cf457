"""Selection operators.  ``DefaultSelection`` follows src/evogp/algorithm/selection/default.py:8-71:
sort by fitness (descending), keep the top ``survival_rate`` fraction as parents and the top
``elite_cnt`` / ``elite_rate`` as elites that are copied unchanged.  Pure index arithmetic in torch."""
from __future__ import annotations

from typing import Optional

import torch

from ..tree import Forest


class BaseSelection:
    def __call__(self, forest: Forest, fitness: torch.Tensor):
        raise NotImplementedError


class DefaultSelection(BaseSelection):
    def __init__(self, survival_rate: float = 0.3, elite_cnt: Optional[int] = None,
                 elite_rate: Optional[float] = None):
        assert 0 <= survival_rate <= 1, "survival_rate should be in [0, 1]"
        assert elite_cnt is None or elite_rate is None, "elite_cnt and elite_rate should not be set at the same time"
        self.survival_rate = survival_rate
        self.elite_cnt = elite_cnt
        self.elite_rate = elite_rate

    def counts(self, pop_size: int):
        n_survive = int(pop_size * self.survival_rate)
        if self.elite_cnt is not None:
            n_elite = self.elite_cnt
        elif self.elite_rate is not None:
            n_elite = int(pop_size * self.elite_rate)
        else:
            n_elite = 0
        return n_elite, n_survive

    def __call__(self, forest: Forest, fitness: torch.Tensor):
        """-> (elite_indices int32, survivor_indices int32), both prefixes of the descending order.
        A stable sort is used so that replicated ranks of a sharded run agree on ties.  NaN ranks worst, behind -inf, and -0 ties
        with +0 -- the ranking of csrc/select.hip and parallel.select_order, so the fused step and this one choose the same two
        sets.  (The reference's plain torch.sort(descending=True) puts NaN FIRST, selection/default.py:65: a tree without a
        fitness would be its first elite.)"""
        n_elite, n_survive = self.counts(forest.pop_size)
        nan = fitness != fitness
        by_value = torch.sort(torch.where(nan, float("-inf"), fitness), descending=True, stable=True).indices
        order = by_value[torch.sort(nan[by_value].to(torch.int8), stable=True).indices]   # NaN behind -inf, both groups in order
        return order[:n_elite].to(torch.int32), order[:n_survive].to(torch.int32)


# ---- selectors and the non-default selections ---------------------------------------------------------------------
# Reference: selection/selection_utils.py:6-130, rank.py, roulette.py, tournament.py:59-133, truncation.py.  All of them
# are index programs over the fitness vector; they are written here for the documented behaviour (the reference's
# Rank/Truncation code indexes its probability vectors with tree indices where ranks are meant) and run without host
# syncs.  ``fitness`` is "higher is better"; -inf / NaN entries are never preferred.

def _clean(fitness: torch.Tensor) -> torch.Tensor:
    return torch.nan_to_num(fitness.to(torch.float32), nan=float("-inf"))


class BaseSelector:
    """fitness, n -> int32[n] indices of chosen individuals (with replacement)"""

    def __call__(self, fitness: torch.Tensor, choosed_num: int) -> torch.Tensor:
        raise NotImplementedError


class RankSelector(BaseSelector):
    """Linear ranking: P(rank r) = (1/n) (1 + sp (1 - 2 r / (n - 1))), r = 0 for the best."""

    def __init__(self, selection_pressure: float = 0.5):
        assert 0 <= selection_pressure <= 1, "selection_pressure should be in [0, 1]"
        self.sp = selection_pressure

    def __call__(self, fitness, choosed_num):
        n = fitness.shape[0]
        order = torch.sort(_clean(fitness), descending=True, stable=True).indices
        r = torch.arange(n, dtype=torch.float32, device=fitness.device)
        prob = (1.0 / n) * (1.0 + self.sp * (1.0 - 2.0 * r / max(n - 1, 1)))
        return order[torch.multinomial(prob, choosed_num, replacement=True)].to(torch.int32)


class RouletteSelector(BaseSelector):
    """P(i) proportional to fitness_i (negative / non-finite fitness counts as 0; all-zero falls back to uniform)."""

    def __call__(self, fitness, choosed_num):
        w = _clean(fitness).clamp(min=0.0)
        w = torch.where(torch.isfinite(w), w, torch.zeros_like(w))
        w = w + (w.sum() <= 0).to(w.dtype)  # uniform when nothing is positive
        return torch.multinomial(w, choosed_num, replacement=True).to(torch.int32)


class TruncationSelector(BaseSelector):
    """Uniform among the best ``survivor_rate`` fraction."""

    def __init__(self, survivor_rate: float = 0.5):
        assert 0 <= survivor_rate <= 1, "survivor_rate should be in [0, 1]"
        self.survivor_rate = survivor_rate

    def __call__(self, fitness, choosed_num):
        n = fitness.shape[0]
        top = max(1, int(n * self.survivor_rate))
        order = torch.sort(_clean(fitness), descending=True, stable=True).indices
        return order[torch.randint(0, top, (choosed_num,), device=fitness.device)].to(torch.int32)


class TournamentSelector(BaseSelector):
    """``choosed_num`` tournaments of ``tournament_size`` contenders (selection/tournament.py:59-133): the k-th best contender
    wins with probability p (1 - p)^k, ranks past the tournament fall back to the best (:98-104).  The contenders come in
    PASSES of ``n // tournament_size`` tournaments, as in the reference (:117-121: one ``torch.multinomial`` row of
    ``n_tournament * t_size`` uniform draws per pass): with ``replace=False`` nobody enters twice in a pass.

    Split into ``draw`` (the random numbers) and ``apply`` (deterministic), like the mutation operators:
    tests/golden/make_tournament_golden.py records the reference's own draws, ``apply`` must return its survivors."""

    def __init__(self, tournament_size: int, best_probability: float = 1, replace: bool = True):
        assert tournament_size >= 1
        self.t_size = tournament_size
        self.best_p = best_probability
        self.replace = replace

    def passes(self, n: int, count: int):
        """-> (tournaments per pass, number of passes) -- tournament.py:117-119"""
        per_pass = max(n // self.t_size, 1)
        return per_pass, (count - 1) // per_pass + 1

    def contenders(self, n: int, count: int, device) -> torch.Tensor:
        """int64[count][t_size]: the tournaments' members"""
        t = self.t_size
        per_pass, passes = self.passes(n, count)
        if self.replace:
            return torch.randint(0, n, (passes * per_pass, t), device=device)[:count]
        perm = torch.rand((passes, n), device=device).argsort(dim=1)[:, : per_pass * t]
        if perm.shape[1] < per_pass * t:  # population smaller than one tournament
            perm = perm.repeat(1, (per_pass * t) // perm.shape[1] + 1)[:, : per_pass * t]
        return perm.reshape(-1, t)[:count]

    def draw(self, n: int, count: int, device):
        """-> (contenders int64[count][t], u float32[count] or None when the best always wins)"""
        c = self.contenders(n, count, device)
        u = None if (self.best_p >= 1 and self.t_size > 1000) else torch.rand(count, device=device)
        return c, u

    def apply(self, fitness: torch.Tensor, contenders: torch.Tensor, u: Optional[torch.Tensor]) -> torch.Tensor:
        f = _clean(fitness)
        c = contenders.to(torch.int64)
        cf = f[c]
        if u is None or self.best_p >= 1:
            # p = 1: log(u) / log(0) = -0 -> rank 0, the best (tournament.py:98-104); :123-124 takes the arg-max directly
            # for tournaments above 1000 contenders
            pick = cf.argmax(dim=1, keepdim=True)
        else:
            rank = cf.argsort(dim=1, descending=True, stable=True)
            one_minus_p = 1 - torch.tensor(self.best_p, dtype=torch.float32, device=f.device)   # in float32, as :100-101
            nth = (torch.log(u.to(torch.float32)) / torch.log(one_minus_p)).to(torch.int64)
            nth = torch.where((nth >= self.t_size) | (nth < 0), torch.zeros_like(nth), nth)
            pick = rank.gather(1, nth[:, None])
        return c.gather(1, pick).squeeze(1).to(torch.int32)

    def __call__(self, fitness, choosed_num):
        c, u = self.draw(fitness.shape[0], choosed_num, fitness.device)
        return self.apply(fitness, c, u)


class _SelectorSelection(BaseSelection):
    """survivors = selector(fitness, survivor count), elites = the best elite count (rank.py, roulette.py, ...)"""

    def __init__(self, selector: BaseSelector, survivor_rate: float = 0.5, elite_rate: float = 0,
                 survivor_cnt: Optional[int] = None, elite_cnt: Optional[int] = None):
        assert 0 <= survivor_rate <= 1, "survivor_rate should be in [0, 1]"
        assert 0 <= elite_rate <= 1, "elite_rate should be in [0, 1]"
        self.selector = selector
        self.survivor_rate = survivor_rate
        self.survivor_cnt = survivor_cnt
        self.elite_rate = elite_rate
        self.elite_cnt = elite_cnt

    def counts(self, pop_size: int):
        n_surv = self.survivor_cnt if self.survivor_cnt is not None else int(pop_size * self.survivor_rate)
        n_elite = self.elite_cnt if self.elite_cnt is not None else int(pop_size * self.elite_rate)
        return n_elite, n_surv

    def __call__(self, forest: Forest, fitness: torch.Tensor):
        n_elite, n_surv = self.counts(forest.pop_size)
        survivors = self.selector(fitness, n_surv)
        if n_elite > 0:
            elites = torch.topk(_clean(fitness), n_elite, sorted=True).indices.to(torch.int32)
        else:
            elites = torch.empty(0, dtype=torch.int32, device=fitness.device)
        return elites, survivors


class RankSelection(_SelectorSelection):
    def __init__(self, selection_pressure: float = 0.5, survivor_rate: float = 0.5, elite_rate: float = 0,
                 survivor_cnt: Optional[int] = None, elite_cnt: Optional[int] = None):
        super().__init__(RankSelector(selection_pressure), survivor_rate, elite_rate, survivor_cnt, elite_cnt)


class RouletteSelection(_SelectorSelection):
    def __init__(self, survivor_rate: float = 0.5, elite_rate: float = 0, survivor_cnt: Optional[int] = None,
                 elite_cnt: Optional[int] = None):
        super().__init__(RouletteSelector(), survivor_rate, elite_rate, survivor_cnt, elite_cnt)


class TruncationSelection(_SelectorSelection):
    def __init__(self, survivor_rate: float = 0.5, elite_rate: float = 0, survivor_cnt: Optional[int] = None,
                 elite_cnt: Optional[int] = None):
        super().__init__(TruncationSelector(survivor_rate), survivor_rate, elite_rate, survivor_cnt, elite_cnt)


class TournamentSelection(_SelectorSelection):
    def __init__(self, tournament_size: int, best_probability: float = 1, replace: bool = True,
                 survivor_rate: float = 0.5, elite_rate: float = 0, survivor_cnt: Optional[int] = None,
                 elite_cnt: Optional[int] = None):
        super().__init__(TournamentSelector(tournament_size, best_probability, replace), survivor_rate, elite_rate,
                         survivor_cnt, elite_cnt)

    def counter_based(self, fitness: torch.Tensor, seed: int, generation: int):
        """The operator with its contenders taken from the counter-based words of evogp_amd/parallel.py (contender k of tournament
        i = word(seed, generation, 16 + k, i) % n) instead of torch's generator: every rank of a sharded run names the same
        contenders without sharing generator state, and on a GPU the whole selection is two launches (csrc/select.hip
        tournament_kernel + the radix select for the elites).  Same distribution as ``__call__`` (tournament.py:59-133).  Only for
        the reference's default arguments — contenders with replacement, the best one wins; None otherwise (the caller then runs
        ``__call__`` under a seeded generator)."""
        sel = self.selector
        if not sel.replace or sel.best_p < 1:
            return None
        from ..parallel import _select_key, default_lists, random_words

        n = fitness.shape[0]
        n_elite, n_surv = self.counts(n)
        if n_surv < 1:
            return None
        fit = fitness.to(torch.float32).contiguous()
        if fit.is_cuda:
            parents = torch.ops.evogp_hip.tournament_select(fit, n_surv, sel.t_size, seed, generation)
        else:
            c = random_words(seed, generation, sel.t_size, 0, n_surv, fit.device, first_row=16).to(torch.int64) % n     # (t, n_surv)
            best = _select_key(fit)[c].argmax(dim=0, keepdim=True)                                                        # first of equal keys
            parents = c.gather(0, best).squeeze(0).to(torch.int32)
        elites = default_lists(fit, n_elite, max(n_elite, 1))[0] if n_elite > 0 else torch.empty(0, dtype=torch.int32, device=fit.device)
        return elites.contiguous(), parents.contiguous()


# ---- epsilon-lexicase (La Cava, Spector & Danai 2016; La Cava, Helmuth, Spector & Moore 2019) ------------------------------------
# Counter-word rows (csrc/evogp_defs.hpp counter_word, parallel.random_words) of a LexicaseSelection's own seed: 2^21 + 0..3 the
# round keys of event k's case permutation, 2^21 + 4 the pick of event k (csrc/lexicase.hip), 2^21 + 5 the down-sampled rows.
LEXICASE_ROW_SAMPLE = 2**21 + 5


def lexicase_epsilon(errors: torch.Tensor) -> torch.Tensor:
    """``(pop, n)`` errors of any strides -> ``(n,)`` float32: eps_c = lowmed(|e - lowmed(e)|) over the finite errors e of case c, the
    median absolute deviation; 0 for a case without a finite error.  lowmed is the lower median, torch.nanmedian's convention once the
    non-finite entries are NaN.  Runs on the errors' device with no host sync."""
    x = errors.to(torch.float32)
    x = torch.where(torch.isfinite(x), x, torch.full_like(x, float("nan")))
    med = torch.nanmedian(x, dim=0).values
    mad = torch.nanmedian((x - med[None, :]).abs(), dim=0).values
    return torch.where(mad == mad, mad, torch.zeros_like(mad))


def _counter_row(seed: int, generation: int, row: int, n: int, device) -> torch.Tensor:
    """int64[n]: counter word ``row`` of items 0 .. n-1 under (seed, generation) -- ``parallel.random_words(seed, generation, 1, 0, n,
    device, first_row=row)[0]`` computed without a host-to-device copy (the base is folded on the host), so nothing synchronises"""
    from ..parallel import _mix64

    m = (1 << 64) - 1

    def mix(x):
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m
        return x ^ (x >> 31)

    start = (mix((seed * 1000003 + generation) & m) + (row << 40)) & m
    start = start - (1 << 64) if start >= 1 << 63 else start          # the same 64 bits as a signed torch scalar
    x = _mix64(torch.arange(n, dtype=torch.int64, device=device) + start)
    return ((x >> 33) & 0x7FFFFFFF) % (2**31 - 1)


class LexicaseSelection(BaseSelection):
    """Semi-dynamic epsilon-lexicase selection over per-case errors (La Cava et al. 2016, 2019): every survivor slot is one event that
    filters the population case by case, in an order of its own, keeping the trees within eps_c of the best error left on case c, and
    draws the survivor from what is left (include/evogp_hip.h evogp_hip_lexicase_select has the exact contract; tests/lexicase_ref.py
    restates it).  Elites are the best elite count by ``fitness``, as in the other selections.

    ``case_errors``: by default ``forest.SR_case_errors(datapoints[rows], labels[rows], use_MSE)`` (absolute errors by default, as in
    La Cava et al.); a callable ``case_errors(forest) -> (pop, n)`` tensor replaces it (e.g. 0/1 misclassification, with epsilon 0:
    plain lexicase).  ``epsilon``: "auto" (``lexicase_epsilon``, the median absolute deviation per case), a float, or an ``(n,)``
    tensor.  ``downsample_rate < 1``: down-sampled lexicase (Hernandez et al. 2019), every call uses max(1, round(rate * D)) rows, the
    rows with the smallest counter words of this call (ties: lower row first).  The random numbers are counter words of a seed the
    object draws once from torch's CPU generator (reproducible under torch.manual_seed) and of its own call counter.  Nothing in
    ``__call__`` synchronises with the host.  GPU forests only (the ops have no CPU kernel); not for a sharded run, whose selection
    sees no trees."""

    def __init__(self, datapoints: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None, epsilon="auto", use_MSE: bool = False,
                 downsample_rate: float = 1.0, survivor_rate: float = 1.0, elite_rate: float = 0.0, survivor_cnt: Optional[int] = None,
                 elite_cnt: Optional[int] = None, case_errors=None):
        assert (datapoints is None) == (labels is None), "datapoints and labels should be given together"
        assert case_errors is not None or datapoints is not None, "LexicaseSelection needs (datapoints, labels) or case_errors"
        assert case_errors is None or callable(case_errors), "case_errors should be a callable forest -> (pop, n) tensor"
        assert 0 < downsample_rate <= 1, "downsample_rate should be in (0, 1]"
        assert 0 <= survivor_rate <= 1, "survivor_rate should be in [0, 1]"
        assert 0 <= elite_rate <= 1, "elite_rate should be in [0, 1]"
        if isinstance(epsilon, str):
            assert epsilon == "auto", f"epsilon should be 'auto', a float or a tensor, but got {epsilon!r}"
        elif not isinstance(epsilon, torch.Tensor):
            epsilon = float(epsilon)
            assert epsilon >= 0, f"epsilon should be >= 0, but got {epsilon}"
        self.datapoints, self.labels = datapoints, labels
        self.epsilon = epsilon
        self.use_MSE = use_MSE
        self.downsample_rate = downsample_rate
        self.survivor_rate, self.survivor_cnt = survivor_rate, survivor_cnt
        self.elite_rate, self.elite_cnt = elite_rate, elite_cnt
        self.case_errors = case_errors
        self.seed = int(torch.randint(0, 2**40, (1,)).item())
        self.generation = 0
        self._data = None

    def counts(self, pop_size: int):
        n_surv = self.survivor_cnt if self.survivor_cnt is not None else int(pop_size * self.survivor_rate)
        n_elite = self.elite_cnt if self.elite_cnt is not None else int(pop_size * self.elite_rate)
        return n_elite, n_surv

    def rows(self, n_rows: int, device) -> Optional[torch.Tensor]:
        """int64 row indices (ascending) of this call's down-sample, None for all rows"""
        m = max(1, round(self.downsample_rate * n_rows))
        if m >= n_rows:
            return None
        w = _counter_row(self.seed, self.generation, LEXICASE_ROW_SAMPLE, n_rows, device)
        return torch.sort(torch.sort(w, stable=True).indices[:m]).values

    def errors(self, forest: Forest) -> torch.Tensor:
        """the ``(pop, n)`` errors this call selects on"""
        dev = forest.batch_node_value.device
        if self.case_errors is not None:
            e = self.case_errors(forest)
            assert e.dim() == 2 and e.shape[0] == forest.pop_size, (
                f"case_errors should return a ({forest.pop_size}, n) tensor, but got {tuple(e.shape)}")
            rows = self.rows(e.shape[1], e.device)
            return e if rows is None else e[:, rows]
        if self._data is None or self._data[0].device != dev:
            self._data = (self.datapoints.to(dev), self.labels.to(dev))   # (once per device)
        X, y = self._data
        rows = self.rows(X.shape[0], dev)
        if rows is not None:
            X, y = X[rows], y[rows]
        return forest.SR_case_errors(X, y, self.use_MSE)

    def __call__(self, forest: Forest, fitness: torch.Tensor):
        if not isinstance(forest, Forest):
            raise TypeError("LexicaseSelection reads every tree's per-case errors: it cannot run in a sharded step, whose selection "
                            "sees only the gathered fitness vector")
        n_elite, n_surv = self.counts(forest.pop_size)
        errors = self.errors(forest)
        n = errors.shape[1]
        if isinstance(self.epsilon, str):
            eps = lexicase_epsilon(errors)
        elif isinstance(self.epsilon, torch.Tensor):
            eps = self.epsilon.to(device=errors.device, dtype=torch.float32).reshape(-1)
            assert eps.shape == (n,), f"epsilon should have shape ({n},), but got {tuple(self.epsilon.shape)}"
        else:
            eps = torch.full((n,), self.epsilon, dtype=torch.float32, device=errors.device)
        E = errors.t().to(torch.float32).contiguous()
        survivors = torch.ops.evogp_hip.lexicase_select(E, eps.contiguous(), n_surv, self.seed, self.generation)
        self.generation += 1
        if n_elite > 0:
            elites = torch.topk(_clean(fitness), n_elite, sorted=True).indices.to(torch.int32)
        else:
            elites = torch.empty(0, dtype=torch.int32, device=fitness.device)
        return elites, survivors


# ---- NSGA-II on (error, complexity) (Deb, Pratap, Agarwal & Meyarivan 2002) -------------------------------------------------------
# Counter-word rows of an NSGA2Selection's own seed: 2^22 + k contender k of tournament i (csrc/nsga2.hip).
class NSGA2Selection(BaseSelection):
    """Two-objective selection: error (``-fitness``) against an integer complexity, tree size by default.  Every call ranks the whole
    population on the device -- non-dominated fronts, crowding distance over the distinct points of a front, and the crowded-comparison
    order (front ascending, distance descending, tree index ascending) -- and holds ``tournament_size``-ary tournaments on that order
    (include/evogp_hip.h evogp_hip_pareto_rank / evogp_hip_nsga2_select have the exact contract; tests/nsga2_ref.py restates it).
    Trees of NaN or infinite fitness are unranked: they come last and are never preferred.  Clones of a point carry distance 0, so a
    collapsed population does not fill the mating pool with copies.

    ``elites = order[:n_elite]``.  ``mating_pool="all"``: the contenders are drawn from the whole population.  ``"elites"``: from the
    elites only, which is NSGA-II proper -- with ``elite_rate=0.5`` the elites are the environmental selection of P and Q (last
    generation's survivors and their offspring) and the parents are drawn among them.  ``complexity``: None for the tree size
    (``batch_subtree_size[:, 0]``, bounded by ``max_tree_len``), or a callable ``complexity(forest) -> integer tensor`` together with
    ``max_complexity`` (<= 65535), the bound the kernels size their tables by: it is never read back from the device, and a tree whose
    complexity lies outside ``[0, max_complexity]`` is unranked.  The random numbers are counter words of a seed the object draws once
    from torch's CPU generator (reproducible under torch.manual_seed) and of its own call counter.  Nothing in ``__call__``
    synchronises with the host.  GPU forests only (the ops have no CPU kernel); not for a sharded run, whose selection sees no trees."""

    def __init__(self, tournament_size: int = 2, survivor_rate: float = 1.0, elite_rate: float = 0.0, survivor_cnt: Optional[int] = None,
                 elite_cnt: Optional[int] = None, complexity=None, mating_pool: str = "all", max_complexity: Optional[int] = None):
        assert 1 <= tournament_size <= 2**20, f"tournament_size should be in [1, 2^20], but got {tournament_size}"
        assert 0 <= survivor_rate <= 1, "survivor_rate should be in [0, 1]"
        assert 0 <= elite_rate <= 1, "elite_rate should be in [0, 1]"
        assert mating_pool in ("all", "elites"), f"mating_pool should be 'all' or 'elites', but got {mating_pool!r}"
        assert complexity is None or callable(complexity), "complexity should be a callable forest -> integer tensor"
        assert (complexity is None) == (max_complexity is None), "complexity and max_complexity should be given together"
        assert max_complexity is None or 0 <= max_complexity <= 65535, f"max_complexity should be in [0, 65535], but got {max_complexity}"
        self.t_size = tournament_size
        self.survivor_rate, self.survivor_cnt = survivor_rate, survivor_cnt
        self.elite_rate, self.elite_cnt = elite_rate, elite_cnt
        self.complexity, self.max_complexity = complexity, max_complexity
        self.mating_pool = mating_pool
        self.seed = int(torch.randint(0, 2**40, (1,)).item())
        self.generation = 0

    def counts(self, pop_size: int):
        n_surv = self.survivor_cnt if self.survivor_cnt is not None else int(pop_size * self.survivor_rate)
        n_elite = self.elite_cnt if self.elite_cnt is not None else int(pop_size * self.elite_rate)
        return n_elite, n_surv

    def objectives(self, forest: Forest, fitness: torch.Tensor):
        """-> (err float32[pop], cx int32[pop], cx_bound): what the ranking sees"""
        if not isinstance(forest, Forest):
            raise TypeError("NSGA2Selection reads every tree's complexity: it cannot run in a sharded step, whose selection sees only "
                            "the gathered fitness vector")
        err = (-fitness.to(torch.float32)).contiguous()
        if self.complexity is None:
            cx, bound = forest.batch_subtree_size[:, 0], forest.max_tree_len
        else:
            cx, bound = self.complexity(forest), self.max_complexity
            assert isinstance(cx, torch.Tensor) and cx.shape == (forest.pop_size,) and not cx.dtype.is_floating_point and \
                cx.dtype != torch.bool, f"complexity should return an integer tensor of shape ({forest.pop_size},)"
        assert err.shape == (forest.pop_size,), f"fitness shape should be ({forest.pop_size}, ), but got {tuple(fitness.shape)}"
        return err, cx.to(device=err.device, dtype=torch.int32).contiguous(), bound

    def rank(self, forest: Forest, fitness: torch.Tensor):
        """-> (front int32, crowding float32, order int32); an unranked tree has front 0x7FFFFFFF and crowding 0"""
        return torch.ops.evogp_hip.pareto_rank(*self.objectives(forest, fitness))

    def pareto_set(self, forest: Forest, fitness: torch.Tensor) -> torch.Tensor:
        """bool[pop] on the device (no host sync): one tree per distinct (error, complexity) point of the first front -- the
        accuracy / complexity trade-off curve of the population"""
        front, crowding, _ = self.rank(forest, fitness)
        return (front == 0) & (crowding > 0)

    def __call__(self, forest: Forest, fitness: torch.Tensor):
        err, cx, bound = self.objectives(forest, fitness)
        pop = forest.pop_size
        n_elite, n_surv = self.counts(pop)
        pool = pop if self.mating_pool == "all" else n_elite
        assert 1 <= pool <= pop, f"mating_pool='elites' needs between 1 and {pop} elites, but got {n_elite}"
        _, _, order = torch.ops.evogp_hip.pareto_rank(err, cx, bound)
        survivors = torch.ops.evogp_hip.nsga2_select(order, pool, n_surv, self.t_size, self.seed, self.generation)
        self.generation += 1
        return order[:n_elite], survivors
