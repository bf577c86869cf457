"""Crossover operators.  ``DefaultCrossover`` follows src/evogp/algorithm/crossover/default.py:8-66:
both parents and both subtree positions are drawn uniformly; the draws only build int32 index
tensors, the tree surgery is one ``tree_crossover`` kernel."""
from __future__ import annotations

import torch

from ..tree import Forest
from .semantic_library import LibraryRefresh, SemanticLibrary


class BaseCrossover:
    def __call__(self, forest: Forest, survivor_indices: torch.Tensor, target_cnt: int, fitness: torch.Tensor):
        raise NotImplementedError


class DefaultCrossover(BaseCrossover):
    def draw(self, tree_sizes: torch.Tensor, n_parents: int, target_cnt: int, device):
        """Index tensors of one crossover round (parents in [0, n_parents), positions = u % size)."""
        parents = torch.randint(0, n_parents, (2, target_cnt), dtype=torch.int32, device=device)
        raw = torch.randint(0, torch.iinfo(torch.int32).max, (2, target_cnt), dtype=torch.int32, device=device)
        left, right = parents[0], parents[1]
        left_pos = raw[0] % tree_sizes[left]
        right_pos = raw[1] % tree_sizes[right]
        return left, right, left_pos.to(torch.int32), right_pos.to(torch.int32)

    def __call__(self, forest: Forest, survivor_indices: torch.Tensor, target_cnt: int, fitness: torch.Tensor):
        parents = forest[survivor_indices]
        sizes = parents.batch_subtree_size[:, 0]
        left, right, left_pos, right_pos = self.draw(sizes, len(parents), target_cnt, sizes.device)
        return parents.crossover(left, right, left_pos, right_pos)


class SemanticMateCrossover(DefaultCrossover):
    """DefaultCrossover with a geometric choice of the second parent (``SemanticMate``): the first parents and their
    positions are drawn as ``DefaultCrossover.draw`` draws them, ``right`` is what ``mate(parents, left)`` chooses for them, and the
    donor position is drawn after that, as ``word % size[right]``.  A subclass, so ``GeneticProgramming`` composes its step from the
    operators instead of taking the fused one.  No host synchronisation."""

    def __init__(self, mate):
        if not callable(mate):
            raise ValueError(f"mate should be a SemanticMate or a callable (parents, left) -> (right, score), but got {type(mate).__name__}")
        self.mate = mate

    def pairs(self, parents: Forest, target_cnt: int):
        """the index tensors of one round: ``(left, right, left_pos, right_pos)``, int32"""
        sizes = parents.batch_subtree_size[:, 0]
        left, _, left_pos, _ = self.draw(sizes, len(parents), target_cnt, sizes.device)
        right = self.mate(parents, left)[0].to(torch.int32)
        word = torch.randint(0, torch.iinfo(torch.int32).max, (target_cnt,), dtype=torch.int32, device=sizes.device)
        return left, right, left_pos, (word % sizes[right]).to(torch.int32)

    def __call__(self, forest: Forest, survivor_indices: torch.Tensor, target_cnt: int, fitness: torch.Tensor):
        parents = forest[survivor_indices]
        return parents.crossover(*self.pairs(parents, target_cnt))


# ---- the non-default crossovers ---------------------------------------------------------------------------------------
# Reference: crossover/diversity.py, crossover/leaf_biased.py.  ``crossover_rate`` of the offspring are recombined, the
# rest are verbatim copies of random survivors.  Here both kinds come out of ONE tree_crossover launch over the whole
# target count: a copy is a crossover whose left position is -1 (the kernel's copy-left rule, mutation.cu:256-266), so
# there is no second gather and no concatenation.

class DiversityCrossover(BaseCrossover):
    """Recipient and donor are drawn independently (uniformly from the survivors, or by ``recipient_selector`` /
    ``donor_selector`` from the whole population), positions uniformly (diversity.py)."""

    def __init__(self, crossover_rate: float = 0.9, recipient_selector=None, donor_selector=None):
        self.crossover_rate = crossover_rate
        self.recipient_selector = recipient_selector
        self.donor_selector = donor_selector

    def _parents(self, selector, fitness, survivor_indices, n):
        if selector is not None:
            return selector(fitness, n).to(torch.int64)
        pick = torch.randint(0, survivor_indices.shape[0], (n,), device=survivor_indices.device)
        return survivor_indices.to(torch.int64)[pick]

    def _positions(self, forest: Forest, recipients, donors):
        sizes = forest.batch_subtree_size[:, 0].to(torch.int64)
        raw = torch.randint(0, torch.iinfo(torch.int32).max, (2, recipients.shape[0]), device=recipients.device)
        return raw[0] % sizes[recipients], raw[1] % sizes[donors]

    def __call__(self, forest: Forest, survivor_indices: torch.Tensor, target_cnt: int, fitness: torch.Tensor):
        target_cnt = int(target_cnt)
        n_cross = int(target_cnt * self.crossover_rate)
        recipients = self._parents(self.recipient_selector, fitness, survivor_indices, target_cnt)
        donors = self._parents(self.donor_selector, fitness, survivor_indices, target_cnt)
        rpos, dpos = self._positions(forest, recipients, donors)
        copy = torch.arange(target_cnt, device=rpos.device) >= n_cross      # the tail of the offspring are plain copies
        rpos = torch.where(copy, torch.full_like(rpos, -1), rpos)
        i32 = lambda t: t.to(torch.int32).contiguous()  # noqa: E731
        return forest.crossover(i32(recipients), i32(donors), i32(rpos), i32(dpos))


class LeafBiasedCrossover(DiversityCrossover):
    """As DiversityCrossover, but with probability ``leaf_bias`` both positions are leaves (leaf_biased.py): swaps of
    single terminals instead of whole subtrees."""

    def __init__(self, crossover_rate: float = 0.9, leaf_bias: float = 0.3, recipient_selector=None, donor_selector=None):
        super().__init__(crossover_rate, recipient_selector, donor_selector)
        self.leaf_bias = leaf_bias

    @staticmethod
    def _leaf_pos(sizes_rows: torch.Tensor) -> torch.Tensor:
        n, L = sizes_rows.shape
        live = torch.arange(L, device=sizes_rows.device)[None, :] < sizes_rows[:, :1]
        return torch.argmax(torch.rand((n, L), device=sizes_rows.device) * (live & (sizes_rows == 1)), dim=1)

    def _positions(self, forest: Forest, recipients, donors):
        rpos, dpos = super()._positions(forest, recipients, donors)
        sizes = forest.batch_subtree_size
        leaf = torch.rand(recipients.shape[0], device=recipients.device) < self.leaf_bias
        return (torch.where(leaf, self._leaf_pos(sizes[recipients]), rpos),
                torch.where(leaf, self._leaf_pos(sizes[donors]), dpos))


class CombinedDefaultCrossover(BaseCrossover):
    """DefaultCrossover on every sub-forest of a CombinedForest: ONE draw of parent pairs shared by all sub-forests (an
    offspring takes all of its expressions from the same two parents), independent cut points per sub-forest
    (crossover/combined_dafault.py:8-54)."""

    def __call__(self, forest, survivor_indices: torch.Tensor, target_cnt: int, fitness: torch.Tensor):
        from ..tree import CombinedForest

        survivors = forest[survivor_indices]
        dev = survivors.forests[0].batch_node_value.device
        left, right = torch.randint(0, len(survivors), (2, target_cnt), dtype=torch.int32, device=dev)
        children = []
        for sub in survivors.forests:
            sizes = sub.batch_subtree_size[:, 0].to(torch.int64)
            raw = torch.randint(0, 2**31 - 1, (2, target_cnt), device=dev)
            lpos = (raw[0] % sizes[left.long()]).to(torch.int32)
            rpos = (raw[1] % sizes[right.long()]).to(torch.int32)
            children.append(sub.crossover(left, right, lpos, rpos))
        return CombinedForest(children, forest.data_info)


# ---- approximately geometric semantic crossover (no counterpart in the reference) ------------------------------------------------------
class ApproxGeometricCrossover(LibraryRefresh, BaseCrossover):
    """The approximately geometric semantic crossover (AGX) of Pawlak, Wieloch & Krawiec (IEEE TEVC 2015), next to their Random Desired
    Operator (``SemanticBackpropMutation``): the recipient is inverted from its root down to a random node towards the MIDPOINT of its
    own and its mate's predictions on ``datapoints`` (``Forest.SR_midpoint_match``, csrc/sr_backprop.hip), and the
    subtree at that node is replaced by the member of a LIBRARY of small trees nearest to what the node would have to return -- or,
    with ``allow_constant``, by the constant that is nearer still.  The offspring lies, approximately, on the segment between its
    parents in semantic space.  It needs no labels.

    ``library``, ``descriptor``, ``library_size``: as for ``SemanticBackpropMutation``; a ``SemanticLibrary`` may be shared with it,
    and ``update_library`` on either then reaches both; ``refresh_every``, ``refresh_max_size``: the periodic rebuild from the subtrees of
    the forest handed to the call (``LibraryRefresh``; with a shared library set it on one operator only).  Pairs and the recipient's position are drawn as ``DefaultCrossover.draw`` draws
    them (the donor position is unused); a pair of one tree with itself is not excluded: its midpoint is the tree's own predictions, so
    the subtree is replaced by the library member nearest to what it already computes.  An offspring without a match (``best == -1``:
    a function on the path has no inverse, no row is REQUIRED, or no library member is finite there) takes the offspring of the same
    index from ``fallback`` -- any ``BaseCrossover``, called once with the same arguments -- or is a copy of its recipient.  ``mate``: a
    ``SemanticMate`` (or any callable ``(parents, left) -> (right, score)``) that replaces the uniformly drawn mates -- ``right`` only;
    None leaves every draw and every result as it is.  No host synchronisation of its own (a rebuild of the library has two)."""

    def __init__(self, datapoints: torch.Tensor, library=None, descriptor=None, library_size: int = 256, allow_constant: bool = True,
                 fallback: BaseCrossover = None, refresh_every: int = 0, refresh_max_size=None, mate=None):
        self._init_refresh(refresh_every, refresh_max_size)
        if mate is not None and not callable(mate):
            raise ValueError(f"mate should be None, a SemanticMate or a callable (parents, left) -> (right, score), but got {type(mate).__name__}")
        self.mate = mate
        if not isinstance(datapoints, torch.Tensor) or datapoints.dim() != 2 or datapoints.shape[0] == 0:
            raise ValueError(f"datapoints should be a (D, input_len) tensor, but got {tuple(getattr(datapoints, 'shape', ()))}")
        if fallback is not None and not isinstance(fallback, BaseCrossover):
            raise ValueError(f"fallback should be a BaseCrossover, but got {type(fallback).__name__}")
        self.datapoints = datapoints.contiguous().to(torch.float32)
        self.allow_constant = bool(allow_constant)
        self.fallback = fallback
        self.semantic_library = SemanticLibrary.of(self.datapoints, library, descriptor, library_size, "ApproxGeometricCrossover")

    @property
    def library(self) -> Forest:
        return self.semantic_library.library

    @property
    def semantics(self) -> torch.Tensor:
        return self.semantic_library.semantics

    def draw(self, tree_sizes: torch.Tensor, n_parents: int, target_cnt: int, device):
        """the draws of ``DefaultCrossover``: pairs and positions; the donor position is drawn and not used"""
        return DefaultCrossover().draw(tree_sizes, n_parents, target_cnt, device)

    def __call__(self, forest: Forest, survivor_indices: torch.Tensor, target_cnt: int, fitness: torch.Tensor):
        self._refresh(forest)
        parents = forest[survivor_indices]
        sizes = parents.batch_subtree_size[:, 0]
        left, right, left_pos, _ = self.draw(sizes, len(parents), target_cnt, sizes.device)
        if self.mate is not None:
            right = self.mate(parents, left)[0].to(torch.int32)
        new, found = self.apply(parents, left, right, left_pos)
        if self.fallback is not None:
            other = self.fallback(forest, survivor_indices, target_cnt, fitness)
            new = Forest(new.input_len, 1, *(torch.where(found[:, None], a, b) for a, b in zip(new._tensors(), other._tensors())),
                         func_mask=Forest.join_masks(new.func_mask, other.func_mask))
        return new

    def apply(self, parents: Forest, left: torch.Tensor, right: torch.Tensor, left_pos: torch.Tensor):
        """``(offspring, found)``: offspring n is ``parents[left[n]]`` with the subtree at ``left_pos[n]`` replaced by the donor that
        brings it nearest to the midpoint between itself and ``parents[right[n]]``; a verbatim copy where ``found[n]`` is False.  No
        host synchronisation."""
        if parents.output_len != 1 or parents.input_len != self.library.input_len:
            raise ValueError(f"ApproxGeometricCrossover: the forest should have {self.library.input_len} inputs and one output, but has "
                             f"{parents.input_len} and {parents.output_len}")
        self.semantic_library.rows(parents.max_tree_len)   # (a library wider than the forest: ValueError before anything runs)
        chosen = parents[left.to(torch.int64)]
        left_pos = left_pos.to(torch.int32)
        best, dist, const, const_dist, _, _ = chosen.SR_midpoint_match(self.datapoints, left_pos, parents, self.semantics, mate_index=right)
        found = best >= 0
        donors = self.semantic_library.donors(best, dist, const, const_dist, self.allow_constant, parents.input_len, parents.max_tree_len)
        return chosen.mutate(torch.where(found, left_pos, torch.full_like(left_pos, -1)), donors), found   # (position -1: a copy)
