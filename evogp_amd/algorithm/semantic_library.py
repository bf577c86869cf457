"""The library of small trees the semantic operators draw their donors from (``SemanticBackpropMutation``,
``ApproxGeometricCrossover``): its build from a descriptor, ``update_library``, its semantics on the datapoints
and its rows padded to a forest's width.  One object may serve several operators: an ``update_library`` call on it reaches them all."""
from __future__ import annotations

from typing import Optional

import torch

from ..tree import Forest, GenerateDescriptor, NType


def leaf_rows(values: torch.Tensor, ntype: int, max_tree_len: int):
    """one-node trees holding ``values`` (n,) as (value, type, size) rows of ``max_tree_len`` words"""
    n = values.shape[0]
    value = torch.zeros((n, max_tree_len), dtype=torch.float32, device=values.device)
    node_type = torch.zeros((n, max_tree_len), dtype=torch.int16, device=values.device)
    size = torch.zeros((n, max_tree_len), dtype=torch.int16, device=values.device)
    value[:, 0], node_type[:, 0], size[:, 0] = values.to(torch.float32), ntype, 1
    return value, node_type, size


class SemanticLibrary:
    """``library``: a single-output Forest (at most 1024 trees are kept).  Without one it is built from ``descriptor``: the one-node
    tree of every variable and ``library_size`` random trees.  Either way it is reduced to one member per semantics
    (``semantic_unique(datapoints, keep="smallest")``) and truncated to 1024; ``semantics`` (K, D) float32 is computed once.
    ``owner`` names the operator in the error texts."""

    def __init__(self, datapoints: torch.Tensor, library: Optional[Forest] = None, descriptor: Optional[GenerateDescriptor] = None,
                 library_size: int = 256, owner: str = "SemanticLibrary"):
        self.datapoints = datapoints
        if library is None:
            if descriptor is None:
                raise ValueError(f"{owner} needs a library or a descriptor to build one from")
            if descriptor.output_len != 1 or descriptor.input_len != datapoints.shape[1]:
                raise ValueError(f"the descriptor should generate single-output trees of {datapoints.shape[1]} inputs, but has "
                                 f"{descriptor.input_len} inputs and {descriptor.output_len} outputs")
            if not isinstance(library_size, int) or library_size < 0:
                raise ValueError(f"library_size should be a non-negative integer, but got {library_size!r}")
            dev = self.datapoints.device
            variables = Forest(descriptor.input_len, 1, *leaf_rows(torch.arange(descriptor.input_len, device=dev), NType.VAR, descriptor.max_tree_len),
                               func_mask=descriptor.func_mask)
            library = variables + Forest.random_generate(library_size, descriptor) if library_size else variables
        self.update_library(library)

    @classmethod
    def of(cls, datapoints: torch.Tensor, library, descriptor, library_size, owner: str) -> "SemanticLibrary":
        """what an operator's ``library=`` argument stands for: a shared SemanticLibrary as it is, or a new one"""
        if isinstance(library, SemanticLibrary):
            if tuple(library.datapoints.shape) != tuple(datapoints.shape):
                raise ValueError(f"the shared library was built on datapoints of shape {tuple(library.datapoints.shape)}, "
                                 f"but {owner} has {tuple(datapoints.shape)}")
            return library
        return cls(datapoints, library, descriptor, library_size, owner)

    def update_library(self, forest: Forest, source: str = "trees", min_size: int = 1, max_size: Optional[int] = None, *,
                       sig: Optional[torch.Tensor] = None) -> None:
        """the library becomes the semantically distinct members of ``forest`` on the datapoints (the smallest tree of every class, in
        index order, at most 1024): a population-derived library when ``forest`` is the population.  One host synchronisation.

        ``source="subtrees"``: the members are drawn from the SUBTREES of ``forest`` instead -- the population-based library of the
        paper.  ``forest.subtree_library(datapoints, 1024, min_size, max_size)`` names up to 1024 distinct subtrees of ``min_size`` to
        ``max_size`` nodes, the most frequent first (csrc/sr_subtree_sig.hip; 64-bit signatures decide, nothing verifies them), and
        these go through the reduction above, which computes the semantics from the extracted trees themselves.  A forest of trees
        that are all too large to be donors still yields a library of their parts.  Two host synchronisations; ``ValueError`` when
        no subtree is eligible.  ``min_size`` and ``max_size`` belong to ``source="subtrees"`` alone, and so does ``sig``:
        ``forest.SR_subtree_signatures(datapoints)`` from a caller that already has it (one signature pass per generation then serves
        this and ``forest.remove_introns(datapoints, sig=sig)``); None computes it."""
        from ..tree.forest import BACKPROP_MAX_LIBRARY

        if not isinstance(forest, Forest) or forest.output_len != 1 or forest.input_len != self.datapoints.shape[1]:
            raise ValueError(f"the library should be a single-output Forest of {self.datapoints.shape[1]} inputs")
        if source not in ("trees", "subtrees"):
            raise ValueError(f"source should be 'trees' or 'subtrees', but got {source!r}")
        if source == "subtrees":
            forest = forest.subtree_library(self.datapoints, BACKPROP_MAX_LIBRARY, min_size, max_size, sig=sig)[0]
            if forest.pop_size == 0:
                raise ValueError(f"the forest has no well-formed subtree of {min_size} to {max_size} nodes to build a library from")
        elif min_size != 1 or max_size is not None or sig is not None:
            raise ValueError("min_size, max_size and sig select subtrees: they need source='subtrees'")
        unique, _, _ = forest.semantic_unique(self.datapoints, keep="smallest")
        self.library = unique[:BACKPROP_MAX_LIBRARY] if unique.pop_size > BACKPROP_MAX_LIBRARY else unique
        self.semantics = self.library.batch_forward(self.datapoints)[:, :, 0].contiguous()
        self._padded = {}

    def rows(self, max_tree_len: int):
        """the library's three tensors at the forest's row width"""
        lib = self.library
        if lib.max_tree_len == max_tree_len:
            return lib.batch_node_value, lib.batch_node_type, lib.batch_subtree_size
        if lib.max_tree_len > max_tree_len:
            raise ValueError(f"the library's max_tree_len {lib.max_tree_len} exceeds the forest's {max_tree_len}")
        if max_tree_len not in self._padded:
            pad = (0, max_tree_len - lib.max_tree_len)
            self._padded[max_tree_len] = tuple(torch.nn.functional.pad(a, pad) for a in (lib.batch_node_value, lib.batch_node_type, lib.batch_subtree_size))
        return self._padded[max_tree_len]

    def donors(self, best: torch.Tensor, dist: torch.Tensor, const: torch.Tensor, const_dist: torch.Tensor, allow_constant: bool,
               input_len: int, max_tree_len: int) -> Forest:
        """the donor of every matched tree: the member ``best`` (member 0 where best is -1: such a row is not spliced), or with
        ``allow_constant`` the one-node CONST where it is nearer than that member"""
        lib_value, lib_type, lib_size = self.rows(max_tree_len)
        found = best >= 0
        member = best.clamp(min=0).to(torch.int64)
        value, node_type, size = lib_value[member], lib_type[member], lib_size[member]
        if allow_constant:
            nearer = found & (const_dist < dist.gather(1, member[:, None]).squeeze(1))
            cv, ct, cs = leaf_rows(const, NType.CONST, max_tree_len)
            value, node_type, size = (torch.where(nearer[:, None], c, a) for c, a in ((cv, value), (ct, node_type), (cs, size)))
        return Forest(input_len, 1, value, node_type, size, func_mask=self.library.func_mask)


class LibraryRefresh:
    """what ``SemanticBackpropMutation`` and ``ApproxGeometricCrossover`` share around their ``semantic_library``: ``update_library`` and
    the periodic rebuild from the population's subtrees.  ``refresh_every = n > 0``: every n-th call of the operator first rebuilds the
    library from the subtrees of at most ``refresh_max_size`` nodes (None: any size) of the forest the operator was handed
    (``update_library(forest, source="subtrees", max_size=refresh_max_size)``, which waits for the host twice); 0: never.  Operators that SHARE a ``SemanticLibrary``
    should set it on one of them only: a rebuild by either reaches both, and two would do the work twice per generation."""

    def _init_refresh(self, refresh_every, refresh_max_size) -> None:
        if isinstance(refresh_every, bool) or not isinstance(refresh_every, int) or refresh_every < 0:
            raise ValueError(f"refresh_every should be a non-negative integer, but got {refresh_every!r}")
        if refresh_max_size is not None and (isinstance(refresh_max_size, bool) or not isinstance(refresh_max_size, int) or refresh_max_size < 1):
            raise ValueError(f"refresh_max_size should be None or a positive integer, but got {refresh_max_size!r}")
        self.refresh_every, self.refresh_max_size, self._refresh_calls = refresh_every, refresh_max_size, 0

    def update_library(self, forest: Forest, source: str = "trees", min_size: int = 1, max_size: Optional[int] = None, *,
                       sig: Optional[torch.Tensor] = None) -> None:
        """the library becomes the semantically distinct members of ``forest`` on the datapoints, or with ``source="subtrees"`` of its
        subtrees of ``min_size`` to ``max_size`` nodes (``SemanticLibrary.update_library``); a shared library changes for every
        operator that holds it.  One host synchronisation, two with ``source="subtrees"``.  ``sig``: the forest's
        ``SR_subtree_signatures`` on the library's datapoints, when the caller already has them."""
        self.semantic_library.update_library(forest, source, min_size, max_size, sig=sig)

    def _refresh(self, forest: Forest) -> None:
        """called once per call of the operator, before it reads the library"""
        if not self.refresh_every:
            return
        self._refresh_calls += 1
        if self._refresh_calls % self.refresh_every == 0:
            self.update_library(forest, source="subtrees", max_size=self.refresh_max_size)
