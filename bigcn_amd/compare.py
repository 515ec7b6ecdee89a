"""The reference's comparison (``compare_similarity.py``) on the HIP path, batched.

The reference's study has three steps: ``explain_PHEME.py`` ranks every tree's nodes by per-stage
activation sums (:func:`bigcn_amd.explain`), a centrality file per tree ranks the same nodes by
out-degree, betweenness and closeness, and ``compute_metrics`` (``compare_similarity.py:38-183``)
scores every pair of those rankings per tree - Pearson, Spearman, Kendall tau, Somers' D and
Jaccard over the top-k lists - one tree at a time through scipy.  Here one :func:`compare` call
takes a normal batch:

* the centralities come from :func:`bigcn_amd.ops.tree_centrality`.  The script that wrote the
  reference's centrality files is not part of it; the definition taken is networkx's
  ``out_degree_centrality``, ``betweenness_centrality`` and ``closeness_centrality`` on the
  ``DiGraph`` of a tree's top-down edges with default arguments, in closed form (child count,
  depth, subtree size).  Nodes with equal integer keys get bit-equal values and rank by ascending
  node index (:func:`bigcn_amd.ops.segment_rank`'s tie rule);
* the statistics come from :func:`bigcn_amd.ops.rank_similarity`, one workgroup per tree.  The
  reference skips every tree of at most k nodes, so each compared list holds k distinct indices:
  no ties, tau-b = tau-a = Somers' D, and everything but the two correlations' square root is
  exact integer arithmetic;
* :meth:`Similarity.summarise` is the reference's ``summarise_metrics`` (``:186-214``), and
  :meth:`Similarity.cat` joins the batches of a fold.

Node swapping (``randomise``) and file I/O stay with the caller, as they do for ``explain``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Mapping, Optional, Sequence, Tuple

import torch

from .bigcn import _num_graphs
from .explain import Explanation, explain
from .ops import (CENTRALITY_NAMES, METRIC_NAMES, _raise_on_compare_status, _rank_similarity, _segment_rank,
                  _tree_centrality, rank_similarity, tree_centrality)

__all__ = ["compare", "ranking_names", "tree_centrality", "rank_similarity", "Similarity", "CENTRALITY_NAMES",
           "METRIC_NAMES"]


@dataclass
class Similarity:
    """What :func:`compare` returns.  ``names`` (V of them, the reference's ``vec``), ``matrix``
    [B, 5, V, V] float64 (metric order :data:`METRIC_NAMES`; zeros for a skipped tree), ``valid``
    [B] bool, ``k``; ``centrality`` [3, N] fp32 (rows :data:`CENTRALITY_NAMES`) with its per-tree
    ranking ``centrality_order`` / ``centrality_sorted`` [3, N] and the batch vector ``batch``
    (the last four are None after :meth:`cat`)."""
    names: Tuple[str, ...]
    matrix: torch.Tensor
    valid: torch.Tensor
    k: int
    centrality: Optional[torch.Tensor] = None
    centrality_order: Optional[torch.Tensor] = None
    centrality_sorted: Optional[torch.Tensor] = None
    batch: Optional[torch.Tensor] = None
    _ptr: Optional[list] = None

    def summarise(self) -> torch.Tensor:
        """``[5, V, V]``: per entry the sum over trees divided by the number of trees where it is
        not zero (``compare_similarity.py:205``; a skipped tree's zeros, and a statistic that is
        exactly 0, do not count), NaN where that number is 0."""
        return self.matrix.sum(0) / torch.count_nonzero(self.matrix, dim=0)

    @staticmethod
    def cat(parts: Sequence["Similarity"]) -> "Similarity":
        """The trees of several batches (a fold's) as one: names and k must agree."""
        parts = list(parts)
        if not parts:
            raise ValueError("Similarity.cat needs at least one part")
        if any(p.names != parts[0].names or p.k != parts[0].k for p in parts):
            raise ValueError("Similarity.cat: the parts compare different rankings or use different k")
        return Similarity(parts[0].names, torch.cat([p.matrix for p in parts]), torch.cat([p.valid for p in parts]),
                          parts[0].k)

    def tree_ptr(self) -> list:
        """First node of every tree (B + 1 entries), on the host."""
        if self.batch is None:
            raise ValueError("no per-node data (the result of Similarity.cat)")
        if self._ptr is None:
            counts = torch.bincount(self.batch.cpu(), minlength=int(self.valid.numel()))
            self._ptr = [0] + torch.cumsum(counts, 0).tolist()
        return self._ptr

    def centrality_dict(self, t: int) -> dict:
        """Tree ``t``'s centrality record in the shape ``compare_similarity.py:87-93`` reads:
        ``{"out_degree": [indices, values], ...}``, indices local to the tree, best first."""
        p = self.tree_ptr()
        if not 0 <= t < len(p) - 1:
            raise IndexError("tree index out of range")
        a, b = p[t], p[t + 1]
        o, v = self.centrality_order[:, a:b].cpu(), self.centrality_sorted[:, a:b].cpu()
        return {name: [o[r].tolist(), v[r].tolist()] for r, name in enumerate(CENTRALITY_NAMES)}


def ranking_names(labels: Sequence[str], stages: Sequence[str] = ("conv1_output_sum", "conv2_output_sum"),
                  extra: Sequence[str] = ()) -> Tuple[str, ...]:
    """The names of the rankings :func:`compare` compares, in its (the reference's ``vec``) order:
    the centralities, per label ``<label>_td_<stage>`` for every stage then ``<label>_bu_<stage>``
    (a stage is named by its first word: ``conv1_output_sum`` -> ``conv1``), then ``extra``."""
    names = list(CENTRALITY_NAMES)
    for label in labels:
        names += [f"{label}_{d}_{stage.split('_')[0]}" for d in ("td", "bu") for stage in stages]
    names += [str(n) for n in extra]
    if len(set(names)) != len(names):
        raise ValueError(f"compare: the rankings' names repeat: {names}")
    return tuple(names)


def compare(data, explanations: Mapping[str, object], k: int = 10,
            stages: Sequence[str] = ("conv1_output_sum", "conv2_output_sum"),
            extra: Optional[Mapping[str, torch.Tensor]] = None, batch_of_one: bool = False) -> Similarity:
    """``compute_metrics`` (``compare_similarity.py:38-183``) for a whole batch.

    ``explanations`` maps a label to an :class:`bigcn_amd.explain.Explanation` of ``data`` or to a
    model, which is passed through ``explain(model, data, batch_of_one)``.  The compared rankings
    are, in the reference's order (:func:`ranking_names`): the three centralities of
    ``data.edge_index``, per label the chosen stages of its top-down then its bottom-up direction,
    then ``extra``: a name -> ``[N]`` value vector, ranked here per tree (the reference's BERT
    columns).  With labels ``bigcn`` and ``ebgcn`` the first 11 names are the reference's.  At
    most 32 rankings, ``k`` in [2, 32].

    One host sync per call (after the models' own): a node with two parents, an edge across trees
    or a cycle raises ValueError, an index out of range IndexError, a list that is not a ranking
    ValueError."""
    names = ranking_names(tuple(explanations), stages, tuple(extra or ()))
    with torch.no_grad():
        batch = data.batch
        B = _num_graphs(data)
        status = torch.zeros(1, dtype=torch.int32, device=batch.device)
        cent = _tree_centrality(data.edge_index, batch, B, status)
        cent_order, cent_sorted = _segment_rank(cent, batch, B, status)
        rows = [cent_order]
        for label, ex in explanations.items():
            if not isinstance(ex, Explanation):
                ex = explain(ex, data, batch_of_one)
            for d, res in (("td", ex.td), ("bu", ex.bu)):
                for stage in stages:
                    if stage not in res.stage_names:
                        raise ValueError(f"{label} has no stage {stage!r} (its stages: {res.stage_names})")
                    rows.append(res.order[res.stage_names.index(stage)].unsqueeze(0))
        for values in (extra or {}).values():
            rows.append(_segment_rank(values, batch, B, status)[0])
        sim, valid = _rank_similarity(torch.cat(rows), batch, k, B, status)
        _raise_on_compare_status(int(status.item()))   # the one host sync
    return Similarity(names, sim, valid.bool(), int(k), cent, cent_order, cent_sorted, batch)
