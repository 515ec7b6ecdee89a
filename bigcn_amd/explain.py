"""The reference's analysis (``explain_PHEME.py``) on the HIP path, batched.

For every test tree the reference re-runs each direction stage by stage
(``extract_intermediates_bigcn`` ``:91-162``, ``extract_intermediates_ebgcn`` ``:165-242``), sums
every node's activation row after each stage and ranks all nodes by that sum with
``torch.topk(row_sum, k=n)``.  Its ``topk`` ranks the whole batch at once, so it runs at batch
size 1 with a Python loop per tree.  Here one :func:`explain` call takes a normal batch:

* the stage sums come from one kernel sequence (:func:`bigcn_amd.ops.explain_sums`) that never
  builds the ``[N, 64 + F]`` concatenations - a tree's root terms are computed once per tree;
* the ranking is per tree, on the device (:func:`bigcn_amd.ops.segment_rank`), with a fixed order
  for ties (ascending node index), which ``torch.topk`` leaves unspecified;
* :meth:`Explanation.to_reference_dict` gives the reference's per-tree record.

Inference only: a model in training mode is refused.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from ._lib import raise_on_status
from .bigcn import _num_graphs
from .ops import (STAGES_BIGCN, STAGES_EBGCN, _segment_rank, build_graph, ebgcn_conv2_lin, edge_infer, explain_sums,
                  gcn_conv, scatter_mean, segment_rank, spmm)

__all__ = ["explain", "explain_direction", "segment_rank", "Explanation", "DirectionExplanation"]


@dataclass
class DirectionExplanation:
    """One direction of one batch: ``sums`` [S, N] fp32 (stage-major), ``order`` [S, N] int32 (per
    tree: local node indices by descending sum), ``sorted`` [S, N] (the sums in that order),
    ``stage_names`` (the reference's keys, S of them) and ``gcn_output`` [B, 128]."""
    sums: torch.Tensor
    order: torch.Tensor
    sorted: torch.Tensor
    stage_names: Tuple[str, ...]
    gcn_output: torch.Tensor


def _raise_on(status: torch.Tensor) -> None:
    # one host sync per public call
    raise_on_status(int(status.item()), bits=1, index_also=", or a batch vector that decreases")


def _batch_of_one_edges(ei, batch, N, B):
    """The edge list whose ``edge_infer`` reads what a batch of one tree would: the reference reads
    node ``id - 1`` and lets id 0 wrap to the LAST node (``EBGCN.py:97-99``), which in a batch of one
    is the tree's own last node.  A tree's first node is therefore renamed to the id after its last
    node (mod N), every other id keeps its meaning."""
    trees = torch.arange(B, device=batch.device)
    first, end = torch.searchsorted(batch, trees), torch.searchsorted(batch, trees, right=True)
    tb = batch[ei.clamp(0, N - 1)].clamp(0, B - 1)
    return torch.where(ei == first[tb], end[tb] % N, ei)


def _direction(mod, data, status, want_x_sum, batch_of_one=False):
    if mod.training:
        raise ValueError("explain needs the model in eval mode (call model.eval())")
    x = data.x.float()
    ei = getattr(data, mod.edge_key)
    batch, rootindex = data.batch, data.rootindex
    N, B = x.size(0), _num_graphs(data)
    bn1 = getattr(mod, "bn1", None)            # EBGCN's directions have it, BiGCN's do not
    g = build_graph(ei, N, degree_on=mod.conv1.degree_on)
    h1 = gcn_conv(x, g, mod.conv1.lin.weight, mod.conv1.bias)
    if bn1 is not None and ei.size(1):
        # the reference's explain code infers the edge weights whatever args.edge_infer_* says (:176)
        ei_infer = _batch_of_one_edges(ei, batch.to(torch.int64).contiguous(), N, B) if batch_of_one else ei
        pred = edge_infer(h1, ei_infer, mod, status=status)
        status |= g.status
        g = build_graph(ei, N, edge_weight=pred, degree_on=mod.conv2.degree_on)
    # conv2's lin over relu([bn1](cat(h1, x[root]))) without the cat; bn1 = None is BiGCN's eval form
    z2 = ebgcn_conv2_lin(h1, x, batch, rootindex, mod.conv2.lin.weight, bn1, status=status)
    h2 = spmm(g, z2, bias=mod.conv2.bias, relu=False)     # conv2's output before its relu
    status |= g.status
    sums, x_sum = explain_sums(h1, h2, x, batch, rootindex, bn1, want_x_sum=want_x_sum, status=status)
    order, srt = _segment_rank(sums, batch, B, status)
    # a bad index is reported through status; the gather below must not read past the arrays
    root_of_node = rootindex.clamp(0, max(N - 1, 0))[batch.clamp(0, max(B - 1, 0))]
    head = torch.cat((torch.relu(h2), h1.index_select(0, root_of_node)), 1)
    out = scatter_mean(head, batch, dim=0, dim_size=B)
    names = STAGES_BIGCN if bn1 is None else STAGES_EBGCN
    return DirectionExplanation(sums, order, srt, names, out), x_sum


def explain_direction(direction_module, data, batch_of_one: bool = False) -> DirectionExplanation:
    """The stage sums and per-tree rankings of one direction: ``direction_module`` is a
    ``TDrumorGCN`` / ``BUrumorGCN`` of :mod:`bigcn_amd.bigcn` or :mod:`bigcn_amd.ebgcn` (the
    family is told by whether the module has ``bn1``), in eval mode.

    conv1 -> (EBGCN, if the batch has edges: ``edge_infer``, always, as the reference's explain
    code does at ``:176``) -> conv2's lin over ``relu(cat(h1, x[root]))`` / ``relu(bn1(cat))`` ->
    conv2's aggregation without its relu -> ``explain_sums`` -> ``segment_rank`` -> ``scatter_mean``
    of ``[relu(h2) | h1[root]]``.

    The reference's explain path applies ``bn1`` even to a one-node batch (``:198``), where
    ``EBGCN.forward`` skips it (``EBGCN.py:80``); this function follows the explain path, so for a
    one-node batch its later stages differ from what the classifier computes.

    ``batch_of_one`` (EBGCN only; BiGCN's trees never see each other): the reference's
    ``edge_infer`` reads node ``id - 1`` and lets id 0 wrap to the batch's last node.  By default
    that is reproduced as written on the batch given, as ``EBGCN.forward`` does, so an edge at a
    tree's first node reads the previous tree's last node.  With ``batch_of_one=True`` the wrap
    stays inside each tree: every tree gets exactly what the reference's explain loop, which runs
    at batch size 1, computes for it."""
    with torch.no_grad():
        status = torch.zeros(1, dtype=torch.int32, device=data.x.device)
        res, _ = _direction(direction_module, data, status, False, batch_of_one)
        _raise_on(status)
    return res


@dataclass
class Explanation:
    """What :func:`explain` returns for one batch.  ``x_sum`` [N], ``x_order`` / ``x_sorted`` [N]
    (its per-tree ranking), ``td`` / ``bu`` (:class:`DirectionExplanation`), ``log_probs`` [B, C]
    of the model's normal forward, ``prediction`` [B]; ``batch`` / ``rootindex`` / ``y`` are the batch's."""
    x_sum: torch.Tensor
    x_order: torch.Tensor
    x_sorted: torch.Tensor
    td: DirectionExplanation
    bu: DirectionExplanation
    log_probs: torch.Tensor
    prediction: torch.Tensor
    batch: torch.Tensor
    rootindex: torch.Tensor
    _ptr: Optional[list] = None
    y: Optional[torch.Tensor] = None   # the batch's labels [B] (None: the batch had none)

    def confusion(self, num_classes: int = 4, out: Optional[torch.Tensor] = None,
                  status: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``prediction`` counted against the batch's ``y`` on the device: the int32 ``[C, C]``
        matrix (row = actual, column = predicted) the reference's explain run keeps per fold
        (``explain_PHEME.py:480, 609``).  With ``out`` the counts are ADDED to it - one zeroed
        buffer over a fold's batches gives the fold's matrix.  No host sync
        (:func:`bigcn_amd.metrics.confusion`; a label outside ``[0, C)`` sets bit 0 of ``status``)."""
        from .metrics import confusion
        if self.y is None:
            raise ValueError("the explained batch has no labels (y)")
        return confusion(self.prediction, self.y, num_classes, out=out, accumulate=out is not None, status=status)

    def tree_ptr(self) -> list:
        """First node of every tree (B + 1 entries), on the host."""
        if self._ptr is None:
            B = int(self.log_probs.size(0))
            counts = torch.bincount(self.batch.cpu(), minlength=B)
            self._ptr = [0] + torch.cumsum(counts, 0).tolist()
        return self._ptr

    def to_reference_dict(self, t: int) -> dict:
        """Tree ``t``'s record as the reference builds it per sample (``explain_PHEME.py:482-607``),
        in plain Python lists: ``x_sum_top_k`` and per direction ``<stage>_topk`` are ``[indices,
        values]`` (indices local to the tree), ``gcn_output`` one list of one row (the reference's
        batch of one), ``rootindex`` local, ``prediction`` an int.  ``tweetids``, node swapping and
        writing files stay with the caller."""
        p = self.tree_ptr()
        if not 0 <= t < len(p) - 1:
            raise IndexError("tree index out of range")
        a, b = p[t], p[t + 1]

        def direction(d: DirectionExplanation) -> dict:
            o, v = d.order[:, a:b].cpu(), d.sorted[:, a:b].cpu()
            rec = {name + "_topk": [o[s].tolist(), v[s].tolist()] for s, name in enumerate(d.stage_names)}
            rec["gcn_output"] = [d.gcn_output[t].tolist()]
            return rec

        return {
            "rootindex": int(self.rootindex[t]) - a,
            "x_sum_top_k": [self.x_order[a:b].tolist(), self.x_sorted[a:b].tolist()],
            "td_gcn_explanations": direction(self.td),
            "bu_gcn_explanations": direction(self.bu),
            "prediction": int(self.prediction[t]),
        }


def explain(model, data, batch_of_one: bool = False) -> Explanation:
    """The body of ``explain_PHEME.py``'s per-sample loop (``:530-607``) for a whole batch:
    ``model`` is a ``BiGCN``, ``Net`` or ``EBGCN`` of this package in eval mode (``ValueError``
    otherwise), ``data`` a normal multi-tree batch.  A ``TreeBERT`` takes the BERT branch (``:581-600``)
    and returns its :class:`bigcn_amd.bert.BertExplanation` (:meth:`TreeBERT.explain_batch`).  Runs under ``torch.no_grad()`` with one host
    sync at the end; an index out of range, or a ``batch`` vector that decreases, raises
    ``IndexError``.  ``batch_of_one``: see :func:`explain_direction`; it changes the stage sums
    only, ``log_probs`` are always the model's normal forward on ``data``."""
    if model.training:
        raise ValueError("explain needs the model in eval mode (call model.eval())")
    from .bert import TreeBERT
    if isinstance(model, TreeBERT):
        return model.explain_batch(data)
    with torch.no_grad():
        status = torch.zeros(1, dtype=torch.int32, device=data.x.device)
        B = _num_graphs(data)
        td, x_sum = _direction(model.TDrumorGCN, data, status, True, batch_of_one)
        bu, _ = _direction(model.BUrumorGCN, data, status, False, batch_of_one)
        x_order, x_sorted = _segment_rank(x_sum, data.batch, B, status)
        out = model(data)
        log_probs = out[0] if isinstance(out, tuple) else out     # EBGCN returns (log_probs, None, None)
        prediction = log_probs.argmax(dim=-1)
        _raise_on(status)
    return Explanation(x_sum, x_order[0], x_sorted[0], td, bu, log_probs, prediction, data.batch, data.rootindex,
                       y=getattr(data, "y", None))
