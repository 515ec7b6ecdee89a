"""EBGCN for inference: the reference's module structure and state_dict on the HIP path.

Mirrors ``model/Twitter/EBGCN.py:23-230`` (``TDrumorGCN``, ``BUrumorGCN``, ``EBGCN``).  Module
and parameter names and shapes are the reference's - the five per-direction networks
(``sim_network`` and the Bayesian ``W_mean`` / ``W_bias`` / ``B_mean`` / ``B_bias``), ``fc1``,
``fc2``, ``bn1`` and every ``num_batches_tracked`` included - so a checkpoint's
``model_state_dict`` loads with ``load_state_dict(..., strict=True)``.

This is the inference-only path: ``model.eval()(data)`` returns ``(log_probs, None, None)``.
The reference's evaluation loop (``EBGCN.py:338``) discards both edge losses, which depend on a
``th.normal`` draw; the Bayesian networks are therefore carried (for the checkpoint) but never
run.  In training mode ``forward`` raises ``NotImplementedError``.

Per direction (``EBGCN.py:61-93``): conv1 -> :func:`bigcn_amd.ops.edge_infer` (the
edge-inference kernel) -> conv2's lin over ``relu(bn1(cat(h1, x[root])))``
(:func:`bigcn_amd.ops.ebgcn_conv2_lin`) -> conv2's aggregation with ``edge_weight = edge_pred``
(``build_graph`` + ``spmm``) -> ``[relu(h2) | h1[root]]`` -> ``scatter_mean``.  No dropout: the
reference's EBGCN forward applies none.
"""
from __future__ import annotations

from collections import OrderedDict

import torch

from . import _lib
from ._lib import check, ptr, stream_handle
from .bigcn import _num_graphs
from .conv import GCNConv
from .ops import _NO_TRAINING, build_graph, ebgcn_conv2_lin, edge_infer, gcn_conv, scatter_mean, spmm


def _edge_network(hidden: int, name: str) -> torch.nn.Sequential:
    """One of the five per-edge networks of a direction (``create_network``, ``EBGCN.py:33-46``):
    Conv1d(k=1, no bias) -> BatchNorm1d -> LeakyReLU -> Conv1d(hidden -> 1, k=1); the layer
    names carry the network's prefix (``sim_valconv0``, ``W_meannorm0``, ...)."""
    return torch.nn.Sequential(OrderedDict([
        (name + "conv0", torch.nn.Conv1d(hidden, hidden, kernel_size=1, bias=False)),
        (name + "norm0", torch.nn.BatchNorm1d(hidden)),
        (name + "relu0", torch.nn.LeakyReLU()),
        (name + "conv_out", torch.nn.Conv1d(hidden, 1, kernel_size=1)),
    ]))


class _EdgeRumorGCN(torch.nn.Module):
    """Shared body of ``TDrumorGCN`` (``EBGCN.py:23-116``) / ``BUrumorGCN`` (``:119-212``)."""

    edge_key = "edge_index"
    infer_flag = "edge_infer_td"

    def __init__(self, args):
        super().__init__()
        F, H, O = int(args.input_features), int(args.hidden_features), int(args.output_features)
        if H != 64 or O != 64:
            raise ValueError("the MI355X EBGCN path is specialised for hidden_features = output_features = 64 "
                             "(the reference configuration)")
        if not 1 <= int(args.edge_num) <= 8:
            raise ValueError("edge_num must be in [1, 8]")
        if F % 4:
            raise ValueError("input_features must be a multiple of 4")
        self.args = args
        self.conv1 = GCNConv(F, H)
        self.conv2 = GCNConv(F + H, O)
        self.device = getattr(args, "device", None)
        self.sim_network = _edge_network(H, "sim_val")
        self.W_mean = _edge_network(H, "W_mean")
        self.W_bias = _edge_network(H, "W_bias")
        self.B_mean = _edge_network(H, "B_mean")
        self.B_bias = _edge_network(H, "B_bias")
        self.fc1 = torch.nn.Linear(H, int(args.edge_num), bias=False)
        self.fc2 = torch.nn.Linear(H, int(args.edge_num), bias=False)
        self.dropout = torch.nn.Dropout(getattr(args, "dropout", 0.5))   # held, never applied (:57)
        self.bn1 = torch.nn.BatchNorm1d(H + F)

    def edge_infer(self, x, edge_index, status=None):
        """``(None, edge_pred [E])``: the reference returns ``(edge_loss, edge_pred)``
        (``:95-116``); the loss needs the Bayesian draw and is not computed here."""
        return None, edge_infer(x, edge_index, self, status=status)

    def _encode(self, data, status):
        x = data.x.float()
        ei = getattr(data, self.edge_key)
        batch, rootindex = data.batch, data.rootindex
        N = x.size(0)
        g = build_graph(ei, N, degree_on=self.conv1.degree_on)
        h1 = gcn_conv(x, g, self.conv1.lin.weight, self.conv1.bias)            # :64
        infer = bool(getattr(self.args, self.infer_flag))
        edge_pred = self.edge_infer(h1, ei, status)[1] if infer else None      # :67-70
        # :72-82 cat, bn1 (skipped for a one-node batch, :80), relu; :84 conv2's lin
        z2 = ebgcn_conv2_lin(h1, x, batch, rootindex, self.conv2.lin.weight, self.bn1 if N != 1 else None,
                             status=status)
        if edge_pred is not None and edge_pred.numel():
            g = build_graph(ei, N, edge_weight=edge_pred, degree_on=self.conv2.degree_on)
        h2 = spmm(g, z2, bias=self.conv2.bias, relu=True)                      # :84-85
        status |= g.status
        root_of_node = rootindex[batch]
        h = torch.cat((h2, h1.index_select(0, root_of_node)), 1)               # :86-90
        return scatter_mean(h, batch, dim=0, dim_size=_num_graphs(data)), edge_pred   # :92

    def forward(self, data):
        """``(x [B, 128], None)`` - the reference's ``(x, edge_loss)`` (``:93``) in eval mode."""
        if self.training:
            raise NotImplementedError(_NO_TRAINING)
        with torch.no_grad():
            status = torch.zeros(1, dtype=torch.int32, device=data.x.device)
            out, _ = self._encode(data, status)
            _raise_on(status)
        return out, None


def _raise_on(status: torch.Tensor) -> None:
    if int(status.item()) & 1:   # one host sync per forward
        raise IndexError("the batch holds an edge, root or tree index out of range")


class TDrumorGCN(_EdgeRumorGCN):
    edge_key = "edge_index"
    infer_flag = "edge_infer_td"


class BUrumorGCN(_EdgeRumorGCN):
    edge_key = "BU_edge_index"
    infer_flag = "edge_infer_bu"


class EBGCN(torch.nn.Module):
    """``EBGCN(args)`` (``EBGCN.py:215-230``) for inference.  ``args``: a namespace with the
    reference's fields ``input_features``, ``hidden_features`` (64), ``output_features`` (64),
    ``num_class`` (<= 16), ``edge_num`` (1..8), ``edge_infer_td``, ``edge_infer_bu``, ``device``.

    ``model.eval()(data)`` returns ``(log_probs [B, num_class], None, None)``; with
    ``edge_infer_td`` / ``edge_infer_bu`` false that direction's conv2 runs without edge
    weights.  ``last_edge_pred`` keeps the two directions' ``edge_pred`` of the last forward."""

    def __init__(self, args):
        super().__init__()
        if not 0 < int(args.num_class) <= 16:
            raise ValueError("num_class must be in [1, 16]")
        self.args = args
        self.TDrumorGCN = TDrumorGCN(args)
        self.BUrumorGCN = BUrumorGCN(args)
        self.fc = torch.nn.Linear((int(args.hidden_features) + int(args.output_features)) * 2, int(args.num_class))
        self.last_edge_pred = (None, None)

    def forward(self, data):
        if self.training:
            raise NotImplementedError(_NO_TRAINING)
        with torch.no_grad():
            status = torch.zeros(1, dtype=torch.int32, device=data.x.device)
            td_x, td_pred = self.TDrumorGCN._encode(data, status)
            bu_x, bu_pred = self.BUrumorGCN._encode(data, status)
            self.last_edge_pred = (td_pred, bu_pred)
            head = torch.cat((bu_x, td_x), 1).contiguous()                     # :227, BU first
            w, b = self.fc.weight.detach().float().contiguous(), self.fc.bias.detach().float().contiguous()
            B, C = head.size(0), w.size(0)
            logp = torch.empty(B, C, dtype=torch.float32, device=head.device)
            check(_lib.lib().bgcn_head_forward(ptr(head), ptr(w), ptr(b), B, C, ptr(logp), stream_handle()))  # :228-229
            _raise_on(status)
        return logp, None, None
