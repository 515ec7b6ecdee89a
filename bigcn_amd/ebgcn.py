"""EBGCN: the reference's module structure and state_dict on the HIP path.

Mirrors ``model/Twitter/EBGCN.py:23-230`` (``TDrumorGCN``, ``BUrumorGCN``, ``EBGCN``).  Module
and parameter names and shapes are the reference's - the five per-direction networks
(``sim_network`` and the Bayesian ``W_mean`` / ``W_bias`` / ``B_mean`` / ``B_bias``), ``fc1``,
``fc2``, ``bn1`` and every ``num_batches_tracked`` included - so a checkpoint's
``model_state_dict`` loads with ``load_state_dict(..., strict=True)``.

Inference: ``model.eval()(data)`` returns ``(log_probs, None, None)``.
The reference's evaluation loop (``EBGCN.py:338``) discards both edge losses, which depend on a
``th.normal`` draw; the Bayesian networks are therefore carried (for the checkpoint) but never
run.  In training mode ``forward`` raises ``NotImplementedError``; the training forward is
:meth:`EBGCN.train_forward` (autograd throughout, the edge inference of both directions on
:func:`bigcn_amd.ops.edge_infer_train`).

Per direction (``EBGCN.py:61-93``): conv1 -> :func:`bigcn_amd.ops.edge_infer` (the
edge-inference kernel) -> conv2's lin over ``relu(bn1(cat(h1, x[root])))``
(:func:`bigcn_amd.ops.ebgcn_conv2_lin`) -> conv2's aggregation with ``edge_weight = edge_pred``
(``build_graph`` + ``spmm``) -> ``[relu(h2) | h1[root]]`` -> ``scatter_mean``.  No dropout: the
reference's EBGCN forward applies none.
"""
from __future__ import annotations

import ctypes
from collections import OrderedDict

import torch

from . import _lib
from ._lib import check, ptr, raise_on_status, stream_handle
from .bigcn import _num_graphs
from .conv import GCNConv
from .ops import (_NO_TRAINING, _check_ei, _i64c, build_graph, degree_code, ebgcn_conv2_lin, ebgcn_conv2_lin_train,
                  edge_infer, edge_infer_train, gcn_aggregate, gcn_conv, scatter_mean, spmm)


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

    def edge_infer(self, x, edge_index, status=None, noise=None, generator=None):
        """``(edge_loss, edge_pred [E])`` (``:95-116``).  In training mode both come from
        :func:`bigcn_amd.ops.edge_infer_train` and carry gradients; in eval mode the loss, which
        needs the Bayesian draw and which the evaluation loop drops, is ``None``."""
        if self.training:
            return edge_infer_train(x, edge_index, self, noise=noise, generator=generator, status=status)
        return None, edge_infer(x, edge_index, self, status=status)

    def _train_encode(self, data, noise, generator, status, graph_status=None):
        """The training forward of one direction (``:61-93``) with autograd: ``(x [B, 128],
        edge_loss or None)``.  The ``[N, 64 + F]`` concat is never formed (a one-node batch, whose bn1
        the reference skips, keeps the torch composition).  Nothing here reads ``status`` on the
        host.  ``graph_status``: the word the convolutions' graph builds OR their own status
        words into (``None``: they stay with the graphs, unread)."""
        x = data.x.float()
        ei = getattr(data, self.edge_key)
        batch, rootindex = data.batch, data.rootindex
        N = x.size(0)
        h1 = gcn_conv(x, ei, self.conv1.lin.weight, self.conv1.bias, degree_on=self.conv1.degree_on,
                      status=graph_status)                                     # :64
        edge_loss = edge_pred = None
        if bool(getattr(self.args, self.infer_flag)):                          # :67-70
            edge_loss, edge_pred = edge_infer_train(h1, ei, self, noise=noise, generator=generator, status=status)
        # a root outside [0, N) is flagged by conv2's lin; the torch gathers below read a clamped row
        # (the step is invalid either way), never memory outside h1 / x
        root_of_node = rootindex[batch].clamp(0, max(N - 1, 0))
        if N != 1:
            # :72-84 cat, bn1 on batch statistics, relu and conv2's lin without the concat, then conv2's
            # aggregation
            z2 = ebgcn_conv2_lin_train(h1, x, batch, rootindex, self.conv2.lin.weight, self.bn1, status=status)
            h2 = gcn_aggregate(z2, ei, self.conv2.bias, edge_weight=edge_pred, degree_on=self.conv2.degree_on,
                               status=graph_status)
        else:                                                                  # :80-81, bn1 skipped
            cat = torch.relu(torch.cat((h1, x.index_select(0, root_of_node)), 1))
            h2 = gcn_conv(cat, ei, self.conv2.lin.weight, self.conv2.bias, edge_weight=edge_pred,
                          degree_on=self.conv2.degree_on, status=graph_status)  # :84
        # :65 x2 = copy.copy(x) is a copy outside the autograd graph: as in the reference, no
        # gradient reaches conv1 through the root rows of the readout (:86-90)
        h = torch.cat((torch.relu(h2), h1.detach().index_select(0, root_of_node)), 1)
        return scatter_mean(h, batch, dim=0, dim_size=_num_graphs(data)), edge_loss   # :92

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
    raise_on_status(int(status.item()), bits=1)   # one host sync per forward


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

    def train_forward(self, data, noise=None, generator=None):
        """The reference's training forward (``EBGCN.py:61-93``, ``:223-230``) with autograd
        throughout: ``(log_probs [B, num_class], TD_edge_loss, BU_edge_loss)``, whatever
        ``self.training`` says for the BatchNorms (batch statistics, running statistics updated).
        A direction whose ``edge_infer_*`` flag is off returns the loss ``None`` and runs conv2
        without edge weights.  ``noise``: a pair ``(td, bu)`` of standard-normal draws ``[E, 64]``
        for the two Bayesian branches (``None``: drawn from ``generator``).

        Per direction it composes ``gcn_conv`` (conv1), :func:`bigcn_amd.ops.edge_infer_train` (fused),
        :func:`bigcn_amd.ops.ebgcn_conv2_lin_train` (fused: batch-statistics bn1, relu and conv2's lin
        without the dense ``[N, 64 + F]`` concat), :func:`bigcn_amd.ops.gcn_aggregate` with
        ``edge_weight=edge_pred`` and ``scatter_mean``; conv1 and the readout are separate calls
        (:class:`bigcn_amd.EBGCNTrainStep` is the loop body around this forward, without its sync).  An index out of range raises ``IndexError`` at the end of
        the call (one host sync); the BatchNorms have by then been updated from the valid part of
        the batch (a direction without one valid edge leaves its per-edge norms untouched)."""
        status = torch.zeros(1, dtype=torch.int32, device=data.x.device)
        out = self._train_body(data, noise, generator, status)
        _raise_on(status)
        return out

    def _train_body(self, data, noise, generator, status, graph_status=None):
        """:meth:`train_forward` without its host sync: flags go into ``status`` (and the graph builds'
        into ``graph_status``, see ``_train_encode``), which is not read here."""
        td_noise, bu_noise = (None, None) if noise is None else noise
        td_x, td_loss = self.TDrumorGCN._train_encode(data, td_noise, generator, status, graph_status)
        bu_x, bu_loss = self.BUrumorGCN._train_encode(data, bu_noise, generator, status, graph_status)
        out = self.fc(torch.cat((bu_x, td_x), 1))                              # :227-228, BU first
        return torch.nn.functional.log_softmax(out, dim=1), td_loss, bu_loss   # :229-230

    # ---- the evaluation loop (EBGCN.py:328-354) as one native call per batch
    def _eval_tensors(self):
        """The tensors ``bgcn_ebgcn_eval_args`` points at, in struct order (TD, BU, fc)."""
        out = []
        for d in (self.TDrumorGCN, self.BUrumorGCN):
            sim = d.sim_network
            out += [d.conv1.lin.weight, d.conv1.bias, d.conv2.lin.weight, d.conv2.bias,
                    d.bn1.weight, d.bn1.bias, d.bn1.running_mean, d.bn1.running_var,
                    sim.sim_valconv0.weight, sim.sim_valnorm0.weight, sim.sim_valnorm0.bias,
                    sim.sim_valnorm0.running_mean, sim.sim_valnorm0.running_var,
                    sim.sim_valconv_out.weight, sim.sim_valconv_out.bias, d.fc1.weight]
        return out + [self.fc.weight, self.fc.bias]

    def _eval_bind(self, dev):
        """The pointer struct, refilled only when a parameter was rebound, moved or (a tensor the
        kernels cannot read in place: not fp32 / contiguous / on ``dev``) changed."""
        src = self._eval_tensors()
        direct = [t.dtype == torch.float32 and t.is_contiguous() and t.device == dev for t in src]
        convs = (self.TDrumorGCN.conv1, self.TDrumorGCN.conv2, self.BUrumorGCN.conv1, self.BUrumorGCN.conv2)
        settings = tuple(c.degree_on for c in convs) + (bool(self.args.edge_infer_td), bool(self.args.edge_infer_bu),
                                                        self.TDrumorGCN.bn1.eps, self.BUrumorGCN.bn1.eps)
        key = (dev, settings) + tuple((t.data_ptr(), t.dtype, None if ok else t._version)
                                      for t, ok in zip(src, direct))
        st = self.__dict__.get("_eval_state")
        if st is not None and st["key"] == key:
            return st
        if len({c.degree_on for c in convs}) != 1:
            raise ValueError("evaluate needs one degree_on for all four convolutions")
        held = [t.detach() if ok else t.detach().to(device=dev, dtype=torch.float32).contiguous()
                for t, ok in zip(src, direct)]
        a = _lib.EbgcnEvalArgs()
        names = [n for n, _ in _lib.EbgcnDir._fields_[:16]]
        for k, (sub, d) in enumerate(((a.td, self.TDrumorGCN), (a.bu, self.BUrumorGCN))):
            for j, n in enumerate(names):
                setattr(sub, n, held[16 * k + j].data_ptr())
            sub.bn1_eps, sub.sim_norm_eps = d.bn1.eps, d.sim_network.sim_valnorm0.eps
            sub.infer = int(bool(getattr(self.args, d.infer_flag)))
        a.fc_w, a.fc_b = held[32].data_ptr(), held[33].data_ptr()
        a.in_feats, a.num_classes = int(self.args.input_features), int(self.args.num_class)
        a.edge_num, a.degree_on = int(self.args.edge_num), degree_code(convs[0].degree_on)
        if st is None or st["status"].device != dev:   # the workspace and the status words outlive a rebinding
            st = {"status": torch.zeros(1, dtype=torch.int32, device=dev),
                  "seen": torch.zeros(1, dtype=torch.int32, device=dev), "ws": None, "sizes": None}
            self.__dict__["_eval_state"] = st
        a.status = st["status"].data_ptr()
        st.update(key=key, args=a, held=held)
        return st

    def evaluate(self, data, logp=None, pred=False):
        """One batch of the reference's test loop (``EBGCN.py:328-354``: ``val_out, _, _ =
        model(Batch_data); val_loss = F.nll_loss(val_out, y); _, val_pred = val_out.max(dim=1);
        correct = val_pred.eq(y).sum()``) as one call (``bgcn_ebgcn_eval_step``), in eval mode
        whatever ``model.training`` says and with no host sync.

        Returns ``(loss, correct)`` (0-dim fp32 / int32 device tensors), plus ``pred`` ([B] int64)
        when ``pred=True``.  ``logp``: an optional contiguous fp32 [B, C] output.  Sets
        ``last_edge_pred``.  Validity of the batch's indices: :meth:`check_status`."""
        x = data.x
        dev = x.device
        if not x.is_cuda:
            raise _lib.BGCNError("bigcn_amd ops take device tensors (no CPU path)")
        st = self._eval_bind(dev)
        a = st["args"]
        x = x if x.dtype == torch.float32 and x.stride(-1) == 1 and x.dim() == 2 else x.float().contiguous()
        td_ei, bu_ei = _check_ei(data.edge_index), _check_ei(data.BU_edge_index)
        batch, rootindex, y = _i64c(data.batch), _i64c(data.rootindex), _i64c(data.y)
        N, F, B = int(x.size(0)), int(x.size(1)), _num_graphs(data)
        Etd, Ebu = int(td_ei.size(1)), int(bu_ei.size(1))
        C = int(a.num_classes)
        if F != a.in_feats:
            raise ValueError(f"data.x has {F} features, the model takes {a.in_feats}")
        if rootindex.numel() != B or y.numel() != B or batch.numel() != N:
            raise ValueError("batch must have one entry per node, rootindex and y one per tree")
        if logp is not None and (logp.dtype != torch.float32 or not logp.is_contiguous() or logp.numel() != B * C
                                 or logp.device != dev):
            raise ValueError("logp must be a contiguous fp32 [B, C] tensor")
        L = _lib.lib()
        sizes = (N, B, F, Etd, Ebu)
        if st["sizes"] != sizes:
            need = L.bgcn_ebgcn_eval_workspace_size(N, B, F, Etd, Ebu, int(a.edge_num))
            if st["ws"] is None or st["ws"].numel() < need or st["ws"].device != dev:
                st["ws"] = _lib.workspace(need, dev)
            st["sizes"] = sizes
        ws = st["ws"]
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        correct = torch.empty(1, dtype=torch.int32, device=dev)
        pr = torch.empty(B, dtype=torch.int64, device=dev) if pred else None
        td_pred = torch.empty(Etd, dtype=torch.float32, device=dev) if a.td.infer else None
        bu_pred = torch.empty(Ebu, dtype=torch.float32, device=dev) if a.bu.infer else None
        b = a.batch
        b.x, b.ldx, b.num_nodes, b.num_graphs = x.data_ptr(), x.stride(0), N, B
        b.batch, b.rootindex = batch.data_ptr(), rootindex.data_ptr()
        b.td_edge_index, b.td_num_edges, b.bu_edge_index, b.bu_num_edges = ptr(td_ei), Etd, ptr(bu_ei), Ebu
        b.x_dtype = _lib.BGCN_DTYPE_F32
        a.y, a.logp, a.loss, a.correct, a.pred = y.data_ptr(), ptr(logp), loss.data_ptr(), correct.data_ptr(), ptr(pr)
        a.td_edge_pred, a.bu_edge_pred = ptr(td_pred), ptr(bu_pred)
        check(L.bgcn_ebgcn_eval_step(ctypes.addressof(a), ptr(ws), ws.numel(), stream_handle()))
        st["seen"].bitwise_or_(st["status"])   # the call zeroes its status word; check_status reads this one
        self.last_edge_pred = (td_pred, bu_pred)
        out = (loss.view(()), correct.view(()))
        return out + (pr,) if pred else out

    def validate(self, batches, metrics=None):
        """The reference's test loop (``EBGCN.py:328-354``) without a host sync: every batch goes
        through ``evaluate(batch, pred=True)`` and its loss, correct count, predictions and labels
        into ``metrics.add(...)`` (:class:`bigcn_amd.metrics.EpochMetrics`; records are appended,
        by default a new one sized for ``batches``).  Returns it; ``result()`` is the epoch's one
        device-to-host read.  Validity of the batches themselves: :meth:`check_status`."""
        from .metrics import EpochMetrics
        batches = list(batches)
        if metrics is None:
            if not batches:
                raise ValueError("validate needs at least one batch")
            metrics = EpochMetrics(int(self.args.num_class), len(batches), batches[0].x.device)
        elif len(metrics) + len(batches) > metrics.max_batches:
            raise IndexError(f"metrics has room for {metrics.max_batches - len(metrics)} more batches, "
                             f"{len(batches)} given")
        for batch in batches:
            loss, correct, pred = self.evaluate(batch, pred=True)
            metrics.add(pred, batch.y, loss, correct)
        return metrics

    def check_status(self) -> None:
        """One host sync: raise the ``IndexError`` ``forward`` raises when any batch evaluated since
        the last check held an edge, root or tree index out of range (or a label outside
        ``[0, num_class)``)."""
        st = self.__dict__.get("_eval_state")
        if st is None:
            return
        s = int(st["seen"].item())
        st["seen"].zero_()
        raise_on_status(s, bits=1 | 2)
