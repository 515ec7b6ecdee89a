"""The body of EBGCN's training loop (``model/Twitter/EBGCN.py:300-312``) without a host sync.

``EBGCNTrainStep.step(data)`` is one iteration: the training forward (``EBGCN._train_body``), the
loss ``nll_loss + edge_loss_td * TD_edge_loss + edge_loss_bu * BU_edge_loss`` with the training
accuracy and the gradient the backward starts from (one launch, ``bgcn_ebgcn_train_loss``),
``backward``, and the update of all 68 parameter tensors (one launch, :class:`MultiAdam`).  An
invalid batch - an edge, root or label out of range - is decided on the device: the loss kernel
turns the step's status word into the optimiser's ``skip_flag``, the update writes nothing, and
:meth:`EBGCNTrainStep.check_status` reports it with one read, whenever the caller asks.
"""
from __future__ import annotations

import types

import torch

from . import _lib
from ._lib import check, ptr, raise_on_status, stream_handle
from .ops import _i64c
from .optim import MultiAdam, ebgcn_adam


class EBGCNTrainStep:
    """``EBGCNTrainStep(model, optimizer=None, args=None)``: ``args`` (default ``model.args``) gives
    ``edge_loss_td`` / ``edge_loss_bu`` and, when no ``optimizer`` (a :class:`MultiAdam`) is given,
    the fields of :func:`ebgcn_adam`.  DropEdge is the caller's (``bigcn_amd.drop_edges`` first)."""

    def __init__(self, model, optimizer: MultiAdam = None, args=None):
        self.model = model
        self.args = model.args if args is None else args
        self.optimizer = ebgcn_adam(model, self.args) if optimizer is None else optimizer
        self.edge_loss_td = float(getattr(self.args, "edge_loss_td", 0.0))
        self.edge_loss_bu = float(getattr(self.args, "edge_loss_bu", 0.0))
        self.last_skipped = 0
        self._st = None

    def _state(self, dev):
        st = self._st
        if st is None or st["dev"] != dev:
            words = torch.zeros(4, dtype=torch.int32, device=dev)   # status, seen, skip_count
            st = {"dev": dev, "words": words, "status": words[0:1], "seen": words[1:2], "skip_count": words[2:3],
                  "skip_flag": torch.zeros(1, dtype=torch.float32, device=dev),
                  # d loss / d edge loss: the weights as device scalars, made once
                  "w_td": torch.full((), self.edge_loss_td, dtype=torch.float32, device=dev),
                  "w_bu": torch.full((), self.edge_loss_bu, dtype=torch.float32, device=dev)}
            self._st = st
        return st

    @property
    def step_count(self) -> int:
        return self.optimizer.step_count

    def step(self, data, noise=None, generator=None, pred: bool = False):
        """One iteration of ``EBGCN.py:300-312``; returns ``(loss, correct)`` (0-dim fp32 / int32 device
        tensors), plus ``pred`` ([B] int64) when ``pred=True``.  ``noise`` / ``generator``: as in
        :meth:`EBGCN.train_forward`.  No host sync: an invalid batch skips the update on the device
        (``step_count`` still advances); :meth:`check_status` tells."""
        dev = data.x.device
        if not data.x.is_cuda:
            raise _lib.BGCNError("bigcn_amd ops take device tensors (no CPU path)")
        st = self._state(dev)
        y = _i64c(data.y)
        B = int(y.numel())
        if B < 1 or data.rootindex.numel() != B:
            raise ValueError("rootindex and y must have one entry per tree, and there must be a tree")
        if getattr(data, "num_graphs", None) is None:   # (max(batch) + 1 would be a device read)
            data = types.SimpleNamespace(x=data.x, edge_index=data.edge_index, BU_edge_index=data.BU_edge_index,
                                         batch=data.batch, rootindex=data.rootindex, num_graphs=B)
        status = st["status"]
        status.zero_()
        logp, td_loss, bu_loss = self.model._train_body(data, noise, generator, status, graph_status=status)
        logp = logp if logp.is_contiguous() else logp.contiguous()
        C = int(logp.size(1))
        loss = torch.empty((), dtype=torch.float32, device=dev)
        correct = torch.empty((), dtype=torch.int32, device=dev)
        pr = torch.empty(B, dtype=torch.int64, device=dev) if pred else None
        dlogp = torch.empty_like(logp)
        check(_lib.lib().bgcn_ebgcn_train_loss(
            logp.data_ptr(), y.data_ptr(), B, C, ptr(td_loss), ptr(bu_loss), self.edge_loss_td, self.edge_loss_bu,
            loss.data_ptr(), correct.data_ptr(), ptr(pr), dlogp.data_ptr(), status.data_ptr(),
            st["skip_flag"].data_ptr(), st["seen"].data_ptr(), stream_handle()))
        roots, seeds = [logp], [dlogp]
        if td_loss is not None:
            roots.append(td_loss)
            seeds.append(st["w_td"])
        if bu_loss is not None:
            roots.append(bu_loss)
            seeds.append(st["w_bu"])
        self.optimizer.zero_grad()
        torch.autograd.backward(roots, seeds)
        self.optimizer.step(skip_flag=st["skip_flag"], skip_count=st["skip_count"])
        return (loss, correct, pr) if pred else (loss, correct)

    def check_status(self) -> int:
        """One host read: the number of updates skipped since the last check (also in
        ``last_skipped``), after raising the ``IndexError`` of :meth:`EBGCN.check_status` when a batch
        stepped on since then held an edge, root or tree index out of range, or a label outside
        ``[0, num_class)``."""
        st = self._st
        if st is None:
            self.last_skipped = 0
            return 0
        _, seen, skipped, _ = st["words"].tolist()
        st["words"][1:3].zero_()
        self.last_skipped = int(skipped)
        raise_on_status(seen, suffix=f" ({skipped} updates skipped)")
        return self.last_skipped
