"""The LSTM baseline of the PHEME comparison (``model/Twitter/LSTM_Twitter.py``), evaluation only.

``LSTM`` is the reference's module key for key (``lstm.weight_ih_l0`` ... ``fc.bias``), so a
checkpoint's ``model_state_dict`` loads with ``strict=True``.  The reference calls ``nn.LSTM`` once
per tree inside a Python loop; here a whole batch of trees goes through one native call
(``bgcn_lstm_eval``): per layer one GEMM for both directions' input projections and one launch per
time step for every tree at once.  ``torch.nn.LSTM`` only holds the parameters; its forward is
never called.  Training (backpropagation through time, the weight gradients and Adam over the
LSTM's tensors) is not built yet: ``forward`` raises in training mode.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._lib import check, ptr, stream_handle


def max_sequence_len(rootindex, num_nodes: int) -> int:
    """The longest sequence of a batch whose tree ``b`` is the rows ``[rootindex[b], rootindex[b + 1])``
    (the last one runs to ``num_nodes``): the ``max_len`` of :meth:`LSTM.forward_batch`.  Reads
    ``rootindex`` on the host, so call it on the CPU batch before the host-to-device copy (on a device
    tensor it is a sync).  At least 1, also for starts that do not increase (the call then flags them)."""
    r = [int(v) for v in (rootindex.tolist() if torch.is_tensor(rootindex) else rootindex)]
    ends = r[1:] + [int(num_nodes)]
    return max([1] + [e - s for s, e in zip(r, ends)])


class LSTM(torch.nn.Module):
    """Drop-in for the reference's ``LSTM`` (``LSTM_Twitter.py:19-49``) in eval mode.

    ``forward(data)`` is the reference's per-tree call; :meth:`forward_batch`, :meth:`evaluate` and
    :meth:`validate` run a whole batch of trees per native call.  ``pooling`` is stored (the
    reference reads ``self.pooling`` without assigning it)."""

    def __init__(self, in_feats=768, hid_feats=768, out_feats=4, num_layers=2, device=None, pooling='max',
                 version=0):
        super().__init__()
        self.in_feats, self.hid_feats, self.out_feats, self.num_layers = in_feats, hid_feats, out_feats, num_layers
        self.lstm = torch.nn.LSTM(in_feats, hid_feats, num_layers=num_layers, batch_first=True, bidirectional=True,
                                  bias=False)
        self.fc = torch.nn.Linear(hid_feats * num_layers * 2, out_feats)
        self.device = device
        self.pooling = pooling
        self.version = version

    # ---- parameters
    def _tensors(self):
        out = []
        for kind in ("weight_ih", "weight_hh"):
            for l in range(self.num_layers):
                out += [getattr(self.lstm, f"{kind}_l{l}"), getattr(self.lstm, f"{kind}_l{l}_reverse")]
        return out + [self.fc.weight, self.fc.bias]

    def _bind(self, dev):
        """The argument struct, refilled only when a parameter was rebound, moved or (a tensor the
        kernels cannot read in place: not fp32 / contiguous / 16-byte aligned / on ``dev``) changed."""
        src = self._tensors()
        direct = [t.dtype == torch.float32 and t.is_contiguous() and t.device == dev and t.data_ptr() % 16 == 0
                  for t in src]
        key = (dev,) + tuple((t.data_ptr(), t.dtype, None if ok else t._version) for t, ok in zip(src, direct))
        st = self.__dict__.get("_state")
        if st is not None and st["key"] == key:
            return st
        held = [t.detach() if ok else t.detach().to(device=dev, dtype=torch.float32).contiguous().clone()
                for t, ok in zip(src, direct)]
        a = _lib.LstmArgs()
        L = self.num_layers
        for l in range(L):
            for d in range(2):
                a.w_ih[l][d] = held[2 * l + d].data_ptr()
                a.w_hh[l][d] = held[2 * L + 2 * l + d].data_ptr()
        a.fc_w, a.fc_b = held[4 * L].data_ptr(), held[4 * L + 1].data_ptr()
        a.in_feats, a.hid, a.num_layers, a.out_feats = self.in_feats, self.hid_feats, L, self.out_feats
        if st is None or st["status"].device != dev:
            st = {"status": torch.zeros(1, dtype=torch.int32, device=dev),
                  "seen": torch.zeros(1, dtype=torch.int32, device=dev), "ws": None, "sizes": None}
            self.__dict__["_state"] = st
        a.status = st["status"].data_ptr()
        st.update(key=key, args=a, held=held)
        return st

    def _pool(self, x):
        """[n, T, in_feats] -> [n, in_feats] over T (``LSTM_Twitter.py:37-40``), one torch reduction."""
        if self.pooling == 'max':
            return x.amax(dim=1)
        if self.pooling == 'mean':
            return x.mean(dim=1)
        raise ValueError(f"pooling must be 'max' or 'mean', not {self.pooling!r}")

    # ---- the native call
    def _run(self, x, rootindex, max_len, y=None, logp=None, want_pred=False, want_states=False):
        if not x.is_cuda:
            raise _lib.BGCNError("bigcn_amd ops take device tensors (no CPU path)")
        if x.dim() != 2 or x.size(1) != self.in_feats:
            raise ValueError(f"the sequences' rows must be [N, {self.in_feats}], got {tuple(x.shape)}")
        dev = x.device
        st = self._bind(dev)
        a = st["args"]
        if not (x.dtype == torch.float32 and x.stride(1) == 1 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0
                and x.stride(0) >= x.size(1)):
            x = x.float().contiguous()
        rootindex = rootindex.to(device=dev, dtype=torch.int64).contiguous()
        N, B, H, L, C = int(x.size(0)), int(rootindex.numel()), self.hid_feats, self.num_layers, self.out_feats
        if N < 1 or B < 1:
            raise ValueError("the batch needs at least one row and one tree")
        if y is not None:
            y = y.to(device=dev, dtype=torch.int64).contiguous()
            if y.numel() != B:
                raise ValueError("y must have one label per tree")
        if logp is None:
            logp = torch.empty(B, C, dtype=torch.float32, device=dev)
        elif logp.dtype != torch.float32 or not logp.is_contiguous() or logp.numel() != B * C or logp.device != dev:
            raise ValueError("logp must be a contiguous fp32 [B, out_feats] tensor")
        lib = _lib.lib()
        sizes = (N, B)
        if st["sizes"] != sizes:
            need = lib.bgcn_lstm_workspace_size(N, B, self.in_feats, H, L)
            if need == 0:
                raise _lib.BGCNError("bgcn_lstm_eval: unsupported shape (in_feats % 4, hid_feats % 64 in [64, 1024], "
                                     "num_layers in [1, 4])")
            if st["ws"] is None or st["ws"].numel() < need or st["ws"].device != dev:
                st["ws"] = _lib.workspace(need, dev)
            st["sizes"] = sizes
        ws = st["ws"]
        loss = torch.empty(1, dtype=torch.float32, device=dev) if y is not None else None
        correct = torch.empty(1, dtype=torch.int32, device=dev) if y is not None else None
        pred = torch.empty(B, dtype=torch.int64, device=dev) if want_pred else None
        out = torch.empty(N, 2 * H, dtype=torch.float32, device=dev) if want_states else None
        h_n = torch.empty(2 * L, B, H, dtype=torch.float32, device=dev) if want_states else None
        a.x, a.ldx, a.num_nodes = x.data_ptr(), x.stride(0), N
        a.seq_start, a.num_seqs, a.max_len = rootindex.data_ptr(), B, int(max_len)
        a.y, a.logp, a.h_n, a.out = ptr(y), logp.data_ptr(), ptr(h_n), ptr(out)
        a.loss, a.correct, a.pred = ptr(loss), ptr(correct), ptr(pred)
        check(lib.bgcn_lstm_eval(ctypes.addressof(a), ptr(ws), ws.numel(), stream_handle()))
        st["seen"].bitwise_or_(st["status"])   # the call zeroes its status word; check_status reads this one
        return {"logp": logp, "loss": loss, "correct": correct, "pred": pred, "out": out, "h_n": h_n}

    def forward(self, data):
        """The reference's per-tree call: ``data`` is one tree's rows, ``[n, in_feats]`` when
        ``version == 2``, else ``[n, T, in_feats]`` pooled over ``T``.  Returns ``[1, out_feats]`` log
        probabilities, on the kernels of :meth:`forward_batch` as a batch of one tree (no host sync)."""
        if self.training:
            raise NotImplementedError("bigcn_amd.LSTM runs in eval mode only: the training follow-up "
                                      "(backpropagation through time, the weight gradients, Adam) is not built; "
                                      "call model.eval()")
        x = data if self.version == 2 else self._pool(data)
        if x.dim() == 3 and x.size(0) == 1:
            x = x[0]
        root = torch.zeros(1, dtype=torch.int64, device=x.device)
        return self._run(x, root, max(1, int(x.size(0))))["logp"]

    def forward_batch(self, x, rootindex, max_len=None, return_states=False):
        """``logp [B, out_feats]`` of a batch of trees: tree ``b`` is the rows ``[rootindex[b],
        rootindex[b + 1])`` of ``x [N, in_feats]`` (the last one runs to ``N``), as the reference slices.

        ``max_len`` is the number of step launches and must be known on the host: ``None`` reads
        ``rootindex`` back (:func:`max_sequence_len`), this call's only host sync - the reference
        syncs there too (``rootindex.tolist()``).  A ``max_len`` below the longest tree is flagged
        (:meth:`check_status`), never silently truncated.  ``return_states=True`` returns ``(logp,
        out [N, 2 hid] of the last layer, h_n [2 num_layers, B, hid])``."""
        if max_len is None:
            max_len = max_sequence_len(rootindex, x.size(0))
        r = self._run(x, rootindex, max_len, want_states=return_states)
        return (r["logp"], r["out"], r["h_n"]) if return_states else r["logp"]

    def _batch_rows(self, data):
        if self.version == 2:
            return data.cls
        x = data.x
        return self._pool(x.reshape(x.size(0), -1, self.in_feats))

    def evaluate(self, data, logp=None, pred=False, max_len=None):
        """One batch of the reference's test loop (``LSTM_Twitter.py:146-173``) as one native call, in
        eval mode whatever ``model.training`` says: the trees' rows are ``data.cls`` when ``version ==
        2``, else ``data.x`` reshaped to ``[N, -1, in_feats]`` and pooled; labels ``data.y``.

        Returns ``(loss, correct)`` (0-dim fp32 / int32 device tensors), plus ``pred`` ([B] int64) when
        ``pred=True``.  ``max_len``: as :meth:`forward_batch` (``None`` = one host read of
        ``data.rootindex``).  Validity of the batch: :meth:`check_status`."""
        x = self._batch_rows(data)
        if max_len is None:
            max_len = max_sequence_len(data.rootindex, x.size(0))
        r = self._run(x, data.rootindex, max_len, y=data.y, logp=logp, want_pred=pred)
        out = (r["loss"].view(()), r["correct"].view(()))
        return out + (r["pred"],) if pred else out

    def validate(self, batches, metrics=None, max_len=None):
        """The reference's test loop without a per-batch sync besides ``max_len``'s: every batch goes
        through ``evaluate(batch, pred=True)`` and its loss, correct count, predictions and labels into
        ``metrics.add(...)`` (:class:`bigcn_amd.metrics.EpochMetrics`; by default a new one sized for
        ``batches``).  ``max_len``: one bound for every batch, or ``None``.  Returns the metrics."""
        from .metrics import EpochMetrics
        batches = list(batches)
        if metrics is None:
            if not batches:
                raise ValueError("validate needs at least one batch")
            metrics = EpochMetrics(int(self.out_feats), len(batches), batches[0].y.device)
        elif len(metrics) + len(batches) > metrics.max_batches:
            raise IndexError(f"metrics has room for {metrics.max_batches - len(metrics)} more batches, "
                             f"{len(batches)} given")
        for batch in batches:
            loss, correct, pred = self.evaluate(batch, pred=True, max_len=max_len)
            metrics.add(pred, batch.y, loss, correct)
        return metrics

    def check_status(self) -> None:
        """One host sync: raise ``IndexError`` when any batch evaluated since the last check held a
        ``rootindex`` that does not increase strictly or lies outside ``[0, N)``, a tree longer than the
        ``max_len`` given, or a label outside ``[0, out_feats)``."""
        st = self.__dict__.get("_state")
        if st is None:
            return
        s = int(st["seen"].item())
        st["seen"].zero_()
        if s & _lib.BGCN_STATUS_SEQUENCE:
            raise IndexError("the batch holds a rootindex that does not increase strictly or is out of range, "
                             "a tree longer than max_len, or a label outside [0, out_feats)")
