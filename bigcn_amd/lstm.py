"""The LSTM baseline of the PHEME comparison (``model/Twitter/LSTM_Twitter.py``).

``LSTM`` is the reference's module key for key (``lstm.weight_ih_l0`` ... ``fc.bias``), so a
checkpoint's ``model_state_dict`` loads with ``strict=True``.  The reference calls ``nn.LSTM`` once
per tree inside a Python loop; here a whole batch of trees goes through one native call
(``bgcn_lstm_eval``): per layer one GEMM for both directions' input projections and one launch per
time step for every tree at once.  ``torch.nn.LSTM`` only holds the parameters; its forward is
never called.

Training: :meth:`LSTM.grad_batch` is the loop body's forward, loss and backward for a whole batch
as one native call (``bgcn_lstm_train_grad``: the same forward keeping the gates and cell states,
backpropagation through time with one launch per time step, GEMMs for the weight gradients), and
:class:`LSTMTrainStep` adds the reference's Adam (:func:`bigcn_amd.lstm_adam`) with no host sync
besides ``max_len``'s.  The per-tree ``forward`` stays an evaluation call and raises in training
mode: there is no autograd path through it.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._lib import check, ptr, raise_on_status, stream_handle
from .optim import MultiAdam

# native entry point -> (the key of its workspace in the module's state, its workspace-size function)
_ENTRY = {"bgcn_lstm_eval": ("ws", "bgcn_lstm_workspace_size"),
          "bgcn_lstm_train_grad": ("tws", "bgcn_lstm_train_workspace_size")}
# what sets BGCN_STATUS_SEQUENCE besides a bad rootindex: the end of both check_status messages
_SEQUENCE_ALSO = "a tree longer than max_len, or a label outside [0, out_feats)"


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
    def names(self):
        """The ``state_dict`` names in the order of the native call's tensors (:meth:`_tensors`)."""
        return [f"lstm.{kind}_l{l}{rev}" for kind in ("weight_ih", "weight_hh") for l in range(self.num_layers)
                for rev in ("", "_reverse")] + ["fc.weight", "fc.bias"]

    def _tensors(self):
        mods = {"lstm": self.lstm, "fc": self.fc}
        return [getattr(mods[mod], attr) for mod, attr in (n.split(".") for n in self.names())]

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
                  "seen": torch.zeros(1, dtype=torch.int32, device=dev), "sizes": {}}
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

    # ---- the native calls
    def _workspace(self, st, entry, N, B, dev):
        """The workspace of ``entry`` (:data:`_ENTRY`), kept in the module's state under the entry's key:
        sized by the largest batch so far, asked for again only when ``(N, B)`` changes."""
        key, size_fn = _ENTRY[entry]
        if st["sizes"].get(key) != (N, B):
            need = getattr(_lib.lib(), size_fn)(N, B, self.in_feats, self.hid_feats, self.num_layers)
            if need == 0:
                raise _lib.BGCNError(f"{entry}: unsupported shape (in_feats % 4, hid_feats % 64 in [64, 1024], "
                                     "num_layers in [1, 4])")
            if st.get(key) is None or st[key].numel() < need or st[key].device != dev:
                st[key] = _lib.workspace(need, dev)
            st["sizes"][key] = (N, B)
        return st[key]

    def _begin(self, entry, x, rootindex, max_len, y, logp=None, want_pred=False, want_states=False):
        """What both native calls start with: the checks, ``x`` re-laid out where the kernels cannot read
        it in place, ``rootindex`` and ``y`` on the device, the outputs, and the per-call fields of the
        entry's ``LstmArgs``.  Returns ``(st, ws, r, (x, rootindex, y))``: ``r`` holds the outputs, and the
        inputs as the kernels read them stay referenced by the caller until the call is queued."""
        if not x.is_cuda:
            raise _lib.BGCNError("bigcn_amd ops take device tensors (no CPU path)")
        if x.dim() != 2 or x.size(1) != self.in_feats:
            raise ValueError(f"the sequences' rows must be [N, {self.in_feats}], got {tuple(x.shape)}")
        dev = x.device
        st = self._bind(dev)
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
        if max_len is None:
            max_len = max_sequence_len(rootindex, N)
        if logp is None:
            logp = torch.empty(B, C, dtype=torch.float32, device=dev)
        elif logp.dtype != torch.float32 or not logp.is_contiguous() or logp.numel() != B * C or logp.device != dev:
            raise ValueError("logp must be a contiguous fp32 [B, out_feats] tensor")
        ws = self._workspace(st, entry, N, B, dev)
        r = {"logp": logp,
             "loss": torch.empty(1, dtype=torch.float32, device=dev) if y is not None else None,
             "correct": torch.empty(1, dtype=torch.int32, device=dev) if y is not None else None,
             "pred": torch.empty(B, dtype=torch.int64, device=dev) if want_pred else None,
             "out": torch.empty(N, 2 * H, dtype=torch.float32, device=dev) if want_states else None,
             "h_n": torch.empty(2 * L, B, H, dtype=torch.float32, device=dev) if want_states else None}
        a = st["args"] if entry == "bgcn_lstm_eval" else self._train_args(st)
        a.x, a.ldx, a.num_nodes = x.data_ptr(), x.stride(0), N
        a.seq_start, a.num_seqs, a.max_len = rootindex.data_ptr(), B, int(max_len)
        a.y, a.logp, a.h_n, a.out = ptr(y), logp.data_ptr(), ptr(r["h_n"]), ptr(r["out"])
        a.loss, a.correct, a.pred = ptr(r["loss"]), ptr(r["correct"]), ptr(r["pred"])
        return st, ws, r, (x, rootindex, y)

    def _run(self, x, rootindex, max_len, y=None, logp=None, want_pred=False, want_states=False):
        st, ws, r, inputs = self._begin("bgcn_lstm_eval", x, rootindex, max_len, y, logp, want_pred, want_states)
        check(_lib.lib().bgcn_lstm_eval(ctypes.addressof(st["args"]), ptr(ws), ws.numel(), stream_handle()))
        st["seen"].bitwise_or_(st["status"])   # the call zeroes its status word; check_status reads this one
        return r

    def _train_args(self, st):
        """The module's ``LstmTrainArgs``, its forward half a fresh copy of the bound ``LstmArgs``."""
        ta = st.get("targs")
        if ta is None:
            ta = st["targs"] = _lib.LstmTrainArgs()
        ctypes.memmove(ctypes.addressof(ta.fwd), ctypes.addressof(st["args"]), ctypes.sizeof(_lib.LstmArgs))
        return ta.fwd

    def _train(self, x, rootindex, y, max_len, dx=False, grads=None, want_pred=False, skip_flag=None):
        """One ``bgcn_lstm_train_grad`` call.  ``grads``: fp32 contiguous buffers in :meth:`names`
        order (default: new ones)."""
        st, ws, r, inputs = self._begin("bgcn_lstm_train_grad", x, rootindex, max_len, y, want_pred=want_pred)
        x, dev, L, ta = inputs[0], x.device, self.num_layers, st["targs"]
        if grads is None:
            grads = [torch.empty(t.shape, dtype=torch.float32, device=dev) for t in st["held"]]
        if skip_flag is None:
            skip_flag = torch.empty(1, dtype=torch.float32, device=dev)
        gx = torch.empty(x.size(0), x.stride(0), dtype=torch.float32, device=dev) if dx else None
        for l in range(L):
            for d in range(2):
                ta.d_w_ih[l][d] = grads[2 * l + d].data_ptr()
                ta.d_w_hh[l][d] = grads[2 * L + 2 * l + d].data_ptr()
        ta.d_fc_w, ta.d_fc_b = grads[4 * L].data_ptr(), grads[4 * L + 1].data_ptr()
        ta.dx, ta.skip_flag = ptr(gx), skip_flag.data_ptr()
        check(_lib.lib().bgcn_lstm_train_grad(ctypes.addressof(ta), ptr(ws), ws.numel(), stream_handle()))
        st["seen"].bitwise_or_(st["status"])
        r.update(grads=grads, dx=None if gx is None else gx[:, :self.in_feats], skip_flag=skip_flag)
        return r

    def grad_batch(self, x, rootindex, y, max_len=None, dx=False):
        """Forward, mean NLL loss and backward of one batch of trees (``LSTM_Twitter.py:96-124`` up to
        ``optimizer.step()``) as one native call: ``(loss, correct, grads)``, 0-dim fp32 / int32 device
        tensors and a dict of the loss's gradients keyed by the ``state_dict`` names, plus ``"x"``
        (``[N, in_feats]``) with ``dx=True``.  New tensors on every call; ``.grad`` is not touched.
        ``max_len``: as :meth:`forward_batch` (``None`` = the call's one host read).  Validity:
        :meth:`check_status`; the gradients of a flagged batch are not to be used."""
        r = self._train(x, rootindex, y, max_len, dx=dx)
        grads = dict(zip(self.names(), r["grads"]))
        if dx:
            grads["x"] = r["dx"]
        return r["loss"].view(()), r["correct"].view(()), grads

    def forward(self, data):
        """The reference's per-tree call: ``data`` is one tree's rows, ``[n, in_feats]`` when
        ``version == 2``, else ``[n, T, in_feats]`` pooled over ``T``.  Returns ``[1, out_feats]`` log
        probabilities, on the kernels of :meth:`forward_batch` as a batch of one tree (no host sync)."""
        if self.training:
            raise NotImplementedError("bigcn_amd.LSTM.forward is the per-tree evaluation call and has no autograd "
                                      "path: for training use bigcn_amd.LSTMTrainStep(model).step(batch) (or "
                                      "LSTM.grad_batch), else call model.eval()")
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
                             + _SEQUENCE_ALSO)


def lstm_adam(model, lr: float = 5e-4, weight_decay: float = 1e-4) -> MultiAdam:
    """The reference's optimiser (``LSTM_Twitter.py``: ``Adam(model.parameters(), lr, weight_decay)``)
    as one :class:`MultiAdam` group over all ``4 num_layers + 2`` tensors: one launch per step."""
    return MultiAdam([{"params": list(model.parameters())}], lr=lr, weight_decay=weight_decay)


class LSTMTrainStep:
    """The body of the reference's training loop (``LSTM_Twitter.py:96-126``) for a whole batch,
    with no host sync besides ``max_len``'s: ``bgcn_lstm_train_grad`` (forward, loss, accuracy,
    backward into buffers this object owns), then one :class:`MultiAdam` launch.  An invalid batch
    is decided on the device: the call sets the optimiser's ``skip_flag``, the update writes nothing,
    and :meth:`check_status` reports it with one read.  ``.grad`` is left alone."""

    def __init__(self, model: LSTM, optimizer: MultiAdam = None, lr: float = 5e-4, weight_decay: float = 1e-4):
        self.model = model
        self.optimizer = lstm_adam(model, lr, weight_decay) if optimizer is None else optimizer
        self.last_skipped = 0
        self._st = None

    def _state(self, dev):
        st = self._st
        if st is None or st["dev"] != dev:
            by_name = dict(self.model.named_parameters())
            st = {"dev": dev, "skip_count": torch.zeros(1, dtype=torch.int32, device=dev),
                  "skip_flag": torch.zeros(1, dtype=torch.float32, device=dev),
                  "grads": [torch.zeros(by_name[n].shape, dtype=torch.float32, device=dev)
                            for n in self.model.names()]}
            self._st = st
        return st

    @property
    def step_count(self) -> int:
        return self.optimizer.step_count

    def grads(self):
        """The last step's gradients by ``state_dict`` name (the step's own buffers, overwritten by the next)."""
        return dict(zip(self.model.names(), self._st["grads"])) if self._st else {}

    def step(self, data, pred: bool = False, max_len=None):
        """One iteration; ``data`` as :meth:`LSTM.evaluate` takes it.  Returns ``(loss, correct)`` (0-dim
        fp32 / int32 device tensors), plus ``pred`` ([B] int64) when ``pred=True``.  An invalid batch
        skips the update on the device (``step_count`` still advances); :meth:`check_status` tells."""
        m = self.model
        x = m._batch_rows(data)
        if not x.is_cuda:
            raise _lib.BGCNError("bigcn_amd ops take device tensors (no CPU path)")
        st = self._state(x.device)
        r = m._train(x, data.rootindex, data.y, max_len, grads=st["grads"], want_pred=pred,
                     skip_flag=st["skip_flag"])
        by_id = {id(p): g for p, g in zip(m._tensors(), st["grads"])}
        self.optimizer.step(grads=[by_id.get(id(p)) for p in self.optimizer.params()], skip_flag=st["skip_flag"],
                            skip_count=st["skip_count"])
        out = (r["loss"].view(()), r["correct"].view(()))
        return out + (r["pred"],) if pred else out

    def check_status(self) -> int:
        """One host read: the number of updates skipped since the last check (also in
        ``last_skipped``), after raising the ``IndexError`` of :meth:`LSTM.check_status` when a batch
        stepped on since then was invalid."""
        mst = self.model.__dict__.get("_state")
        if self._st is None or mst is None:
            self.last_skipped = 0
            return 0
        words = torch.cat([mst["seen"], self._st["skip_count"]]).tolist()   # the one read
        mst["seen"].zero_()
        self._st["skip_count"].zero_()
        self.last_skipped = int(words[1])
        raise_on_status(1 if int(words[0]) & _lib.BGCN_STATUS_SEQUENCE else 0,
                        index_also=f" (a rootindex that does not increase strictly, {_SEQUENCE_ALSO})",
                        suffix=f" ({self.last_skipped} updates skipped)")
        return self.last_skipped
