"""The TreeBERT baseline of the PHEME comparison (``model/Twitter/BERT_Twitter.py``): evaluation,
explain and training.

``TreeBERT`` holds the reference's parameters key for key (``BERT.embeddings...``, ``BERT.encoder.
layer.{i}...``, ``BERT.pooler.dense.*``, ``fc.*``: ``BertModel``'s names and shapes), so a
checkpoint's ``model_state_dict`` loads with ``strict=True``; ``transformers`` is not imported and
nothing is downloaded.  The reference runs ``BertModel(is_decoder=True)`` on ``inputs_embeds`` once
per tree inside a Python loop; here a whole batch of trees is one native call (``bgcn_bert_eval``).

The class is a function of each tree's first row alone: ``is_decoder=True`` makes self-attention
causal, the pooler reads position 0, position 0 attends to itself only and a softmax over one key
is exactly 1.  :meth:`TreeBERT.evaluate`, :meth:`TreeBERT.validate`, :meth:`TreeBERT.forward` and
a plain :meth:`TreeBERT.forward_batch` therefore run the *root-only* form: a chain of ``[B, hidden]``
GEMMs with no q, k or score work.  The explain run needs every row (``last_hidden_state`` and the
attention probabilities): :meth:`TreeBERT.explain_batch` and ``forward_batch(..., return_hidden /
return_sums)`` run the *full* form, the causal encoder over all rows.

Training: the loss is a function of each tree's first row in training mode too (dropout is
element-wise and cannot couple rows; the gradient of a softmax over one unmasked key is exactly 0),
so :meth:`TreeBERT.grad_batch` - the loop body's forward, loss and backward (``BERT_Twitter.py:89-119``)
for a whole batch as one native call, ``bgcn_bert_train_grad`` - is a chain of ``[B, hidden]`` GEMMs
with ``BertModel``'s four dropout sites drawn from a counter-based hash of ``(drop_seed, site, tree,
column or head)``.  The query / key parameters get exact-zero gradients (zeros, not ``None``: the
reference's Adam still decays them), ``position_embeddings`` and ``token_type_embeddings`` a gradient
in row 0 only, ``word_embeddings`` none.  :class:`TreeBERTTrainStep` adds the reference's Adam
(:func:`bert_adam`: BERT-base's 200 tensors as consecutive :class:`MultiAdam` slices) with no host
sync.  The per-tree ``forward`` stays an evaluation call and raises in training mode: there is no
autograd path through it.

:class:`TweetEncoder` is the step that makes ``data.x`` and ``data.cls`` (``Process/getPHEMEgraph.py:104-118``):
a plain bidirectional ``BertModel`` over token ids, one native call (``bgcn_bert_encode``) per tree of tweets.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import torch

from . import _lib
from ._lib import check, ptr, raise_on_status, stream_handle
from .optim import MULTI_MAX_TENSORS, MultiAdam

_LAYER_FIELDS = (("q_w", "attention.self.query.weight"), ("q_b", "attention.self.query.bias"),
                 ("k_w", "attention.self.key.weight"), ("k_b", "attention.self.key.bias"),
                 ("v_w", "attention.self.value.weight"), ("v_b", "attention.self.value.bias"),
                 ("ao_w", "attention.output.dense.weight"), ("ao_b", "attention.output.dense.bias"),
                 ("ao_ln_w", "attention.output.LayerNorm.weight"), ("ao_ln_b", "attention.output.LayerNorm.bias"),
                 ("i_w", "intermediate.dense.weight"), ("i_b", "intermediate.dense.bias"),
                 ("o_w", "output.dense.weight"), ("o_b", "output.dense.bias"),
                 ("o_ln_w", "output.LayerNorm.weight"), ("o_ln_b", "output.LayerNorm.bias"))
_TOP_FIELDS = (("pos_emb", "BERT.embeddings.position_embeddings.weight"),
               ("type_emb", "BERT.embeddings.token_type_embeddings.weight"),   # row 0 is the tensor's start
               ("emb_ln_w", "BERT.embeddings.LayerNorm.weight"), ("emb_ln_b", "BERT.embeddings.LayerNorm.bias"),
               ("pooler_w", "BERT.pooler.dense.weight"), ("pooler_b", "BERT.pooler.dense.bias"),
               ("fc_w", "fc.weight"), ("fc_b", "fc.bias"))
LN_EPS = 1e-12   # BertConfig.layer_norm_eps
# grad_batch's ``gemm``: the workspace's key in TreeBERT._state, its size function, the native call
_TRAIN_GEMMS = {"tiled": ("train", "bgcn_bert_train_workspace_size", "bgcn_bert_train_grad"),
                "skinny": ("train_skinny", "bgcn_bert_train_skinny_workspace_size", "bgcn_bert_train_grad_skinny")}


def _holder(**children):
    m = torch.nn.Module()
    for name, child in children.items():
        m.add_module(name, child)
    return m


def _bert_holders(hidden, intermediate, num_layers, max_pos, vocab):
    """``BertModel``'s parameter tree as plain torch.nn holders (their forwards are never called)."""
    Lin, LN, Emb = torch.nn.Linear, torch.nn.LayerNorm, torch.nn.Embedding

    def layer():
        return _holder(
            attention=_holder(self=_holder(query=Lin(hidden, hidden), key=Lin(hidden, hidden), value=Lin(hidden, hidden)),
                              output=_holder(dense=Lin(hidden, hidden), LayerNorm=LN(hidden, eps=LN_EPS))),
            intermediate=_holder(dense=Lin(hidden, intermediate)),
            output=_holder(dense=Lin(intermediate, hidden), LayerNorm=LN(hidden, eps=LN_EPS)))

    return _holder(
        embeddings=_holder(word_embeddings=Emb(vocab, hidden), position_embeddings=Emb(max_pos, hidden),
                           token_type_embeddings=Emb(2, hidden), LayerNorm=LN(hidden, eps=LN_EPS)),
        encoder=_holder(layer=torch.nn.ModuleList([layer() for _ in range(num_layers)])),
        pooler=_holder(dense=Lin(hidden, hidden)))


def _bert_init(holders):
    """BERT's initialisation: Linear and embedding weights normal with std 0.02, biases 0."""
    with torch.no_grad():
        for m in holders.modules():
            if isinstance(m, (torch.nn.Linear, torch.nn.Embedding)):
                m.weight.normal_(mean=0.0, std=0.02)
                if getattr(m, "bias", None) is not None:
                    m.bias.zero_()


def _bind_weights(owner, names, top_fields, dev, new_args):
    """``owner._state`` with the argument struct ``new_args()`` holding the parameters ``names`` (the
    ``top_fields``, then every layer's ``_LAYER_FIELDS``), refilled only when a parameter was rebound, moved
    or (a tensor the kernels cannot read in place: not fp32 / contiguous / 16-byte aligned / on ``dev``)
    changed.  The state also holds the call's status word, the word :func:`_take_seen` reads and the
    workspaces (:func:`_grow_workspace`).  Shared by :class:`TreeBERT` and :class:`TweetEncoder`."""
    by_name = dict(owner.named_parameters())
    src = [by_name[n] for n in names]
    direct = [t.dtype == torch.float32 and t.is_contiguous() and t.device == dev and t.data_ptr() % 16 == 0
              for t in src]
    key = (dev,) + tuple((t.data_ptr(), t.dtype, None if ok else t._version) for t, ok in zip(src, direct))
    st = owner.__dict__.get("_state")
    if st is not None and st["key"] == key:
        return st
    held = [t.detach() if ok else t.detach().to(device=dev, dtype=torch.float32).contiguous().clone()
            for t, ok in zip(src, direct)]
    a = new_args()
    it = iter(held)
    for field, _ in top_fields:
        setattr(a, field, next(it).data_ptr())
    for i in range(owner.num_layers):
        for field, _ in _LAYER_FIELDS:
            setattr(a.layer[i], field, next(it).data_ptr())
    a.hidden, a.heads, a.intermediate, a.num_layers = owner.hidden, owner.heads, owner.intermediate, owner.num_layers
    a.max_pos, a.ln_eps = owner.max_pos, LN_EPS
    if st is None or st["status"].device != dev:
        st = {"status": torch.zeros(1, dtype=torch.int32, device=dev),
              "seen": torch.zeros(1, dtype=torch.int32, device=dev), "sizes": {}, "ws": {}}
        owner.__dict__["_state"] = st
    a.status = st["status"].data_ptr()
    st.update(key=key, args=a, held=held)
    return st


def _grow_workspace(st, form, shape, need, what, dev):
    """``st``'s workspace of one form of a call, asked for again (``need()`` bytes) only when ``shape``
    changes; never shrinks."""
    if st["sizes"].get(form) != shape:
        n = need()
        if n == 0:
            raise _lib.BGCNError(f"{what}: unsupported shape (hidden = 64 heads in [64, 1024], intermediate "
                                 "% 64 in [64, 4096], num_layers in [1, 24])")
        if st["ws"].get(form) is None or st["ws"][form].numel() < n or st["ws"][form].device != dev:
            st["ws"][form] = _lib.workspace(n, dev)
        st["sizes"][form] = shape
    return st["ws"][form]


def _take_seen(owner) -> int:
    """One host sync: the status bits of ``owner``'s calls since the last read, which it clears."""
    st = owner.__dict__.get("_state")
    if st is None:
        return 0
    s = int(st["seen"].item())
    st["seen"].zero_()
    return s


@dataclass
class BertExplanation:
    """What :meth:`TreeBERT.explain_batch` returns: ``prediction`` [B] and ``log_probs`` [B, C];
    ``hidden_sum`` / ``attn_sum`` [N] (per node: ``last_hidden_state`` summed over the features,
    and the attention probabilities summed over layers, heads and queries per key); per tree their
    rankings ``hidden_order`` / ``attn_order`` [N] int32 (local node indices, best first) with the
    values in that order (``hidden_sorted`` / ``attn_sorted``); ``batch`` is the batch's."""
    prediction: torch.Tensor
    log_probs: torch.Tensor
    hidden_sum: torch.Tensor
    attn_sum: torch.Tensor
    hidden_order: torch.Tensor
    hidden_sorted: torch.Tensor
    attn_order: torch.Tensor
    attn_sorted: torch.Tensor
    batch: torch.Tensor

    def to_reference_dict(self, t: int) -> dict:
        """Tree ``t``'s record as ``explain_PHEME.py:581-600`` builds it: ``bert_last_hidden_sum_top_k``
        and ``bert_attentions_top_k`` are ``[indices, values]`` in plain lists, ``prediction`` an int."""
        B = int(self.log_probs.size(0))
        if not 0 <= t < B:
            raise IndexError("tree index out of range")
        sel = (self.batch == t).nonzero().flatten()
        a, b = (int(sel[0]), int(sel[-1]) + 1) if sel.numel() else (0, 0)
        return {"bert_last_hidden_sum_top_k": [self.hidden_order[a:b].tolist(), self.hidden_sorted[a:b].tolist()],
                "bert_attentions_top_k": [self.attn_order[a:b].tolist(), self.attn_sorted[a:b].tolist()],
                "prediction": int(self.prediction[t])}


class TreeBERT(torch.nn.Module):
    """Drop-in for the reference's ``TreeBERT`` (``BERT_Twitter.py:20-42``) in eval mode; training goes
    through :meth:`grad_batch` / :class:`TreeBERTTrainStep`.

    The positional signature is the reference's, which ignores ``in_feats``, ``hid_feats`` and
    ``out_feats`` (they are stored): its encoder is BERT-base and its head ``Linear(768, 4)``.  The
    keywords give the encoder's sizes (defaults: BERT-base) and ``num_classes`` the head's width, so
    the default module has exactly the reference's ``state_dict``.  Initialisation is BERT's: normal
    with std 0.02, LayerNorm weights 1 and biases 0, every other bias 0.  ``hidden_dropout`` and
    ``attn_dropout`` (``BertConfig``'s 0.1 defaults) are used by training only and are no part of the
    ``state_dict``.

    ``forward(data)`` is the reference's per-tree call; :meth:`forward_batch`, :meth:`evaluate`,
    :meth:`validate` and :meth:`explain_batch` run a whole batch of trees per native call."""

    def __init__(self, in_feats=256 * 768, hid_feats=64, out_feats=64, device=None, pooling='max', version=0, *,
                 hidden=768, heads=12, intermediate=3072, num_layers=12, max_pos=512, vocab=30522, num_classes=4,
                 hidden_dropout=0.1, attn_dropout=0.1):
        super().__init__()
        self.in_feats, self.hid_feats, self.out_feats = in_feats, hid_feats, out_feats
        self.hidden, self.heads, self.intermediate, self.num_layers = hidden, heads, intermediate, num_layers
        self.max_pos = max_pos
        self.hidden_dropout, self.attn_dropout = float(hidden_dropout), float(attn_dropout)
        self.BERT = _bert_holders(hidden, intermediate, num_layers, max_pos, vocab)
        self.fc = torch.nn.Linear(hidden, num_classes)
        _bert_init(self.BERT)
        self.device = device
        self.pooling = pooling
        self.version = version
        # a checkpoint written by an older transformers also holds this buffer: dropped on load
        self._register_load_state_dict_pre_hook(
            lambda sd, prefix, *_: sd.pop(prefix + "BERT.embeddings.position_ids", None))
        if device is not None:
            self.to(device)

    @property
    def num_classes(self) -> int:
        return self.fc.out_features

    # ---- parameters
    def names(self):
        """The ``state_dict`` names the native call reads, in the order of its argument struct."""
        return [n for _, n in _TOP_FIELDS] + [f"BERT.encoder.layer.{i}.{n}" for i in range(self.num_layers)
                                              for _, n in _LAYER_FIELDS]

    def _bind(self, dev):
        """The argument struct (:func:`_bind_weights`), refilled only when a parameter changed."""
        st = _bind_weights(self, self.names(), _TOP_FIELDS, dev, _lib.BertArgs)
        st["args"].out_feats = self.num_classes
        return st

    # ---- bf16 weight images of the root-only chain
    @property
    def weight_images(self):
        """``"bf16"`` when the root-only calls read bf16 weight images, else ``None`` (fp32, the default)."""
        return self.__dict__.get("_weight_images")

    def use_weight_images(self, kind="bf16"):
        """Select what the root-only calls (:meth:`evaluate`, :meth:`validate`, :meth:`forward` and a plain
        :meth:`forward_batch`) read their GEMM weights from.  ``"bf16"``: images of the value, attention-
        output, intermediate, output and pooler weights rounded to bf16 (nearest even), read by the split-K
        kernel of ``bgcn_bert_eval_w16`` - half the bytes on every compute unit, and ``logp`` moves by the
        rounding of the weights (up to about 1e-2).  ``None``: the fp32 parameters, bit for bit as before.

        The images are built at the next root-only call and again whenever a source parameter was rebound,
        moved or written (``data_ptr``, device, dtype, ``_version``), so an optimiser step or a
        ``load_state_dict`` is picked up.  They are no parameter or buffer: ``state_dict()`` is unchanged.
        The full form, :meth:`grad_batch` and :class:`TreeBERTTrainStep` always read the fp32 parameters.
        Returns ``self``."""
        if kind not in (None, "bf16"):
            raise ValueError(f"weight images are 'bf16' or None, not {kind!r}")
        self.__dict__["_weight_images"] = kind
        if kind is None:
            self.__dict__.pop("_w16", None)
        return self

    def _stale_images(self):
        """Forget the images: a native optimiser step wrote the parameters behind torch's version counters."""
        self.__dict__.pop("_w16", None)

    def _image_sources(self):
        """(field of bgcn_bert_w16_args, layer or None, state_dict name) of every imaged weight."""
        out = [(f + "16", i, f"BERT.encoder.layer.{i}.{dict(_LAYER_FIELDS)[f]}")
               for i in range(self.num_layers) for f in ("v_w", "ao_w", "i_w", "o_w")]
        return out + [("pooler_w16", None, "BERT.pooler.dense.weight")]

    def _images(self, st, dev):
        """``bgcn_bert_w16_args`` with current images: one device buffer, repacked when a source changed."""
        by_name = dict(self.named_parameters())
        srcs = self._image_sources()
        key = (dev,) + tuple((by_name[n].data_ptr(), by_name[n].device, by_name[n].dtype, by_name[n]._version)
                             for _, _, n in srcs)
        im = self.__dict__.get("_w16")
        if im is not None and im["key"] == key:
            return im["args"]
        L = _lib.lib()
        held = dict(zip(self.names(), st["held"]))       # fp32, contiguous, aligned, on dev (_bind)
        sizes = [L.bgcn_w16_image_size(*held[n].shape) for _, _, n in srcs]
        if not all(sizes):
            raise _lib.BGCNError("bgcn_w16_pack: unsupported shape (hidden and intermediate multiples of 64 in [64, 4096])")
        offs, total = [], 0
        for s in sizes:
            offs.append(total)
            total += (s + 255) // 256 * 256
        buf = im["buf"] if im is not None and im["buf"].numel() == total and im["buf"].device == dev \
            else _lib.workspace(total, dev)
        wa = _lib.BertW16Args()
        stream = stream_handle()
        for (field, layer, n), off in zip(srcs, offs):
            w = held[n]
            p = buf.data_ptr() + off
            check(L.bgcn_w16_pack(w.data_ptr(), w.stride(0), w.size(0), w.size(1), p, stream))
            if layer is None:
                setattr(wa, field, p)
            else:
                getattr(wa, field)[layer] = p
        self.__dict__["_w16"] = {"key": key, "buf": buf, "args": wa}
        return wa

    def _pool(self, x):
        """[n, T, hidden] -> [n, hidden] over T (``BERT_Twitter.py:34-37``), one torch reduction."""
        if self.pooling == 'max':
            return x.amax(dim=1)
        if self.pooling == 'mean':
            return x.mean(dim=1)
        raise ValueError(f"pooling must be 'max' or 'mean', not {self.pooling!r}")

    # ---- the native call
    def _workspace(self, st, N, B, full, dev):
        """The form's workspace, asked for again only when ``(N, B)`` changes; never shrinks.  ``full``:
        True, False, or ``"w16"`` (the root-only form on weight images)."""
        def need():
            if full == "w16":
                return _lib.lib().bgcn_bert_w16_workspace_size(B, self.hidden, self.intermediate, self.num_layers)
            return _lib.lib().bgcn_bert_workspace_size(N, B, self.hidden, self.intermediate, self.num_layers, int(full))
        return _grow_workspace(st, full, (N, B), need, "bgcn_bert_eval", dev)

    def _run(self, x, rootindex, y=None, logp=None, want_pred=False, want_hidden=False, want_sums=False, hidden=None):
        if not x.is_cuda:
            raise _lib.BGCNError("bigcn_amd ops take device tensors (no CPU path)")
        if x.dim() != 2 or x.size(1) != self.hidden:
            raise ValueError(f"the sequences' rows must be [N, {self.hidden}], got {tuple(x.shape)}")
        dev = x.device
        st = self._bind(dev)
        if not (x.dtype == torch.float32 and x.stride(1) == 1 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0
                and x.stride(0) >= x.size(1)):
            x = x.float().contiguous()
        rootindex = rootindex.to(device=dev, dtype=torch.int64).contiguous()
        N, B, C = int(x.size(0)), int(rootindex.numel()), self.num_classes
        if N < 1 or B < 1:
            raise ValueError("the batch needs at least one row and one tree")
        if y is not None:
            y = y.to(device=dev, dtype=torch.int64).contiguous()
            if y.numel() != B:
                raise ValueError("y must have one label per tree")
        if logp is None:
            logp = torch.empty(B, C, dtype=torch.float32, device=dev)
        elif logp.dtype != torch.float32 or not logp.is_contiguous() or logp.numel() != B * C or logp.device != dev:
            raise ValueError("logp must be a contiguous fp32 [B, num_classes] tensor")
        if hidden is None and want_hidden:
            hidden = torch.empty(N, self.hidden, dtype=torch.float32, device=dev)
        elif hidden is not None and (hidden.dtype != torch.float32 or not hidden.is_contiguous()
                                     or hidden.numel() != N * self.hidden or hidden.device != dev):
            raise ValueError("hidden must be a contiguous fp32 [N, hidden] tensor")
        full = hidden is not None or want_sums
        w16 = not full and self.weight_images == "bf16"
        ws = self._workspace(st, N, B, "w16" if w16 else full, dev)
        r = {"logp": logp, "hidden": hidden,
             "loss": torch.empty(1, dtype=torch.float32, device=dev) if y is not None else None,
             "correct": torch.empty(1, dtype=torch.int32, device=dev) if y is not None else None,
             "pred": torch.empty(B, dtype=torch.int64, device=dev) if want_pred else None,
             # [2, N] with a row stride of whole 16-byte units: hidden_sum, attn_sum
             "sums": torch.empty(2, (N + 3) // 4 * 4, dtype=torch.float32, device=dev)[:, :N] if want_sums else None}
        a = st["args"]
        a.x, a.ldx, a.num_nodes = x.data_ptr(), x.stride(0), N
        a.seq_start, a.num_seqs = rootindex.data_ptr(), B
        a.y, a.logp, a.loss, a.correct, a.pred = ptr(y), logp.data_ptr(), ptr(r["loss"]), ptr(r["correct"]), ptr(r["pred"])
        a.hidden_out = ptr(hidden)
        a.hidden_sum = r["sums"][0].data_ptr() if want_sums else 0
        a.attn_sum = r["sums"][1].data_ptr() if want_sums else 0
        if w16:
            wa = self._images(st, dev)
            ctypes.memmove(ctypes.addressof(wa.base), ctypes.addressof(a), ctypes.sizeof(_lib.BertArgs))
            check(_lib.lib().bgcn_bert_eval_w16(ctypes.addressof(wa), ptr(ws), ws.numel(), stream_handle()))
        else:
            check(_lib.lib().bgcn_bert_eval(ctypes.addressof(a), ptr(ws), ws.numel(), stream_handle()))
        st["seen"].bitwise_or_(st["status"])   # the call zeroes its status word; check_status reads this one
        return r

    def _train(self, x, rootindex, y, dx=False, grads=None, want_pred=False, skip_flag=None, drop_seed=0,
               hidden_dropout=None, attn_dropout=None, gemm="tiled"):
        """One ``bgcn_bert_train_grad`` call (``gemm="skinny"``: ``bgcn_bert_train_grad_skinny``).  ``grads``:
        fp32 contiguous buffers in :meth:`names` order (default: new ones)."""
        if gemm not in _TRAIN_GEMMS:
            raise ValueError(f"gemm must be 'tiled' or 'skinny', not {gemm!r}")
        form, size_fn, grad_fn = _TRAIN_GEMMS[gemm]
        if not x.is_cuda:
            raise _lib.BGCNError("bigcn_amd ops take device tensors (no CPU path)")
        if x.dim() != 2 or x.size(1) != self.hidden:
            raise ValueError(f"the sequences' rows must be [N, {self.hidden}], got {tuple(x.shape)}")
        dev = x.device
        st = self._bind(dev)
        if not (x.dtype == torch.float32 and x.stride(1) == 1 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0
                and x.stride(0) >= x.size(1)):
            x = x.float().contiguous()
        rootindex = rootindex.to(device=dev, dtype=torch.int64).contiguous()
        N, B, C = int(x.size(0)), int(rootindex.numel()), self.num_classes
        if N < 1 or B < 1:
            raise ValueError("the batch needs at least one row and one tree")
        y = y.to(device=dev, dtype=torch.int64).contiguous()
        if y.numel() != B:
            raise ValueError("y must have one label per tree")
        ws = _grow_workspace(st, form, B, lambda: getattr(_lib.lib(), size_fn)(N, B, self.hidden, self.intermediate,
                                                                            self.num_layers), grad_fn, dev)
        r = {"logp": torch.empty(B, C, dtype=torch.float32, device=dev),
             "loss": torch.empty(1, dtype=torch.float32, device=dev),
             "correct": torch.empty(1, dtype=torch.int32, device=dev),
             "pred": torch.empty(B, dtype=torch.int64, device=dev) if want_pred else None}
        ta = st.get("targs")
        if ta is None:
            ta = st["targs"] = _lib.BertTrainArgs()
        ctypes.memmove(ctypes.addressof(ta.fwd), ctypes.addressof(st["args"]), ctypes.sizeof(_lib.BertArgs))
        a = ta.fwd
        a.x, a.ldx, a.num_nodes = x.data_ptr(), x.stride(0), N
        a.seq_start, a.num_seqs = rootindex.data_ptr(), B
        a.y, a.logp, a.loss, a.correct, a.pred = y.data_ptr(), r["logp"].data_ptr(), r["loss"].data_ptr(), \
            r["correct"].data_ptr(), ptr(r["pred"])
        a.hidden_out = a.hidden_sum = a.attn_sum = None
        if grads is None:
            by_name = dict(self.named_parameters())
            grads = [torch.empty(by_name[n].shape, dtype=torch.float32, device=dev) for n in self.names()]
        if skip_flag is None:
            skip_flag = torch.empty(1, dtype=torch.float32, device=dev)
        gx = torch.empty(N, x.stride(0), dtype=torch.float32, device=dev) if dx else None
        it = iter(grads)
        for field, _ in _TOP_FIELDS:
            setattr(ta, "d_" + field, next(it).data_ptr())
        for i in range(self.num_layers):
            for field, _ in _LAYER_FIELDS:
                setattr(ta.d_layer[i], field, next(it).data_ptr())
        ta.dx, ta.skip_flag, ta.drop_seed = ptr(gx), skip_flag.data_ptr(), int(drop_seed) & (2 ** 64 - 1)
        ta.hidden_dropout = self.hidden_dropout if hidden_dropout is None else float(hidden_dropout)
        ta.attn_dropout = self.attn_dropout if attn_dropout is None else float(attn_dropout)
        check(getattr(_lib.lib(), grad_fn)(ctypes.addressof(ta), ptr(ws), ws.numel(), stream_handle()))
        st["seen"].bitwise_or_(st["status"])
        r.update(grads=grads, dx=None if gx is None else gx[:, :self.hidden], skip_flag=skip_flag)
        return r

    def grad_batch(self, x, rootindex, y, dx=False, drop_seed=0, hidden_dropout=None, attn_dropout=None,
                   gemm="tiled"):
        """Forward in training mode, mean NLL loss and backward of one batch of trees
        (``BERT_Twitter.py:89-119`` up to ``optimizer.step()``) as one native call: ``(loss, correct,
        grads)``, 0-dim fp32 / int32 device tensors and a dict of the loss's gradients keyed by the
        ``state_dict`` names - every name of :meth:`names` (zeros for the query / key tensors and for
        the rows past the first of both embeddings), no ``word_embeddings`` entry - plus ``"x"`` (``[N,
        hidden]``: the root rows' gradient, zeros elsewhere) with ``dx=True``.  Only the trees' first
        rows of ``x`` are read.  The dropout masks are a function of ``drop_seed``; the rates default
        to the module's.  New tensors on every call; ``.grad`` is not touched; no host sync.  Validity:
        :meth:`check_status`; the gradients of a flagged batch are not to be used.

        ``gemm`` selects the kernels of the chain's products: ``"tiled"`` (the default) the block-tiled
        GEMMs, whose forward has :meth:`evaluate`'s bits; ``"skinny"`` the split kernels of
        ``bgcn_bert_train_grad_skinny``, which put each ``[B, hidden]`` product on 256 or more workgroups
        and read the fp32 parameters as they are.  Same masks, same contract; the results agree within
        fp32 rounding, not bit for bit.  Any other string raises ``ValueError``."""
        r = self._train(x, rootindex, y, dx=dx, drop_seed=drop_seed, hidden_dropout=hidden_dropout,
                        attn_dropout=attn_dropout, gemm=gemm)
        grads = dict(zip(self.names(), r["grads"]))
        if dx:
            grads["x"] = r["dx"]
        return r["loss"].view(()), r["correct"].view(()), grads

    def forward(self, data):
        """The reference's per-tree call, on the root-only form (no host sync).  ``version != 2``:
        ``data [n, T, hidden]`` is pooled over ``T`` and run as one sequence of ``n`` rows, giving
        ``[1, num_classes]`` log probabilities.  ``version == 2``: ``data [n, T, hidden]`` is ``n``
        sequences of ``T`` tokens, giving ``[n, num_classes]``."""
        if self.training:
            raise NotImplementedError("bigcn_amd.TreeBERT.forward is the per-tree evaluation call and has no autograd "
                                      "path: for training use bigcn_amd.TreeBERTTrainStep(model).step(batch) (or "
                                      "TreeBERT.grad_batch), else call model.eval()")
        if data.dim() != 3:
            raise ValueError(f"data must be [n, T, {self.hidden}], got {tuple(data.shape)}")
        if self.version == 2:
            n, T = int(data.size(0)), int(data.size(1))
            root = torch.arange(n, dtype=torch.int64, device=data.device) * T
            return self._run(data.reshape(n * T, -1), root)["logp"]
        root = torch.zeros(1, dtype=torch.int64, device=data.device)
        return self._run(self._pool(data), root)["logp"]

    def forward_batch(self, x, rootindex, return_hidden=False, return_sums=False):
        """``logp [B, num_classes]`` of a batch of trees: tree ``b`` is the rows ``[rootindex[b],
        rootindex[b + 1])`` of ``x [N, hidden]`` (the last one runs to ``N``), as the reference slices.
        No host sync; a tree longer than ``max_pos`` is flagged (:meth:`check_status`), never truncated.

        Alone this is the root-only form and reads the trees' first rows only.  ``return_hidden=True``
        also returns ``last_hidden_state [N, hidden]``, ``return_sums=True`` also ``(hidden_sum [N],
        attn_sum [N])``; either runs the full causal encoder, and ``logp`` then comes from its own
        root rows."""
        r = self._run(x, rootindex, want_hidden=return_hidden, want_sums=return_sums)
        out = (r["logp"],)
        if return_hidden:
            out += (r["hidden"],)
        if return_sums:
            out += ((r["sums"][0], r["sums"][1]),)
        return out if len(out) > 1 else out[0]

    def _root_rows(self, data):
        """``[N, hidden]`` holding the pooled row of every tree's root; the other rows are left
        unwritten, as the root-only form never reads them.  Only ``B`` of the ``N`` rows of ``data.x``
        are pooled (the indices are clamped for this gather; the native call flags a bad one)."""
        x = data.x
        N = int(x.size(0))
        roots = data.rootindex.to(device=x.device, dtype=torch.int64).clamp(0, max(N - 1, 0))
        pooled = self._pool(x.index_select(0, roots).reshape(roots.numel(), -1, self.hidden).float())
        rows = torch.empty(N, self.hidden, dtype=torch.float32, device=x.device)
        rows[roots] = pooled
        return rows

    def evaluate(self, data, logp=None, pred=False):
        """One batch of the reference's test loop (``BERT_Twitter.py:127-150``) as one native call on the
        root-only form, in eval mode whatever ``model.training`` says: ``data.x`` is reshaped to ``[N,
        -1, hidden]`` and pooled over the middle axis - only the ``B`` root rows are pooled, the class
        does not depend on any other; labels ``data.y``.

        Returns ``(loss, correct)`` (0-dim fp32 / int32 device tensors), plus ``pred`` ([B] int64) when
        ``pred=True``.  No host sync.  Validity of the batch: :meth:`check_status`."""
        if self.version == 2:
            raise NotImplementedError("TreeBERT.evaluate with version == 2: the reference's loop body assigns the "
                                      "[n, 4] result of an n-node tree into one row of out_labels "
                                      "(BERT_Twitter.py:103-105), which fails for any tree of more than one node")
        r = self._run(self._root_rows(data), data.rootindex, y=data.y, logp=logp, want_pred=pred)
        out = (r["loss"].view(()), r["correct"].view(()))
        return out + (r["pred"],) if pred else out

    def validate(self, batches, metrics=None):
        """The reference's test loop without a host sync: every batch goes through ``evaluate(batch,
        pred=True)`` and its loss, correct count, predictions and labels into ``metrics.add(...)``
        (:class:`bigcn_amd.metrics.EpochMetrics`; by default a new one sized for ``batches``)."""
        from .metrics import EpochMetrics
        batches = list(batches)
        if metrics is None:
            if not batches:
                raise ValueError("validate needs at least one batch")
            metrics = EpochMetrics(int(self.num_classes), len(batches), batches[0].y.device)
        elif len(metrics) + len(batches) > metrics.max_batches:
            raise IndexError(f"metrics has room for {metrics.max_batches - len(metrics)} more batches, "
                             f"{len(batches)} given")
        for batch in batches:
            loss, correct, pred = self.evaluate(batch, pred=True)
            metrics.add(pred, batch.y, loss, correct)
        return metrics

    def explain_batch(self, data) -> BertExplanation:
        """The BERT branch of the explain run (``explain_PHEME.py:581-600``) for a whole batch: one
        full-form call on all rows of ``data.x`` (reshaped to ``[N, -1, hidden]`` and pooled), then
        ``bgcn_segment_rank`` on ``hidden_sum`` and ``attn_sum`` - per-tree ``topk`` with ``k = n``,
        ties by ascending node index.  ``data.batch`` is the PyG batch vector.  One host sync at the
        end (the status words)."""
        from .ops import _segment_rank
        if self.training:
            raise ValueError("explain needs the model in eval mode (call model.eval())")
        with torch.no_grad():
            x = data.x
            rows = self._pool(x.reshape(x.size(0), -1, self.hidden).float())
            r = self._run(rows, data.rootindex, want_pred=True, want_sums=True)
            status = torch.zeros(1, dtype=torch.int32, device=x.device)
            order, srt = _segment_rank(r["sums"], data.batch, int(data.rootindex.numel()), status)
            self.check_status()
            if int(status.item()) & 1:
                raise IndexError("the batch vector decreases or holds an id outside [0, B)")
        return BertExplanation(r["pred"], r["logp"], r["sums"][0], r["sums"][1], order[0], srt[0], order[1], srt[1],
                               data.batch)

    def check_status(self) -> None:
        """One host sync: raise ``IndexError`` when any batch evaluated since the last check held a
        ``rootindex`` that does not increase strictly or lies outside ``[0, N)``, a tree longer than
        ``max_pos``, or a label outside ``[0, num_classes)``."""
        if _take_seen(self) & _lib.BGCN_STATUS_SEQUENCE:
            raise IndexError("the batch holds a rootindex that does not increase strictly or is out of range, "
                             "a tree longer than max_pos, or a label outside [0, num_classes)")


class ChunkedAdam:
    """What :func:`bert_adam` returns: :class:`MultiAdam`'s step over more tensors than one
    ``MultiAdam`` takes, as ``ceil(n / 128)`` of them over consecutive slices of the parameter list,
    one launch each.  Only the first slice is given ``skip_count``, so a skipped step counts once."""

    def __init__(self, params, lr: float, weight_decay: float, after_step=None):
        params = list(params)
        self.after_step = after_step   # called after every step: the launches write the parameters in place
        self.chunks = [MultiAdam([{"params": params[i:i + MULTI_MAX_TENSORS]}], lr=lr, weight_decay=weight_decay)
                       for i in range(0, len(params), MULTI_MAX_TENSORS)]

    def params(self):
        return [p for c in self.chunks for p in c.params()]

    @property
    def step_count(self) -> int:
        return self.chunks[0].step_count if self.chunks else 0

    def step(self, grads=None, skip_flag=None, skip_count=None) -> None:
        """``grads``: one entry per parameter in :meth:`params` order (``None`` allowed: that parameter is
        left alone), default ``p.grad``; ``skip_flag`` / ``skip_count`` as :meth:`MultiAdam.step`."""
        if grads is not None and len(grads) != len(self.params()):
            raise ValueError("grads must have one entry per parameter")
        k = 0
        for i, c in enumerate(self.chunks):
            n = len(c.params())
            c.step(grads=None if grads is None else grads[k:k + n], skip_flag=skip_flag,
                   skip_count=skip_count if i == 0 else None)
            k += n
        if self.after_step is not None:
            self.after_step()

    def state_dict(self) -> dict:
        """``step_count`` and, in :meth:`params` order, copies of both moments."""
        ps = self.params()
        state = {p: c.state[p] for c in self.chunks for p in c.params()}
        return {"step_count": self.step_count, "exp_avg": [state[p][0].clone() for p in ps],
                "exp_avg_sq": [state[p][1].clone() for p in ps]}

    def load_state_dict(self, sd: dict) -> None:
        ps = self.params()
        if len(sd["exp_avg"]) != len(ps) or len(sd["exp_avg_sq"]) != len(ps):
            raise ValueError("the state holds another number of tensors")
        state = {p: c.state[p] for c in self.chunks for p in c.params()}
        with torch.no_grad():
            for p, m, v in zip(ps, sd["exp_avg"], sd["exp_avg_sq"]):
                state[p][0].copy_(m)
                state[p][1].copy_(v)
        for c in self.chunks:
            c.step_count = int(sd["step_count"])


def bert_adam(model, lr: float = 5e-4, weight_decay: float = 1e-4) -> ChunkedAdam:
    """The reference's optimiser (``BERT_Twitter.py``: ``Adam(model.parameters(), lr=5e-4,
    weight_decay=1e-4)``) over all of ``model.parameters()`` in their order.  ``word_embeddings`` is
    in the list and never gets a gradient, so it is left alone, as by torch.  Its launches write the
    parameters behind torch's version counters, so every step also tells ``model`` to rebuild its weight
    images (:meth:`TreeBERT.use_weight_images`) at the next root-only call."""
    return ChunkedAdam(model.parameters(), lr, weight_decay, after_step=model._stale_images)


class TreeBERTTrainStep:
    """The body of the reference's training loop (``BERT_Twitter.py:89-119``) for a whole batch with no
    host sync: the trees' root rows pooled, ``bgcn_bert_train_grad`` (forward with dropout, loss,
    accuracy, backward into buffers this object owns), then the Adam launches.  The k-th step draws
    its masks from ``drop_seed + k`` (``drop_seed=None``: drawn once from torch's generator); the seed
    of the last step is ``last_drop_seed``.  An invalid batch is decided on the device: the call sets
    the optimiser's ``skip_flag``, the update writes nothing, and :meth:`check_status` reports it with
    one read.  ``.grad`` is left alone.  ``gemm``: as :meth:`TreeBERT.grad_batch` takes it (``"tiled"``, the
    default, or ``"skinny"``)."""

    def __init__(self, model: TreeBERT, optimizer=None, lr: float = 5e-4, weight_decay: float = 1e-4, drop_seed=None,
                 gemm="tiled"):
        if gemm not in _TRAIN_GEMMS:
            raise ValueError(f"gemm must be 'tiled' or 'skinny', not {gemm!r}")
        self.gemm = gemm
        self.model = model
        self.optimizer = bert_adam(model, lr, weight_decay) if optimizer is None else optimizer
        self.drop_seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if drop_seed is None else int(drop_seed)
        self.last_drop_seed = None
        self.last_skipped = 0
        self._steps = 0
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

    def step(self, data, pred: bool = False):
        """One iteration; ``data`` as :meth:`TreeBERT.evaluate` takes it.  Returns ``(loss, correct)``
        (0-dim fp32 / int32 device tensors), plus ``pred`` ([B] int64) when ``pred=True``.  An invalid
        batch skips the update on the device (``step_count`` still advances); :meth:`check_status` tells."""
        m = self.model
        if m.version == 2:
            raise NotImplementedError("TreeBERTTrainStep.step with version == 2: the reference's loop body assigns "
                                      "the [n, 4] result of an n-node tree into one row of out_labels "
                                      "(BERT_Twitter.py:103-105), which fails for any tree of more than one node")
        if not data.x.is_cuda:
            raise _lib.BGCNError("bigcn_amd ops take device tensors (no CPU path)")
        st = self._state(data.x.device)
        self.last_drop_seed = (self.drop_seed + self._steps) & (2 ** 64 - 1)
        self._steps += 1
        r = m._train(m._root_rows(data), data.rootindex, data.y, grads=st["grads"], want_pred=pred,
                     skip_flag=st["skip_flag"], drop_seed=self.last_drop_seed, gemm=self.gemm)
        by_name = dict(m.named_parameters())
        by_id = {id(by_name[n]): g for n, g in zip(m.names(), st["grads"])}
        self.optimizer.step(grads=[by_id.get(id(p)) for p in self.optimizer.params()], skip_flag=st["skip_flag"],
                            skip_count=st["skip_count"])
        m._stale_images()
        out = (r["loss"].view(()), r["correct"].view(()))
        return out + (r["pred"],) if pred else out

    def check_status(self) -> int:
        """One host read: the number of updates skipped since the last check (also in
        ``last_skipped``), after raising the ``IndexError`` of :meth:`TreeBERT.check_status` when a batch
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
                        index_also=" (a rootindex that does not increase strictly, a tree longer than max_pos, or a "
                                   "label outside [0, num_classes))",
                        suffix=f" ({self.last_skipped} updates skipped)")
        return self.last_skipped


# bgcn_bert_encode_args' top-level weights: BertModel's own names (TreeBERT's without "BERT." and fc)
_ENC_TOP_FIELDS = (("word_emb", "embeddings.word_embeddings.weight"),) + tuple(
    (f, n[len("BERT."):]) for f, n in _TOP_FIELDS if n.startswith("BERT."))


class TweetEncoder(torch.nn.Module):
    """The feature extraction of the PHEME study (``Process/getPHEMEgraph.py:104-118``): a plain
    ``BertModel`` in eval mode over token ids - not a decoder and no attention mask, so every position
    of a tweet, padding included, attends to every other - as one native call (``bgcn_bert_encode``)
    per tree of tweets::

        embeddings = model.embeddings(input_ids)          # [n, T, hidden] -> x, root
        cls = model(input_ids).pooler_output              # [n, hidden]    -> cls

    The module holds ``BertModel``'s parameters under its own names (``embeddings.word_embeddings.weight``
    ... ``pooler.dense.bias``), so ``BertModel.state_dict()`` loads with ``strict=True``.  The tokenizer
    and the pretrained weights stay with the caller: ``transformers`` is not imported and nothing is
    downloaded.  Initialisation is BERT's (normal with std 0.02).  The parameters are read in place, fp32;
    there is no autograd path.

    ``pooler_output`` reads position 0 of the last layer only, so by default that layer runs on the
    ``[n, hidden]`` first rows (its keys and values on all rows): exact, like the root-only form of
    :class:`TreeBERT`.  Asking for ``last_hidden_state`` runs it on every row."""

    def __init__(self, hidden=768, heads=12, intermediate=3072, num_layers=12, max_pos=512, vocab=30522, device=None,
                 _holders=None):
        super().__init__()
        self.hidden, self.heads, self.intermediate, self.num_layers = hidden, heads, intermediate, num_layers
        self.max_pos, self.vocab = max_pos, vocab
        b = _holders
        if b is None:
            b = _bert_holders(hidden, intermediate, num_layers, max_pos, vocab)
            _bert_init(b)
        self.embeddings, self.encoder, self.pooler = b.embeddings, b.encoder, b.pooler
        # a checkpoint written by an older transformers also holds this buffer: dropped on load
        self._register_load_state_dict_pre_hook(
            lambda sd, prefix, *_: sd.pop(prefix + "embeddings.position_ids", None))
        if device is not None:
            self.to(device)

    @classmethod
    def from_treebert(cls, model: TreeBERT) -> "TweetEncoder":
        """An encoder on ``model.BERT``'s parameters: the same tensors (and holder modules), not copies, so
        a ``load_state_dict``, an optimiser step or a ``.to()`` of either is the other's too."""
        return cls(model.hidden, model.heads, model.intermediate, model.num_layers, model.max_pos,
                   model.BERT.embeddings.word_embeddings.num_embeddings, _holders=model.BERT)

    def names(self):
        """The ``state_dict`` names the native call reads, in the order of its argument struct."""
        return [n for _, n in _ENC_TOP_FIELDS] + [f"encoder.layer.{i}.{n}" for i in range(self.num_layers)
                                                  for _, n in _LAYER_FIELDS]

    def _run(self, input_ids, want_cls=True, want_hidden=False, emb=None, cls=None):
        """One ``bgcn_bert_encode`` call.  ``emb`` / ``cls``: contiguous fp32 ``[n, T, hidden]`` / ``[n, hidden]``
        tensors to write into (default: new ones); ``want_cls=False``: the embeddings alone."""
        if not isinstance(input_ids, torch.Tensor) or input_ids.dim() != 2 or input_ids.is_floating_point() \
                or input_ids.is_complex() or input_ids.dtype == torch.bool:
            raise ValueError("input_ids must be a 2-D integer tensor [n, T]")
        n, T = int(input_ids.size(0)), int(input_ids.size(1))
        if n < 1 or T < 1 or T > self.max_pos:
            raise ValueError(f"input_ids must hold at least one sequence of 1 to max_pos = {self.max_pos} tokens, "
                             f"got {tuple(input_ids.shape)}")
        if not input_ids.is_cuda:
            raise _lib.BGCNError("bigcn_amd ops take device tensors (no CPU path)")
        dev = input_ids.device
        st = _bind_weights(self, self.names(), _ENC_TOP_FIELDS, dev, _lib.BertEncodeArgs)
        ids = input_ids.to(torch.int64).contiguous()
        H = self.hidden
        if emb is None:
            emb = torch.empty(n, T, H, dtype=torch.float32, device=dev)
        if cls is None and want_cls:
            cls = torch.empty(n, H, dtype=torch.float32, device=dev)
        hid = torch.empty(n, T, H, dtype=torch.float32, device=dev) if want_hidden else None
        a = st["args"]
        a.input_ids, a.num_seqs, a.seq_len, a.vocab = ids.data_ptr(), n, T, self.vocab
        a.embeddings, a.ld_embeddings, a.cls, a.hidden_out = emb.data_ptr(), H, ptr(cls), ptr(hid)
        a.last_layer_full, a.embed_only = int(want_hidden), int(not want_cls)
        ws = None
        if want_cls:
            ws = _grow_workspace(st, "encode", (n, T), lambda: _lib.lib().bgcn_bert_encode_workspace_size(
                n, T, H, self.intermediate, self.num_layers, int(want_hidden)), "bgcn_bert_encode", dev)
        check(_lib.lib().bgcn_bert_encode(ctypes.addressof(a), ptr(ws), 0 if ws is None else ws.numel(), stream_handle()))
        st["seen"].bitwise_or_(st["status"])   # the call zeroes its status word; check_status reads this one
        return emb, cls, hid

    def encode(self, input_ids, return_hidden=False):
        """``(embeddings [n, T, hidden], cls [n, hidden])`` of the ``n`` sequences ``input_ids [n, T]``
        (integer ids on the GPU; int32 is converted): ``model.embeddings(input_ids)`` and
        ``model(input_ids).pooler_output``.  ``return_hidden=True`` also returns ``last_hidden_state
        [n, T, hidden]`` and runs the last layer on every row.  New tensors on every call, no host sync;
        a token id outside ``[0, vocab)`` is flagged (:meth:`check_status`), never read out of bounds."""
        emb, cls, hid = self._run(input_ids, want_hidden=return_hidden)
        return (emb, cls, hid) if return_hidden else (emb, cls)

    def embed(self, input_ids):
        """``model.embeddings(input_ids)`` alone, ``[n, T, hidden]``: no encoder layer runs."""
        return self._run(input_ids, want_cls=False)[0]

    def forward(self, input_ids):
        """:meth:`encode`."""
        return self.encode(input_ids)

    def features(self, input_ids, max_seqs=64, root_index=0):
        """The arrays ``getPHEMEgraph.py:116-118`` stores for one tree of ``n`` tweets, as device tensors:
        ``{"x": [n, T * hidden], "cls": [n, hidden], "root": x[root_index : root_index + 1]}``.  A tree of
        more than ``max_seqs`` tweets goes through several calls (the sequences are independent), each
        writing its rows of the one preallocated result; the workspace is that of ``max_seqs`` tweets."""
        if max_seqs < 1:
            raise ValueError("max_seqs must be at least 1")
        if not isinstance(input_ids, torch.Tensor) or input_ids.dim() != 2 or input_ids.size(0) < 1:
            raise ValueError("input_ids must be a 2-D integer tensor [n, T]")
        if not input_ids.is_cuda:
            raise _lib.BGCNError("bigcn_amd ops take device tensors (no CPU path)")
        n, T = int(input_ids.size(0)), int(input_ids.size(1))
        if not 0 <= root_index < n:
            raise IndexError("root_index out of range")
        x = torch.empty(n, T, self.hidden, dtype=torch.float32, device=input_ids.device)
        cls = torch.empty(n, self.hidden, dtype=torch.float32, device=input_ids.device)
        for i in range(0, n, max_seqs):
            self._run(input_ids[i:i + max_seqs], emb=x[i:i + max_seqs], cls=cls[i:i + max_seqs])
        x = x.view(n, T * self.hidden)
        return {"x": x, "cls": cls, "root": x[root_index:root_index + 1]}

    def check_status(self) -> None:
        """One host sync: raise ``IndexError`` when any call since the last check read a token id outside
        ``[0, vocab)``."""
        raise_on_status(_take_seen(self), bits=_lib.BGCN_STATUS_TOKEN)
