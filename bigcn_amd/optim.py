"""Fused Adam for the BiGCN training loop (one HIP launch per step).

Mirrors ``torch.optim.Adam([{base}, {BU conv1, lr/5}, {BU conv2, lr/5}], lr=5e-4,
weight_decay=1e-4)`` of ``model/Twitter/BiGCN_Twitter.py:146-153`` (step at ``:189``):
same update rule (amsgrad off, weight decay as L2 in the gradient), same parameter
groups and learning rates, kernel ``bgcn_adam_step`` in ``csrc/bgcn_optim.hip``.
"""
from __future__ import annotations

import ctypes
import math
from typing import Iterable, List, Optional, Sequence

import torch

from . import _lib
from ._lib import check, ptr, stream_handle

MAX_TENSORS = 16


class _AdamTensor(ctypes.Structure):
    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p),
                ("exp_avg_sq", ctypes.c_void_p), ("numel", ctypes.c_int64), ("lr", ctypes.c_float)]


class AdamArgs(ctypes.Structure):
    _fields_ = [("t", _AdamTensor * MAX_TENSORS), ("block_start", ctypes.c_int64 * MAX_TENSORS),
                ("count", ctypes.c_int), ("beta1", ctypes.c_float), ("beta2", ctypes.c_float),
                ("eps", ctypes.c_float), ("weight_decay", ctypes.c_float),
                ("bias_correction1", ctypes.c_float), ("bias_correction2_sqrt", ctypes.c_float),
                ("grad_scale", ctypes.c_float), ("skip_flag", ctypes.c_void_p),
                ("images", ctypes.c_void_p), ("images_in_feats", ctypes.c_int64),
                ("image_role", ctypes.c_int32 * MAX_TENSORS), ("skip_count", ctypes.c_void_p)]

# BGCN_IMAGE_* (include/bgcn.h): which weight image a conv weight's update also writes
IMAGE_TD_W1, IMAGE_BU_W1, IMAGE_TD_W2, IMAGE_BU_W2 = 1, 2, 3, 4


class _AdamBase:
    """What :class:`FusedAdam` and :class:`MultiAdam` share on the host: the parameter groups (torch
    layout), the moments, the gradients of a step and the arguments both kernels take."""

    def __init__(self, param_groups: Sequence[dict], lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0):
        self.param_groups = [{"params": list(g["params"]), "lr": g.get("lr", lr)} for g in param_groups]
        self.betas, self.eps, self.weight_decay = betas, eps, weight_decay
        self.step_count = 0
        self.state = {}
        self._cache = None
        self._keep = []
        self._check_limits()
        self._pointer_key(self.params())

    def params(self) -> List[torch.nn.Parameter]:
        return [p for g in self.param_groups for p in g["params"]]

    def zero_grad(self, set_to_none: bool = True) -> None:
        for p in self.params():
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    def _check_param(self, p) -> None:
        if p.dtype != torch.float32 or not p.is_contiguous():
            raise ValueError(f"{type(self).__name__}: contiguous fp32 parameters only")

    def _pointer_key(self, ps):
        """Every pointer a cached table captures, so that reassigning ``p.data``, swapping a parameter
        in ``param_groups`` or replacing a moment rebuilds it; a parameter without moments (one
        added to ``param_groups`` after construction) gets them here."""
        for p in ps:
            if p not in self.state:
                self._check_param(p)
                self.state[p] = (torch.zeros_like(p), torch.zeros_like(p))
        return (tuple((p.data_ptr(), p.numel(), self.state[p][0].data_ptr(), self.state[p][1].data_ptr())
                      for p in ps),
                tuple(len(g["params"]) for g in self.param_groups))

    def _gradients(self, ps, grads):
        """One gradient or ``None`` per parameter: ``grads``, else ``p.grad``.  A gradient that is
        not contiguous is replaced by a contiguous copy, kept alive through the launch."""
        gs = list(grads) if grads is not None else [p.grad for p in ps]
        if len(gs) != len(ps):
            raise ValueError("grads must have one entry per parameter")
        self._keep = []
        for k, (p, gr) in enumerate(zip(ps, gs)):
            if gr is None:
                continue
            if gr.dtype != torch.float32 or gr.numel() != p.numel():
                raise ValueError(f"{type(self).__name__}: a gradient must be fp32 and of its parameter's size")
            if not gr.is_contiguous():
                gs[k] = gr.contiguous()
                self._keep.append(gs[k])
        return gs

    def _fill_step(self, a, device, grad_scale, skip_flag, skip_count) -> None:
        """The fields of the next step (step count + 1) that both argument structs have."""
        if skip_flag is not None and (skip_flag.dtype != torch.float32 or skip_flag.numel() != 1
                                      or skip_flag.device != device):
            raise ValueError("skip_flag must be a one-element fp32 tensor on the parameters' device")
        if skip_count is not None and (skip_count.dtype != torch.int32 or skip_count.numel() != 1):
            raise ValueError("skip_count must be a one-element int32 tensor")
        a.skip_flag, a.skip_count = ptr(skip_flag), ptr(skip_count)
        t = self.step_count + 1
        b1, b2 = self.betas
        a.beta1, a.beta2, a.eps, a.weight_decay = b1, b2, self.eps, self.weight_decay
        a.bias_correction1 = 1.0 - b1 ** t
        a.bias_correction2_sqrt = math.sqrt(1.0 - b2 ** t)
        a.grad_scale = grad_scale


class FusedAdam(_AdamBase):
    """``param_groups``: list of dicts {"params": [...], "lr": float} (torch layout)."""

    def _check_limits(self) -> None:
        if sum(len(g["params"]) for g in self.param_groups) > MAX_TENSORS:
            raise ValueError(f"FusedAdam handles at most {MAX_TENSORS} tensors")

    def step(self, grads: Optional[Sequence[torch.Tensor]] = None, grad_scale: float = 1.0,
             skip_flag: Optional[torch.Tensor] = None, images=None,
             skip_count: Optional[torch.Tensor] = None) -> None:
        a = self.prepare(grads, grad_scale, skip_flag, images, skip_count)
        self.step_count += 1
        if a is not None:
            check(_lib.lib().bgcn_adam_step(ctypes.addressof(a), stream_handle()))

    def prepare(self, grads: Optional[Sequence[torch.Tensor]] = None, grad_scale: float = 1.0,
                skip_flag: Optional[torch.Tensor] = None, images=None,
                skip_count: Optional[torch.Tensor] = None):
        """The ``bgcn_adam_args`` of the next :meth:`step` (step count + 1) without launching it
        - for a caller that hands them to the training step (``bgcn_step_args.adam``, which
        performs the update inside the step) and then advances ``step_count`` itself; None when
        no parameter has a gradient.

        ``grads`` overrides ``p.grad`` (e.g. views of a reduced flat DP bucket).
        ``skip_flag``: a one-element fp32 device tensor; when it holds a non-zero value at
        execution time the launch updates nothing (an invalid training step, decided on
        the device without a host sync; the step counter still advances).
        ``skip_count``: a one-element int32 device tensor incremented on the device by
        every skipped update (the number of invalid steps of a run, read once).
        ``images``: ``(buffer, in_feats, {id(param): IMAGE_*})`` - the updates of those
        conv weights also write the weight images a :class:`FusedTrainStep` reads
        (``bgcn_weight_images_size``), so its next step derives nothing from the weights.

        Learning rates are read from ``param_groups`` on every call, so schedulers that
        edit ``group['lr']`` (as with torch.optim.Adam) take effect."""
        ps = self.params()
        self._check_limits()
        gs = self._gradients(ps, grads)
        # the tensor table (parameter / moment pointers, sizes, groups) holds the parameters
        # with a gradient only and is built once per set of present gradients and pointer key;
        # only the gradient pointers are written per step (autograd hands out fresh gradient
        # tensors every step)
        key = (tuple(g is None for g in gs),) + self._pointer_key(ps)
        if self._cache is None or self._cache[0] != key:
            a = AdamArgs()
            groups = []         # param_groups index of each table entry (lr refreshed per step)
            entries = []        # params() index of each table entry
            for gi, p in enumerate(ps):
                if gs[gi] is None:
                    continue
                m, v = self.state[p]
                e = a.t[len(entries)]
                e.param, e.exp_avg, e.exp_avg_sq = ptr(p), ptr(m), ptr(v)
                e.numel = p.numel()
                groups.append(self._group_of(p))
                entries.append(gi)
            a.count = len(entries)
            self._cache = (key, a, [a.t[k] for k in range(a.count)], groups, entries)   # entry proxies
        _, a, ents, groups, entries = self._cache
        if a.count == 0:
            return None
        for e, gi, gj in zip(ents, entries, groups):
            e.grad = gs[gi].data_ptr()
            e.lr = float(self.param_groups[gj]["lr"])
        self._fill_step(a, ps[0].device, grad_scale, skip_flag, skip_count)
        if images is not None:
            buf, F, roles = images
            a.images, a.images_in_feats = ptr(buf), int(F)
            for k, gi in enumerate(entries):
                a.image_role[k] = roles.get(id(ps[gi]), 0)
        else:
            a.images, a.images_in_feats = None, 0
        return a

    def _group_of(self, p) -> int:
        for gi, g in enumerate(self.param_groups):
            if any(q is p for q in g["params"]):
                return gi
        raise KeyError("parameter not managed by this optimiser")


MULTI_MAX_TENSORS = _lib.BGCN_ADAM_MULTI_MAX_TENSORS
MULTI_MAX_GROUPS = _lib.BGCN_ADAM_MULTI_MAX_GROUPS


class MultiAdam(_AdamBase):
    """:class:`FusedAdam`'s interface for up to 128 tensors in up to 8 parameter groups, one launch
    per step (``bgcn_adam_multi_step``, ``csrc/bgcn_adam_multi.hip``); the update has
    ``FusedAdam``'s bits.  ``param_groups``: list of dicts {"params": [...], "lr": float} (torch
    layout).

    The table of parameter / moment pointers, sizes and groups is planned on the host
    (``bgcn_adam_multi_plan``) and uploaded once, and again only when a parameter's or a moment's
    storage changes; the gradient pointers and the groups' learning rates travel in the kernel
    arguments, so a step copies nothing to the device.  A parameter whose gradient is ``None``
    is left alone (no weight decay either), as by ``torch.optim.Adam``."""

    def _check_limits(self) -> None:
        if len(self.param_groups) > MULTI_MAX_GROUPS:
            raise ValueError(f"MultiAdam handles at most {MULTI_MAX_GROUPS} parameter groups")
        if sum(len(g["params"]) for g in self.param_groups) > MULTI_MAX_TENSORS:
            raise ValueError(f"MultiAdam handles at most {MULTI_MAX_TENSORS} tensors")

    def _table(self, ps):
        """``(key, args, device table)``, rebuilt when a parameter, a moment or the grouping changed."""
        key = self._pointer_key(ps)
        if self._cache is not None and self._cache[0] == key:
            return self._cache
        self._check_limits()
        n = len(ps)
        L = _lib.load_library()
        nbytes = int(L.bgcn_adam_multi_table_size(n))
        entries = (_lib.AdamMultiTensor * n)()
        k = 0
        for gi, g in enumerate(self.param_groups):
            for p in g["params"]:
                self._check_param(p)
                m, v = self.state[p]
                e = entries[k]
                e.param, e.exp_avg, e.exp_avg_sq = ptr(p), ptr(m), ptr(v)
                e.numel, e.group = p.numel(), gi
                k += 1
        host = torch.empty(nbytes, dtype=torch.uint8)
        blocks = ctypes.c_int64()
        check(L.bgcn_adam_multi_plan(ctypes.addressof(entries), n, host.data_ptr(), nbytes, ctypes.byref(blocks)))
        table = host.to(ps[0].device)   # the one upload
        a = _lib.AdamMultiArgs()
        a.table, a.count, a.blocks = table.data_ptr(), n, blocks.value
        self._cache = (key, a, table)
        return self._cache

    def step(self, grads: Optional[Sequence[Optional[torch.Tensor]]] = None, grad_scale: float = 1.0,
             skip_flag: Optional[torch.Tensor] = None, skip_count: Optional[torch.Tensor] = None) -> None:
        """``grads`` overrides ``p.grad`` (one entry per parameter in ``params()`` order, ``None``
        allowed); ``skip_flag`` / ``skip_count`` as in :meth:`FusedAdam.prepare`.  Learning rates
        are read from ``param_groups`` on every call."""
        ps = self.params()
        if not ps:
            self.step_count += 1
            return
        gs = self._gradients(ps, grads)
        _, a, _ = self._table(ps)
        for k, gr in enumerate(gs):
            a.grad[k] = None if gr is None else gr.data_ptr()
        for gi, g in enumerate(self.param_groups):
            a.lr[gi] = float(g["lr"])
        self._fill_step(a, ps[0].device, grad_scale, skip_flag, skip_count)
        self.step_count += 1
        check(_lib.lib().bgcn_adam_multi_step(ctypes.addressof(a), stream_handle()))


def ebgcn_adam(model, args) -> MultiAdam:
    """The reference's EBGCN optimiser (``EBGCN.py:249-260``) on :class:`MultiAdam`: five groups in
    the reference's order - base (``args.lr``), BU conv1 and BU conv2 (``args.lr /
    args.lr_scale_bu``), TD conv1 and TD conv2 (``args.lr / args.lr_scale_td``) - with
    ``weight_decay = args.l2`` on all of them."""
    td, bu = model.TDrumorGCN, model.BUrumorGCN
    convs = (bu.conv1, bu.conv2, td.conv1, td.conv2)
    ids = {id(p) for c in convs for p in c.parameters()}
    lr = float(args.lr)
    lr_bu, lr_td = lr / args.lr_scale_bu, lr / args.lr_scale_td
    return MultiAdam([
        {"params": [p for p in model.parameters() if id(p) not in ids]},
        {"params": list(bu.conv1.parameters()), "lr": lr_bu},
        {"params": list(bu.conv2.parameters()), "lr": lr_bu},
        {"params": list(td.conv1.parameters()), "lr": lr_td},
        {"params": list(td.conv2.parameters()), "lr": lr_td},
    ], lr=lr, weight_decay=float(args.l2))


def bigcn_adam(model, lr: float = 5e-4, weight_decay: float = 1e-4) -> FusedAdam:
    """The reference's optimiser (``BiGCN_Twitter.py:146-153``) on FusedAdam."""
    bu_ids = {id(p) for p in model.BUrumorGCN.conv1.parameters()}
    bu_ids |= {id(p) for p in model.BUrumorGCN.conv2.parameters()}
    base = [p for p in model.parameters() if id(p) not in bu_ids]
    return FusedAdam([
        {"params": base},
        {"params": list(model.BUrumorGCN.conv1.parameters()), "lr": lr / 5},
        {"params": list(model.BUrumorGCN.conv2.parameters()), "lr": lr / 5},
    ], lr=lr, weight_decay=weight_decay)
