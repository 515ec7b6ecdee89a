"""The reference's evaluation metrics (``tools/evaluate.py``) from a confusion matrix counted on
the device, and a validation epoch recorded without a host sync.

The reference's test loop (``BiGCN_Twitter.py:207-233``) hands every batch's predictions and
labels to ``evaluation4class`` (``tools/evaluate.py:3-91``): a Python loop with sixteen tensor
comparisons per tree, each a host sync on device tensors, plus two ``.item()`` calls per batch.
Every number it returns is a function of how often label ``a`` met prediction ``p``, so here

* :func:`confusion` counts that ``[C, C]`` matrix (row = actual, column = predicted) in one launch
  (``bgcn_confusion``; numpy for host inputs);
* :func:`class_metrics` derives the reference's numbers from the integer counts on the host, with
  its ``round(., 4)`` at every step, its zero branches and Python float arithmetic, so the values
  agree digit for digit;
* :func:`evaluation4class` / :func:`evaluationclass` are drop-ins for the reference's two functions:
  one kernel and one read for device inputs;
* :class:`EpochMetrics` records a whole validation epoch in device buffers (``add`` does not sync)
  and turns it into what the reference logs with one device-to-host read (``result``).
  ``FusedTrainStep.validate`` is the test loop around it.

Early stopping and checkpoint files stay with the caller: the reference's ``EarlyStopping`` takes
the numbers ``result()`` returns.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_handle

__all__ = ["confusion", "class_metrics", "evaluation4class", "evaluationclass", "EpochMetrics", "EpochResult",
           "MAX_CLASSES"]

MAX_CLASSES = 16   # bgcn_confusion counts in at most 16 x 16 bins


def _is_dev(t) -> bool:
    return isinstance(t, torch.Tensor) and t.is_cuda


def _host_labels(t) -> np.ndarray:
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    a = np.asarray(t)
    if a.size and a.dtype.kind not in "iub":
        raise TypeError("labels and predictions must be integers")
    return a.astype(np.int64).reshape(-1)


def _raise_flagged(C: int) -> None:
    raise IndexError(f"a prediction or label lies outside [0, {C})")


def confusion(pred, y, num_classes: int, out=None, accumulate: bool = False, status=None, validate: bool = False):
    """``counts[a, p]`` = how many entries have label ``a`` and prediction ``p``: int32 ``[C, C]``.

    Device tensors (any integer dtype, any stride) are counted by ``bgcn_confusion`` on the current
    stream with no host sync; CPU tensors, numpy arrays and lists with numpy.  ``out``: an int32
    buffer of ``C * C`` contiguous elements on the inputs' device (a CPU tensor or numpy array for
    host inputs) that is overwritten, or added to with ``accumulate=True`` (which needs ``out``).
    An entry outside ``[0, C)`` is not counted and sets bit 0 of ``status`` (int32 ``[1]``, the
    package's convention); ``validate=True`` raises ``IndexError`` for one, at the cost of a host
    sync on the device path."""
    C = int(num_classes)
    if not 1 <= C <= MAX_CLASSES:
        raise ValueError(f"num_classes must be in [1, {MAX_CLASSES}]")
    if accumulate and out is None:
        raise ValueError("accumulate=True needs the buffer to add to (out)")
    if _is_dev(pred) or _is_dev(y):
        return _confusion_device(pred, y, C, out, accumulate, status, validate)
    p, a = _host_labels(pred), _host_labels(y)
    if p.size != a.size:
        raise ValueError("pred and y must have one entry each per tree")
    ok = (p >= 0) & (p < C) & (a >= 0) & (a < C)
    counts = np.bincount(a[ok] * C + p[ok], minlength=C * C).astype(np.int32).reshape(C, C)
    flagged = not bool(ok.all())
    if status is not None and flagged:
        status[0] |= 1
    if out is None:
        res = torch.from_numpy(counts)
    else:
        view = out.numpy() if isinstance(out, torch.Tensor) else out
        if view.dtype != np.int32 or view.size != C * C or not view.flags.c_contiguous:
            raise ValueError("out must be a contiguous int32 buffer of num_classes * num_classes elements")
        flat = view.reshape(-1)   # (a view: contiguous)
        flat[:] = flat + counts.reshape(-1) if accumulate else counts.reshape(-1)
        res = out
    if validate and flagged:
        _raise_flagged(C)
    return res


def _confusion_device(pred, y, C, out, accumulate, status, validate):
    if not (_is_dev(pred) and _is_dev(y)) or pred.device != y.device:
        raise ValueError("pred and y must be on the same device")
    for t in (pred, y):
        if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
            raise TypeError("labels and predictions must be integers")
    dev = pred.device
    p = pred.detach().reshape(-1).to(torch.int64).contiguous()
    a = y.detach().reshape(-1).to(torch.int64).contiguous()
    if p.numel() != a.numel():
        raise ValueError("pred and y must have one entry each per tree")
    if out is None:
        out = torch.empty(C, C, dtype=torch.int32, device=dev)
    elif (not _is_dev(out) or out.device != dev or out.dtype != torch.int32 or out.numel() != C * C
          or not out.is_contiguous()):
        raise ValueError("out must be a contiguous int32 device buffer of num_classes * num_classes elements")
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    elif not _is_dev(status) or status.device != dev or status.dtype != torch.int32 or status.numel() < 1:
        raise ValueError("status must be an int32 device tensor")
    # an empty tensor has no storage (a null pointer, which the library refuses): with B = 0 the
    # kernel reads neither array, so any valid address stands in and the bins are still written
    pp, pa = (ptr(p), ptr(a)) if p.numel() else (ptr(status), ptr(status))
    with torch.cuda.device(dev):
        check(_lib.lib().bgcn_confusion(pp, pa, p.numel(), C, ptr(out), int(bool(accumulate)), ptr(status),
                                        stream_handle()))
    if validate and int(status.reshape(-1)[0].item()) & 1:   # the one host sync
        _raise_flagged(C)
    return out


# ----------------------------------------------------------------------------- the reference's numbers
def _one_matrix(m: np.ndarray, K: int) -> tuple:
    n = int(m.sum())
    if n == 0:
        raise ValueError("no counted entry: the reference's metrics divide by the batch size")
    diag = [int(m[k, k]) for k in range(K)]
    out = [round(float(sum(diag)) / float(n), 4)]                     # Acc_all (evaluate.py:34)
    for k in range(K):
        TP = diag[k]
        FN = int(m[k, :].sum()) - TP                                  # any other prediction: "not this class"
        FP = int(m[:, k].sum()) - TP
        TN = n - TP - FN - FP
        acc = round(float(TP + TN) / float(TP + TN + FN + FP), 4)
        prec = 0 if TP + FP == 0 else round(float(TP) / float(TP + FP), 4)
        rec = 0 if TP + FN == 0 else round(float(TP) / float(TP + FN), 4)
        f = 0 if prec + rec == 0 else round(2 * prec * rec / (prec + rec), 4)   # from the rounded values
        out += [acc, prec, rec, f]
    return tuple(out)


def class_metrics(counts, reference_classes: int):
    """What the reference's ``evaluation4class`` (``reference_classes=4``) / ``evaluationclass``
    (``2``) return, from integer counts ``[..., C, C]`` (row = actual, column = predicted,
    ``C >= reference_classes``): the tuple ``(Acc_all, Acc1, Prec1, Recll1, F1, Acc2, ...)`` of
    ``1 + 4 * reference_classes`` numbers; with leading dimensions, a list of such tuples (nested
    per dimension).

    Per class k: TP = ``counts[k, k]``, FN / FP = the rest of row / column k, TN = everything
    else, so a label or prediction of a class beyond the leading ones counts as "not this class",
    as the reference's comparisons have it; ``Acc_all`` is the leading diagonal over the number of
    counted entries.  Every ratio is ``round(., 4)`` of a Python float division, ``Prec`` /
    ``Recll`` / ``F`` are ``0`` where their denominator is zero, and ``F`` is computed from the
    rounded ``Prec`` and ``Recll``.  A matrix without entries raises ``ValueError`` (the reference
    divides by zero)."""
    K = int(reference_classes)
    if isinstance(counts, torch.Tensor):
        counts = counts.detach().cpu().numpy()   # (a device tensor: one read)
    m = np.asarray(counts)
    if m.dtype.kind not in "iu":
        raise TypeError("counts must be integers")
    if m.ndim < 2 or m.shape[-1] != m.shape[-2]:
        raise ValueError("counts must be [..., C, C]")
    if not 1 <= K <= m.shape[-1]:
        raise ValueError("reference_classes must be in [1, C]")
    if m.ndim == 2:
        return _one_matrix(m, K)
    return [class_metrics(sub, K) for sub in m]


def _drop_in(prediction, y, K: int) -> tuple:
    n = len(y)
    if n == 0:
        raise ValueError("an empty batch has no metrics (the reference divides by its size)")
    C = MAX_CLASSES
    if _is_dev(prediction) or _is_dev(y):
        dev = prediction.device if _is_dev(prediction) else y.device
        buf = torch.zeros(C * C + 1, dtype=torch.int32, device=dev)      # the counts and the status word:
        confusion(prediction, y, C, out=buf[:C * C], status=buf[C * C:])  # one kernel,
        host = buf.cpu().numpy()                                          # one read
    else:
        host = np.zeros(C * C + 1, dtype=np.int32)
        confusion(prediction, y, C, out=host[:C * C], status=host[C * C:])
    if host[C * C] & 1:
        _raise_flagged(C)
    return _one_matrix(host[:C * C].reshape(C, C), K)


def evaluation4class(prediction, y) -> tuple:
    """Drop-in for the reference's ``evaluation4class`` (``tools/evaluate.py:3-91``): the 17 numbers
    ``Acc_all, Acc1, Prec1, Recll1, F1, ..., Acc4, Prec4, Recll4, F4``, equal to the reference's
    digit for digit.  ``prediction`` / ``y``: device tensors (one kernel and one read instead of a
    sync per comparison), CPU tensors, numpy arrays or lists.  Only classes 0..3 get numbers; a
    label of 4..15 counts as "not this class" and ``Acc_all`` divides by ``len(y)``, as in the
    reference.  Labels must lie in ``[0, 16)`` (``IndexError``); an empty batch raises
    ``ValueError``."""
    return _drop_in(prediction, y, 4)


def evaluationclass(prediction, y) -> tuple:
    """Drop-in for the reference's two-class ``evaluationclass`` (``tools/evaluate.py:93-139``): 9
    numbers.  See :func:`evaluation4class`."""
    return _drop_in(prediction, y, 2)


# ----------------------------------------------------------------------------- one validation epoch
class EpochResult(NamedTuple):
    """What :meth:`EpochMetrics.result` returns.  ``loss`` / ``acc``: ``np.mean`` of the per-batch
    losses / of the per-batch ``correct / len(y)`` (``BiGCN_Twitter.py:234-235``); ``metrics``: the
    per-batch :func:`class_metrics` tuples (``batch_metrics``) averaged per position with
    ``np.mean`` (``:239-247``); ``confusion``: the epoch's total matrix, int64 ``[C, C]``;
    ``precision`` / ``recall`` / ``f1``: float64 ``[C]``, unrounded from that total as the explain
    run computes them (``explain_PHEME.py:652-663``), ``nan`` for a class never predicted / never
    present; ``losses`` / ``correct`` / ``sizes``: the per-batch records."""
    loss: float
    acc: float
    metrics: Tuple[float, ...]
    confusion: np.ndarray
    precision: np.ndarray
    recall: np.ndarray
    f1: np.ndarray
    batch_metrics: List[tuple]
    losses: np.ndarray
    correct: np.ndarray
    sizes: np.ndarray


class EpochMetrics:
    """The bookkeeping of one validation epoch in device buffers::

        m = EpochMetrics(num_classes=4, max_batches=len(test_loader), device=device)
        for batch in test_loader:
            loss, correct, pred = step.evaluate(batch, pred=True)
            m.add(pred, batch.y, loss, correct)          # no host sync
        r = m.result()                                   # one device-to-host read

    One int32 buffer holds ``max_batches`` confusion matrices ``[max_batches, C, C]``, the batches'
    losses (fp32), correct counts and sizes, and a status word.  ``device`` may be the CPU (host
    inputs, counted with numpy)."""

    def __init__(self, num_classes: int, max_batches: int, device=None):
        C, M = int(num_classes), int(max_batches)
        if not 1 <= C <= MAX_CLASSES:
            raise ValueError(f"num_classes must be in [1, {MAX_CLASSES}]")
        if M < 1:
            raise ValueError("max_batches must be at least 1")
        self.num_classes, self.max_batches = C, M
        self.device = torch.device("cuda" if device is None else device)
        buf = torch.zeros(M * (C * C + 3) + 1, dtype=torch.int32, device=self.device)
        self._buf = buf
        self.counts = buf[:M * C * C].view(M, C, C)
        rest = buf[M * C * C:]
        self.losses = rest[:M].view(torch.float32)
        self.correct = rest[M:2 * M]
        self.sizes = rest[2 * M:3 * M]
        self.status = rest[3 * M:]
        self.reset()

    def __len__(self) -> int:
        return self._n

    def reset(self) -> None:
        """Start a new epoch in the same buffers (no host sync)."""
        self._n = 0
        self._no_loss = False
        self._no_correct = []
        self.status.zero_()

    def add(self, pred, y, loss=None, correct=None) -> None:
        """Record one batch in the next slot, without a host sync: its confusion matrix
        (:func:`confusion` straight into the slot), its size, and ``loss`` / ``correct`` as
        ``FusedTrainStep.evaluate`` returns them (device-to-device copies; numbers are accepted
        too).  Without ``loss`` the epoch's mean loss is ``nan``; without ``correct`` the matrix's
        diagonal is taken.  Raises ``IndexError`` when all ``max_batches`` slots are taken."""
        k = self._n
        if k >= self.max_batches:
            raise IndexError(f"EpochMetrics holds {self.max_batches} batches (max_batches); reset() starts a new epoch")
        confusion(pred, y, self.num_classes, out=self.counts[k], status=self.status)
        self.sizes[k].fill_(int(y.numel()) if isinstance(y, torch.Tensor) else int(np.asarray(y).size))
        if loss is None:
            self._no_loss = True
        elif isinstance(loss, torch.Tensor):
            self.losses[k:k + 1].copy_(loss.detach().reshape(1))
        else:
            self.losses[k].fill_(float(loss))
        if correct is None:
            self._no_correct.append(k)
        elif isinstance(correct, torch.Tensor):
            self.correct[k:k + 1].copy_(correct.detach().reshape(1))
        else:
            self.correct[k].fill_(int(correct))
        self._n = k + 1

    def result(self) -> EpochResult:
        """The epoch's numbers, after ONE device-to-host read of the record buffer.  A prediction or
        label outside ``[0, C)`` in any batch raises ``IndexError``, an epoch without batches (or
        with an empty batch) ``ValueError``."""
        n, C, M = self._n, self.num_classes, self.max_batches
        if n == 0:
            raise ValueError("no batch was added")
        host = self._buf.cpu().numpy()   # the one read
        if host[-1] & 1:
            _raise_flagged(C)
        counts = host[:M * C * C].reshape(M, C, C)[:n].astype(np.int64)
        rest = host[M * C * C:]
        losses = rest[:M].view(np.float32)[:n].copy()
        correct = rest[M:2 * M][:n].astype(np.int64)
        sizes = rest[2 * M:3 * M][:n].astype(np.int64)
        for k in self._no_correct:
            correct[k] = int(np.trace(counts[k]))
        if (sizes == 0).any():
            raise ValueError("an empty batch has no metrics (the reference divides by its size)")
        per_batch = class_metrics(counts, C)
        # the reference appends val_loss.item() and correct / len(y) per batch and logs np.mean of the lists
        loss = float("nan") if self._no_loss else float(np.mean([float(v) for v in losses]))
        acc = float(np.mean([int(c) / int(s) for c, s in zip(correct, sizes)]))
        means = tuple(float(np.mean([t[j] for t in per_batch])) for j in range(1 + 4 * C))
        total = counts.sum(0)
        conf = total.astype(np.float64)   # explain_PHEME.py:480 counts in a float matrix
        with np.errstate(divide="ignore", invalid="ignore"):
            precision = conf.diagonal() / conf.sum(0)
            recall = conf.diagonal() / conf.sum(1)
            f1 = 2 * precision * recall / (precision + recall)
        return EpochResult(loss, acc, means, total, precision, recall, f1, per_batch, losses, correct, sizes)
