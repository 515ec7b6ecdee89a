"""GPU checks of bigcn_amd.metrics: bgcn_confusion against a numpy count (integers: bit for bit),
EpochMetrics on the device against the recorded reference numbers of tests/golden/metrics_cases.npz,
FusedTrainStep.validate against a manual loop of evaluate() - and that the validation loop up to
result() performs no host sync (torch's sync debug mode set to "error")."""
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import bigcn_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SIZES = (0, 1, 63, 64, 65, 257, 1000)     # below, at and above a wave; more than the 256 threads; several strides
CLASSES = (2, 4, 16)


def _np_count(pred, y, C):
    pred, y = np.asarray(pred, dtype=np.int64), np.asarray(y, dtype=np.int64)
    ok = (pred >= 0) & (pred < C) & (y >= 0) & (y < C)
    return np.bincount(y[ok] * C + pred[ok], minlength=C * C).reshape(C, C).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _labels(B, C):
    """(pred, y): random, and with every (label, prediction) pair present once B >= C * C."""
    rng = np.random.default_rng(1000 * C + B)
    pred, y = rng.integers(0, C, size=B), rng.integers(0, C, size=B)
    if B >= C * C:
        pairs = np.arange(C * C)
        y[:C * C], pred[:C * C] = pairs // C, pairs % C
        order = rng.permutation(B)
        pred, y = pred[order], y[order]
        assert (_np_count(pred, y, C) > 0).all()
    return pred.astype(np.int64), y.astype(np.int64)


def _dev(a, dtype=torch.int64):
    return torch.as_tensor(a).to(DEV, dtype)


@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("B", SIZES)
def test_confusion_is_the_numpy_count(B, C):
    from bigcn_amd import confusion
    pred, y = _labels(B, C)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = confusion(_dev(pred), _dev(y), C, status=status)
    assert got.dtype == torch.int32 and got.shape == (C, C) and got.device == DEV
    assert np.array_equal(got.cpu().numpy(), _np_count(pred, y, C))
    assert int(status) == 0
    # the same launch again: the same bits
    again = confusion(_dev(pred), _dev(y), C)
    assert torch.equal(got, again)


@pytest.mark.parametrize("C", CLASSES)
def test_accumulate_adds_and_overwrite_ignores_what_the_buffer_held(C):
    from bigcn_amd import confusion
    (p0, y0), (p1, y1) = _labels(257, C), _labels(1000, C)
    want0, want1 = _np_count(p0, y0, C), _np_count(p1, y1, C)
    out = torch.full((C, C), -12345, dtype=torch.int32, device=DEV)     # garbage: no zeroing before the call
    assert confusion(_dev(p0), _dev(y0), C, out=out) is out
    assert np.array_equal(out.cpu().numpy(), want0)
    confusion(_dev(p1), _dev(y1), C, out=out, accumulate=True)
    assert np.array_equal(out.cpu().numpy(), want0 + want1)
    # B = 0: accumulate leaves the buffer, overwrite leaves zeros
    empty = torch.zeros(0, dtype=torch.int64, device=DEV)
    confusion(empty, empty, C, out=out, accumulate=True)
    assert np.array_equal(out.cpu().numpy(), want0 + want1)
    confusion(empty, empty, C, out=out)
    assert int(out.abs().sum()) == 0
    # a slot of a larger buffer: the neighbours stay as they were
    slots = torch.full((3, C, C), 9, dtype=torch.int32, device=DEV)
    confusion(_dev(p0), _dev(y0), C, out=slots[1])
    assert np.array_equal(slots[1].cpu().numpy(), want0) and bool((slots[0] == 9).all()) and bool((slots[2] == 9).all())


@pytest.mark.parametrize("C", CLASSES)
def test_entries_out_of_range_are_flagged_and_not_counted(C):
    from bigcn_amd import confusion
    pred, y = (a.copy() for a in _labels(257, C))
    pred[[3, 70, 200]] = [-1, C, 2**40]
    y[[5, 70, 256]] = [C, -2**63, -7]
    want = _np_count(pred, y, C)
    assert int(want.sum()) == 257 - 5
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = confusion(_dev(pred), _dev(y), C, status=status)
    assert np.array_equal(got.cpu().numpy(), want)
    assert int(status) == 1
    with pytest.raises(IndexError):
        confusion(_dev(pred), _dev(y), C, validate=True)
    # bits a caller's status word already holds are kept
    status.fill_(4)
    confusion(_dev(pred), _dev(y), C, status=status)
    assert int(status) == 5
    confusion(_dev(_labels(65, C)[0]), _dev(_labels(65, C)[1]), C, status=status, validate=False)
    assert int(status) == 5


def test_int32_and_strided_inputs():
    from bigcn_amd import confusion
    pred, y = _labels(1000, 4)
    wide = torch.full((1000, 3), 77, dtype=torch.int64, device=DEV)
    wide[:, 1] = _dev(pred)
    got = confusion(wide[:, 1], _dev(y, torch.int32), 4)
    assert np.array_equal(got.cpu().numpy(), _np_count(pred, y, 4))
    got = confusion(_dev(pred, torch.int32)[::2], _dev(y, torch.uint8)[::2], 4)
    assert np.array_equal(got.cpu().numpy(), _np_count(pred[::2], y[::2], 4))
    got = confusion(_dev(pred).view(1000, 1), _dev(y), 4)      # [B, 1] predictions
    assert np.array_equal(got.cpu().numpy(), _np_count(pred, y, 4))
    with pytest.raises(TypeError):
        confusion(_dev(pred).float(), _dev(y), 4)
    with pytest.raises(ValueError):
        confusion(_dev(pred), torch.as_tensor(y), 4)           # one on the host
    with pytest.raises(ValueError):
        confusion(_dev(pred), _dev(y), 4, out=torch.zeros(4, 4, dtype=torch.int64, device=DEV))


def test_drop_ins_on_device_tensors_return_the_reference_tuples():
    from bigcn_amd import evaluation4class, evaluationclass
    g = load_golden("metrics_cases.npz")
    for key, fn in (("names4", evaluation4class), ("names2", evaluationclass)):
        for n in (str(n) for n in g[key]):
            assert fn(_dev(g[n + ":pred"]), _dev(g[n + ":y"])) == tuple(g[n + ":ref"].tolist()), n
    empty = torch.zeros(0, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError):
        evaluation4class(empty, empty)
    with pytest.raises(IndexError):
        evaluation4class(_dev([0, 16]), _dev([0, 1]))


def test_epoch_metrics_on_the_device_returns_the_recorded_epoch():
    from bigcn_amd import EpochMetrics
    g = load_golden("metrics_cases.npz")
    m = EpochMetrics(4, 3, DEV)
    assert m.counts.shape == (3, 4, 4) and m.counts.dtype == torch.int32 and m.counts.device == DEV
    assert m.losses.dtype == torch.float32 and m.correct.shape == (3,) and m.sizes.shape == (3,)
    for rep in range(2):        # reset() gives a clean second epoch in the same buffers
        for k in range(3):
            pred, y = _dev(g[f"epoch:pred:{k}"]), _dev(g[f"epoch:y:{k}"])
            loss = torch.tensor(g["epoch:loss"][k], device=DEV)
            correct = pred.eq(y).sum().to(torch.int32)
            m.add(pred, y, loss, correct)
        with pytest.raises(IndexError):
            m.add(pred, y, loss, correct)
        r = m.result()
        assert r.loss == float(g["epoch:loss_mean"]) and r.acc == float(g["epoch:acc_mean"])
        assert r.metrics == tuple(g["epoch:mean"].tolist())
        assert r.batch_metrics == [tuple(t) for t in g["epoch:tuples"].tolist()]
        assert np.array_equal(r.confusion, g["epoch:conf"])
        for got, key in ((r.precision, "precision"), (r.recall, "recall"), (r.f1, "f1")):
            assert np.array_equal(got, g["epoch:" + key], equal_nan=True), key
        assert np.array_equal(r.sizes, [7, 5, 3]) and np.array_equal(r.correct, [
            int((g[f"epoch:pred:{k}"] == g[f"epoch:y:{k}"]).sum()) for k in range(3)])
        m.reset()
    m.add(_dev([0, 9]), _dev([0, 1]))
    with pytest.raises(IndexError):
        m.result()


def _validation_set():
    """A small 4-class model (F = 32) and three ragged batches of 2-5 small trees."""
    from bigcn_amd import BiGCN
    from bigcn_amd.data import synth_batch
    rng = np.random.default_rng(77)
    batches = [synth_batch(rng, sizes, 32, 4, 0.0, 0.0, device=DEV) for sizes in ([3, 5, 2], [1, 4, 6, 2, 3], [7, 2])]
    for b in batches:     # labels that do not follow the tree index
        b.y = torch.as_tensor(rng.integers(0, 4, size=b.num_graphs), device=DEV)
    model = BiGCN(32, 64, 64).to(DEV)
    model.load_state_dict({k: v.float() for k, v in O.make_params(32, 64, 64, 4, seed=5).items()})
    return model.eval(), batches


def test_validate_is_the_manual_loop_and_does_not_sync():
    from bigcn_amd import EpochMetrics, FusedTrainStep, evaluation4class
    model, batches = _validation_set()
    step = FusedTrainStep(model)
    # the manual loop: evaluate() per batch, the metrics on the CPU from the copied predictions
    manual = []
    for b in batches:
        loss, correct, pred = step.evaluate(b, pred=True)
        manual.append((loss.clone(), correct.clone(), pred.clone()))
    torch.cuda.synchronize()
    step.check_status()
    tuples = [evaluation4class(pred.cpu().tolist(), b.y.cpu().tolist()) for (_, _, pred), b in zip(manual, batches)]

    try:
        torch.cuda.set_sync_debug_mode("error")
        sync_checked = True
    except Exception:       # this torch build has no such mode: the loop still runs, unchecked
        sync_checked = False
    try:
        m = step.validate(batches)                      # a host sync in here raises
        m2 = EpochMetrics(4, 3, DEV)
        assert step.validate(batches[:2], m2) is m2
        step.validate(batches[2:], m2)                  # records are appended
        if sync_checked:                                # the mode is live: reading a device word raises
            with pytest.raises(RuntimeError):
                m.status.item()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    print("sync debug mode checked:", sync_checked)
    assert len(m) == 3 and len(m2) == 3
    for res in (m.result(), m2.result()):
        for k, (loss, correct, pred) in enumerate(manual):
            assert res.losses[k] == float(loss) and res.correct[k] == int(correct)
            assert res.correct[k] == int(pred.eq(batches[k].y).sum())
            assert res.sizes[k] == batches[k].num_graphs
        assert res.batch_metrics == tuples
        assert res.metrics == tuple(float(np.mean([t[j] for t in tuples])) for j in range(17))
        assert res.loss == float(np.mean([float(l) for l, _, _ in manual]))
        assert res.acc == float(np.mean([int(c) / b.num_graphs for (_, c, _), b in zip(manual, batches)]))
        want = sum(_np_count(p.cpu().numpy(), b.y.cpu().numpy(), 4).astype(np.int64) for (_, _, p), b in zip(manual, batches))
        assert np.array_equal(res.confusion, want)
    step.check_status()
    with pytest.raises(IndexError):
        step.validate(batches, m2)                      # no room left
    with pytest.raises(ValueError):
        step.validate([])


def test_explanation_confusion_counts_prediction_against_y():
    from bigcn_amd import explain
    model, batches = _validation_set()
    fold = torch.zeros(4, 4, dtype=torch.int32, device=DEV)
    total = np.zeros((4, 4), dtype=np.int32)
    for b in batches[:2]:
        ex = explain(model, b)
        want = _np_count(ex.prediction.cpu().numpy(), b.y.cpu().numpy(), 4)
        got = ex.confusion()
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
        assert np.array_equal(ex.confusion(num_classes=16).cpu().numpy()[:4, :4], want)
        assert ex.confusion(out=fold) is fold
        total += want
    assert np.array_equal(fold.cpu().numpy(), total) and int(total.sum()) == 3 + 5
    ex.y = None
    with pytest.raises(ValueError):
        ex.confusion()
