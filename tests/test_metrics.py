"""CPU checks of bigcn_amd.metrics against tests/golden/metrics_cases.npz: the tuples the reference's
own tools/evaluate.py returned for the recorded (prediction, y) cases (tools/gen_metrics_golden.py).
Every comparison is `==` on Python floats: the numbers are derived from integer counts by the
reference's own arithmetic (round(., 4) of float divisions), so they agree digit for digit.
The argument checks of bgcn_confusion run before any device work and need no GPU."""
import numpy as np
import pytest
import torch

from conftest import load_golden


@pytest.fixture(scope="module")
def cases():
    return load_golden("metrics_cases.npz")


def _names(g, key):
    return [str(n) for n in g[key]]


def _np_count(pred, y, C):
    m = np.zeros((C, C), dtype=np.int64)
    for p, a in zip(np.asarray(pred).tolist(), np.asarray(y).tolist()):
        if 0 <= p < C and 0 <= a < C:
            m[a, p] += 1
    return m


def _ref(g, name):
    return tuple(g[name + ":ref"].tolist())


def test_fixture_covers_the_cases_the_metrics_can_go_wrong_on(cases):
    g = cases
    n4, n2 = _names(g, "names4"), _names(g, "names2")
    sizes4 = {len(g[n + ":y"]) for n in n4}
    assert {1, 3, 7, 9, 11} <= sizes4 and 1 in {len(g[n + ":y"]) for n in n2}
    assert any(len(set(g[n + ":y"].tolist()) | set(g[n + ":pred"].tolist())) == 1 for n in n4)   # one class only
    assert any(2 not in g[n + ":pred"] and 2 in g[n + ":y"] for n in n4)        # a class never predicted
    assert any(3 not in g[n + ":y"] and 3 in g[n + ":pred"] for n in n4)        # a class never present
    assert any(int(g[n + ":y"].max()) >= 4 for n in n4) and any(int(g[n + ":y"].max()) >= 2 for n in n2)
    # Prec + Recll == 0 with a non-zero denominator each: TP = 0, FP > 0, FN > 0 for class 0
    m = _np_count(g["4:prec_recll_zero:pred"], g["4:prec_recll_zero:y"], 4)
    assert m[0, 0] == 0 and m[:, 0].sum() > 0 and m[0, :].sum() > 0
    assert [len(g[f"epoch:y:{k}"]) for k in range(3)] == [7, 5, 3]
    for n in n4:
        assert g[n + ":ref"].shape == (17,)
    for n in n2:
        assert g[n + ":ref"].shape == (9,)


@pytest.mark.parametrize("form", ["numpy", "list", "tensor", "int32_tensor"])
def test_drop_ins_return_the_reference_tuples(cases, form):
    from bigcn_amd import evaluation4class, evaluationclass
    conv = {"numpy": lambda a: a, "list": lambda a: a.tolist(), "tensor": torch.from_numpy,
            "int32_tensor": lambda a: torch.from_numpy(a.astype(np.int32))}[form]
    g = cases
    for key, fn, arity in (("names4", evaluation4class, 17), ("names2", evaluationclass, 9)):
        for n in _names(g, key):
            got = fn(conv(g[n + ":pred"]), conv(g[n + ":y"]))
            assert isinstance(got, tuple) and len(got) == arity
            assert got == _ref(g, n), n


def test_class_metrics_from_numpy_counts(cases):
    from bigcn_amd import class_metrics
    g = cases
    for key, K in (("names4", 4), ("names2", 2)):
        for n in _names(g, key):
            C = max(K, int(max(g[n + ":y"].max(), g[n + ":pred"].max())) + 1)
            m = _np_count(g[n + ":pred"], g[n + ":y"], C)
            assert class_metrics(m, K) == _ref(g, n), n
            assert class_metrics(m.astype(np.int32), K) == _ref(g, n), n
            assert class_metrics(torch.from_numpy(m), K) == _ref(g, n), n
    # leading dimensions: one tuple per matrix
    stack = np.stack([_np_count(g[f"epoch:pred:{k}"], g[f"epoch:y:{k}"], 4) for k in range(3)])
    assert class_metrics(stack, 4) == [tuple(t) for t in g["epoch:tuples"].tolist()]
    with pytest.raises(ValueError):
        class_metrics(np.zeros((4, 4), dtype=np.int64), 4)
    with pytest.raises(ValueError):
        class_metrics(np.ones((2, 2), dtype=np.int64), 4)
    with pytest.raises(TypeError):
        class_metrics(np.ones((4, 4)), 4)


def test_confusion_on_the_host_is_the_numpy_count(cases):
    from bigcn_amd import confusion
    g = cases
    for n in _names(g, "names4"):
        pred, y = g[n + ":pred"], g[n + ":y"]
        for C in (2, 4, 16):
            want = _np_count(pred, y, C)
            status = np.zeros(1, dtype=np.int32)
            got = confusion(pred, y, C, status=status)
            assert got.dtype == torch.int32 and np.array_equal(got.numpy(), want)
            inside = bool(((pred >= 0) & (pred < C) & (y >= 0) & (y < C)).all())
            assert int(status[0]) == (0 if inside else 1)
            if not inside:
                with pytest.raises(IndexError):
                    confusion(pred, y, C, validate=True)
    out = torch.full((4, 4), 7, dtype=torch.int32)
    pred, y = g["4:rand11:pred"], g["4:rand11:y"]
    assert confusion(pred, y, 4, out=out) is out and np.array_equal(out.numpy(), _np_count(pred, y, 4))
    confusion(torch.from_numpy(pred), torch.from_numpy(y), 4, out=out, accumulate=True)
    assert np.array_equal(out.numpy(), 2 * _np_count(pred, y, 4))
    assert np.array_equal(confusion([], [], 4).numpy(), np.zeros((4, 4)))
    assert np.array_equal(confusion([-1, 0], [0, 0], 4).numpy(), _np_count([0], [0], 4))
    for bad in (0, 17):
        with pytest.raises(ValueError):
            confusion(pred, y, bad)
    with pytest.raises(ValueError):
        confusion(pred, y, 4, accumulate=True)
    with pytest.raises(ValueError):
        confusion(pred[:3], y, 4)


def test_epoch_means_equal_the_recorded_ones(cases):
    from bigcn_amd import EpochMetrics
    g = cases
    m = EpochMetrics(4, 3, "cpu")
    for rep in range(2):        # the second epoch after reset() is as clean as the first
        for k in range(3):
            pred, y = g[f"epoch:pred:{k}"], g[f"epoch:y:{k}"]
            correct = int((pred == y).sum())
            if k == 1:
                m.add(torch.from_numpy(pred), torch.from_numpy(y), torch.tensor(g["epoch:loss"][k]),
                      torch.tensor(correct, dtype=torch.int32))
            else:
                m.add(pred.tolist(), y.tolist(), float(g["epoch:loss"][k]), None if k == 2 else correct)
        assert len(m) == 3
        with pytest.raises(IndexError):
            m.add([0], [0])
        r = m.result()
        assert r.loss == float(g["epoch:loss_mean"]) and r.acc == float(g["epoch:acc_mean"])
        assert r.metrics == tuple(g["epoch:mean"].tolist())
        assert r.batch_metrics == [tuple(t) for t in g["epoch:tuples"].tolist()]
        assert r.confusion.dtype == np.int64 and np.array_equal(r.confusion, g["epoch:conf"])
        for got, key in ((r.precision, "precision"), (r.recall, "recall"), (r.f1, "f1")):
            want = g["epoch:" + key]
            assert np.isnan(want).any() or key == "precision"      # (class 3 is never a label)
            assert np.array_equal(got, want, equal_nan=True), key
        assert np.array_equal(r.sizes, [7, 5, 3]) and np.array_equal(r.losses, g["epoch:loss"])
        m.reset()
        assert len(m) == 0
    with pytest.raises(ValueError):
        m.result()
    m.add([0, 9], [0, 1])
    with pytest.raises(IndexError):
        m.result()


def test_empty_batch_raises():
    from bigcn_amd import EpochMetrics, evaluation4class, evaluationclass
    for fn in (evaluation4class, evaluationclass):
        with pytest.raises(ValueError):
            fn([], [])
        with pytest.raises(ValueError):
            fn(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64))
        with pytest.raises(IndexError):
            fn([0, 16], [0, 1])
        with pytest.raises(IndexError):
            fn([0, 1], [0, -1])
    m = EpochMetrics(2, 1, "cpu")
    m.add([], [])
    with pytest.raises(ValueError):
        m.result()


def test_confusion_entry_point_refuses_bad_arguments_before_any_device_work():
    """Fake 16-byte-aligned addresses that are never dereferenced: every call is refused."""
    from bigcn_amd import _lib
    lib = _lib.load_library()
    P = 4096
    good = dict(pred=P, y=P + 64, B=5, C=4, counts=P + 128, acc=0, status=P + 256)

    def call(**kw):
        a = dict(good, **kw)
        return lib.bgcn_confusion(a["pred"], a["y"], a["B"], a["C"], a["counts"], a["acc"], a["status"], None)

    for name in ("pred", "y", "counts", "status"):
        assert call(**{name: None}) == -1, name
        assert b"null pointer" in lib.bgcn_last_error()
    for C in (0, 17, -1):
        assert call(C=C) == -1
        assert b"num_classes must be in [1, 16]" in lib.bgcn_last_error()
    assert call(B=-1) == -1
    assert b"negative size" in lib.bgcn_last_error()
    assert lib.bgcn_abi_version() == 12


def test_binding_and_package_list_the_new_names():
    import bigcn_amd
    from bigcn_amd import _lib, metrics
    assert "bgcn_confusion" in _lib.EXPORTED_SYMBOLS and "bgcn_confusion" in _lib._SIGS
    assert len(_lib._SIGS["bgcn_confusion"][1]) == 8
    for name in ("metrics", "confusion", "class_metrics", "evaluation4class", "evaluationclass", "EpochMetrics"):
        assert name in bigcn_amd.__all__ and getattr(bigcn_amd, name) is not None
    assert bigcn_amd.metrics is metrics and bigcn_amd.confusion is metrics.confusion
    from bigcn_amd import FusedTrainStep
    from bigcn_amd.explain import Explanation
    assert callable(FusedTrainStep.validate) and callable(Explanation.confusion)

