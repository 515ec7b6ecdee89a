"""GPU checks of the LSTM baseline (bgcn_lstm_eval, bigcn_amd.LSTM) against the fp64 restatement
tests/lstm_ref.py, which loops torch.nn.LSTM over the trees as the reference does.

Bar: last-layer ``out``, ``h_n`` and ``logp`` within 1e-4 absolute of the fp64 oracle
(test_lstm.py::test_the_bar_is_feasible shows torch's own fp32 at <= 1e-5 on the same cases).
With BGCN_LSTM_PARITY_OUT set, each case's worst error and margin go to that JSON file
(profiles/lstm_parity.json is such a record)."""
import functools
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lstm_ref as R
from lstm_gpu_util import DEV, _data, _new_model, _x

pytestmark = pytest.mark.gpu

TOL = 1e-4
SEQ_TILE = 32   # sequences per workgroup of a step launch (BGCN_LSTM_SEQ_TILE): "tile_plus_one" has 33
_parity = {}


@functools.lru_cache(maxsize=None)
def _model(name, version=2, pooling='max'):
    return _new_model(R.case(name), version=version, pooling=pooling)


def _err(got, want):
    return float((got.double().cpu() - want).abs().max())


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_parity_with_the_fp64_oracle(name):
    from bigcn_amd import _lib
    assert SEQ_TILE == _lib.BGCN_LSTM_SEQ_TILE
    c = R.case(name)
    m = _model(name)
    x = _x(c)
    logp, out, h_n = m.forward_batch(x, c.rootindex.to(DEV), max_len=c.max_len, return_states=True)
    m.check_status()
    errs = {"out": _err(out, c.ref.out), "h_n": _err(h_n, c.ref.h_n), "logp": _err(logp, c.ref.logp)}
    print(name, {k: f"{v:.3e}" for k, v in errs.items()})
    _parity[name] = {"N": c.N, "B": c.B, "in_feats": c.cfg["in_feats"], "hid": c.cfg["hid"],
                     "layers": c.cfg["layers"], "out_feats": c.cfg["out"], "weight_factor": c.weight_factor,
                     "max_abs_err": errs, "bar": TOL, "margin": TOL / max(max(errs.values()), 1e-30)}
    path = os.environ.get("BGCN_LSTM_PARITY_OUT")
    if path:
        with open(path, "w") as f:
            json.dump(_parity, f, indent=1, sort_keys=True)
    for what, e in errs.items():
        assert e <= TOL, (what, e)
    if name == "tile_plus_one":
        assert c.B == SEQ_TILE + 1
    if name == "offset_strided":
        assert int(c.rootindex[0]) == 2 and x.stride(0) > c.cfg["in_feats"]
        assert float(out[:2].abs().sum()) == 0.0


def test_forward_of_one_tree_is_its_row_of_the_batch():
    """``forward(tensor)`` on one tree equals that tree's row of ``forward_batch``; a tree alone and
    inside a batch agree to 1e-6 (by design bitwise below the input GEMM's kernel switch)."""
    c = R.case("boundaries")
    m = _model("boundaries")
    x = _x(c)
    logp, out, h_n = m.forward_batch(x, c.rootindex.to(DEV), max_len=c.max_len, return_states=True)
    ends = c.rootindex.tolist()[1:] + [c.N]
    for b, (s, e) in enumerate(zip(c.rootindex.tolist(), ends)):
        one = m(x[s:e])
        assert one.shape == (1, c.cfg["out"])
        assert float((one[0] - logp[b]).abs().max()) <= 1e-6
        l1, o1, h1 = m.forward_batch(x[s:e], torch.zeros(1, dtype=torch.int64), return_states=True)
        assert float((o1 - out[s:e]).abs().max()) <= 1e-6
        assert float((h1[:, 0] - h_n[:, b]).abs().max()) <= 1e-6
    m.check_status()


@pytest.mark.parametrize("pooling", ["max", "mean"])
def test_pooled_versions_equal_pooling_in_torch(pooling):
    c = R.case("boundaries")
    m2, m0 = _model("boundaries"), _model("boundaries", 0, pooling)
    g = torch.Generator().manual_seed(5)
    T, F_in = 3, c.cfg["in_feats"]
    raw = torch.randn(c.N, T, F_in, generator=g).to(DEV)
    pooled = raw.amax(dim=1) if pooling == "max" else raw.mean(dim=1)
    want = m2.forward_batch(pooled, c.rootindex.to(DEV), max_len=c.max_len)
    # the per-tree call on [n, T, in]
    s, e = int(c.rootindex[3]), int(c.rootindex[4])
    assert float((m0(raw[s:e]) - want[3:4]).abs().max()) <= 1e-6
    # the batch call on data.x [N, T * in]
    data = SimpleNamespace(x=raw.reshape(c.N, T * F_in), rootindex=c.rootindex.to(DEV), y=c.y.to(DEV))
    got = torch.empty_like(want)
    loss, correct = m0.evaluate(data, logp=got, max_len=c.max_len)
    assert torch.equal(got, want)
    assert abs(float(loss) - float(F.nll_loss(want, c.y.to(DEV)))) <= 1e-6


@pytest.mark.parametrize("name", ["boundaries", "twitter", "tile_plus_one"])
def test_evaluate_is_the_reference_loop(name):
    c = R.case(name)
    m = _model(name)
    data = _data(c)
    loss, correct, pred = m.evaluate(data, pred=True, max_len=None if name == "boundaries" else c.max_len)
    m.check_status()
    assert loss.shape == () and correct.dtype == torch.int32 and pred.dtype == torch.int64
    want_loss = float(F.nll_loss(c.ref.logp, c.y))
    print(name, "loss", float(loss), "oracle", want_loss)
    assert abs(float(loss) - want_loss) <= TOL
    ok = R.margin_ok(c.ref.logp)
    assert float(ok.float().mean()) >= 0.9
    assert torch.equal(pred.cpu()[ok], c.ref.pred[ok])
    assert int(correct) == int(pred.cpu().eq(c.y).sum())
    if bool(ok.all()):
        assert int(correct) == c.ref.correct


def test_validate_feeds_epoch_metrics():
    from bigcn_amd import evaluation4class
    c = R.case("boundaries")
    m = _model("boundaries")
    lstm, fc = R.build(c.cfg["in_feats"], c.cfg["hid"], c.cfg["out"], c.cfg["layers"], torch.float64, c.seed)
    roots = c.rootindex.tolist()
    # three batches cut from the case: all six trees, the first three, the last three
    cuts = [(0, c.N, roots), (0, roots[3], roots[:3]), (roots[3], c.N, [r - roots[3] for r in roots[3:]])]
    batches, tuples, losses = [], [], []
    for (s, e, r), ys in zip(cuts, (c.y, c.y[:3], c.y[3:])):
        x, r = c.x[s:e].contiguous(), torch.tensor(r)
        ref = R.run(lstm, fc, x, r, ys)
        assert bool(R.margin_ok(ref.logp).all())
        batches.append(SimpleNamespace(cls=x.to(DEV), rootindex=r.to(DEV), y=ys.to(DEV)))
        tuples.append(evaluation4class(ref.pred.tolist(), ys.tolist()))
        losses.append(float(ref.loss))
    res = m.validate(batches).result()
    m.check_status()
    assert res.batch_metrics == tuples
    assert res.metrics == tuple(float(np.mean([t[j] for t in tuples])) for j in range(17))
    assert np.abs(res.losses - np.array(losses)).max() <= TOL
    assert list(res.sizes) == [6, 3, 3]


def test_two_runs_are_bitwise_equal():
    c = R.case("pheme")
    m = _model("pheme")
    x, root = _x(c), c.rootindex.to(DEV)
    a = m.forward_batch(x, root, max_len=c.max_len, return_states=True)
    b = m.forward_batch(x, root, max_len=c.max_len, return_states=True)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def _bad(c, kind):
    root, y, max_len = c.rootindex.clone(), c.y.clone(), c.max_len
    if kind == "not_increasing":
        root[2] = root[1]
    elif kind == "start_past_the_end":
        root[-1] = c.N
    elif kind == "label_out_of_range":
        y[1] = c.cfg["out"]
    elif kind == "max_len_one_short":
        max_len = c.max_len - 1
    return SimpleNamespace(cls=_x(c), rootindex=root.to(DEV), y=y.to(DEV)), max_len


@pytest.mark.parametrize("kind", ["not_increasing", "start_past_the_end", "label_out_of_range", "max_len_one_short"])
def test_invalid_batches_are_flagged_and_leave_the_model_usable(kind):
    """The call itself returns normally and stays in bounds (bounds handling on the device: every
    sequence of a batch with a bad start or a short max_len is emptied); check_status raises; a
    following valid batch evaluates correctly."""
    c = R.case("boundaries")
    m = _model("boundaries")
    data, max_len = _bad(c, kind)
    loss, correct, pred = m.evaluate(data, pred=True, max_len=max_len)
    assert bool(torch.isfinite(loss))
    with pytest.raises(IndexError):
        m.check_status()
    m.check_status()   # cleared
    logp = torch.empty(c.B, c.cfg["out"], device=DEV)
    m.evaluate(_data(c), logp=logp, max_len=c.max_len)
    m.check_status()
    assert _err(logp, c.ref.logp) <= TOL
