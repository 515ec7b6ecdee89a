"""GPU checks of the LSTM baseline's training path: bgcn_lstm_train_grad (LSTM.grad_batch) against the
fp64 autograd restatement of the reference loop (tests/lstm_train_ref.py), properties that hold bit
for bit by construction, the structure of the backward, validity decided on the device, and
LSTMTrainStep against grad_batch + MultiAdam and against the reference loop with torch.optim.Adam.

Bar: 1e-4 in the metric max|got - ref| / max|ref| per gradient tensor (loss, logp: 1e-4 absolute);
tests/test_lstm_train.py shows torch's own fp32 autograd at least 10x under it on every case.  With
BGCN_LSTM_TRAIN_PARITY_OUT set, the parity test's records go to that path
(profiles/lstm_train_parity.json is such a record).

None of the invalid batches reads or writes out of bounds: a flagged batch is emptied by the call."""
import ctypes
import functools
import json
import os
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import lstm_ref as R
import lstm_train_ref as T
import lstm_gpu_util as U
from lstm_gpu_util import DEV, _buf, _data, _ends, _x

pytestmark = pytest.mark.gpu

_parity = {}


def _new_model(c, train=True):
    return U._new_model(c, train=train)


@functools.lru_cache(maxsize=None)
def _model(name):
    return _new_model(T.case(name))


def _same_grads(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k


# ---------------------------------------------------------------- parity
@pytest.mark.parametrize("name", T.PARITY_CASES)
def test_gradients_match_the_fp64_autograd_loop(name):
    c = T.case(name)
    want = T.oracle(name)
    m = _new_model(c)   # not kept: t_largest holds about 340 MB of weights
    loss, correct, g = m.grad_batch(_x(c), c.rootindex.to(DEV), c.y.to(DEV), max_len=c.max_len, dx=True)
    m.check_status()
    assert sorted(g) == sorted(want.grads)
    errs = {k: T.rel_err(g[k], want.grads[k]) for k in want.grads}
    errs_abs = {"loss": abs(float(loss) - float(want.loss))}
    worst = max(errs.values())
    print(name, {k: f"{v:.2e}" for k, v in errs.items()}, errs_abs)
    _parity[name] = {"N": c.N, "B": c.B, "in_feats": c.cfg["in_feats"], "hid": c.cfg["hid"],
                     "layers": c.cfg["layers"], "out_feats": c.cfg["out"], "weight_factor": c.weight_factor,
                     "rel_err": errs, "loss_abs_err": errs_abs["loss"], "bar": T.BAR,
                     "margin": T.BAR / max(worst, errs_abs["loss"], 1e-30)}
    path = os.environ.get("BGCN_LSTM_TRAIN_PARITY_OUT")
    if path:
        with open(path, "w") as f:
            json.dump(_parity, f, indent=1, sort_keys=True)
    for k, e in errs.items():
        assert e <= T.BAR, (k, e)
    assert errs_abs["loss"] <= T.BAR
    assert int(correct) == int(c.ref.pred.eq(c.y).sum()) or not bool(R.margin_ok(c.ref.logp).all())
    assert g["x"].shape == (c.N, c.cfg["in_feats"])
    first = int(c.rootindex[0])
    if first:
        assert float(g["x"][:first].abs().sum()) == 0.0   # rows of no tree
    if name == "t_rows_over_switch":
        assert c.N >= 8192
    if name == "t_one_class":
        assert all(float(v.abs().max()) == 0.0 for v in g.values())   # softmax = 1: dz = 0


# ---------------------------------------------------------------- the C ABI, called directly
def _states(c, bufs):
    """Host copies of the caller's ``out [N, 2H]`` and ``h_n [2L, B, H]``."""
    H, L = c.cfg["hid"], c.cfg["layers"]
    return (bufs["out"].view(torch.float32)[:c.N * 2 * H].view(c.N, 2 * H).cpu(),
            bufs["h_n"].view(torch.float32)[:2 * L * c.B * H].view(2 * L, c.B, H).cpu())


def _eval_states(name):
    """``(out, h_n)`` of one bgcn_lstm_eval call on the case, both pre-filled with 0xFF bytes."""
    from bigcn_amd import _lib
    lib = _lib.lib()
    c = T.case(name)
    H, L = c.cfg["hid"], c.cfg["layers"]
    x, root, y = _x(c), c.rootindex.to(DEV), c.y.to(DEV)
    ws = _buf(lib.bgcn_lstm_workspace_size(c.N, c.B, c.cfg["in_feats"], H, L), "ff")
    bufs = {"logp": _buf(4 * c.B * c.cfg["out"], "ff"), "status": _buf(4, "ff"),
            "out": _buf(4 * c.N * 2 * H, "ff"), "h_n": _buf(4 * 2 * L * c.B * H, "ff")}
    a = _lib.LstmArgs()
    U._fwd_args(a, c, U._weights(name, T.case), x, root)
    a.y, a.logp, a.status = y.data_ptr(), bufs["logp"].data_ptr(), bufs["status"].data_ptr()
    a.out, a.h_n = bufs["out"].data_ptr(), bufs["h_n"].data_ptr()
    rc = lib.bgcn_lstm_eval(ctypes.addressof(a), ws.data_ptr(), ws.numel(), _lib.stream_handle())
    assert rc == 0, lib.bgcn_last_error()
    torch.cuda.synchronize()
    assert int(bufs["status"].view(torch.int32)[0]) == 0
    return _states(c, bufs)


def _capi(name, fill="zero", rootindex=None, y=None, max_len=None, states=False):
    """One bgcn_lstm_train_grad call on a workspace, outputs and gradient buffers all pre-filled with
    ``fill``.  Returns host copies of every output, the status word and the skip flag.  ``states``: the
    call also gets the caller's ``out`` and ``h_n`` (else NULL)."""
    from bigcn_amd import _lib
    lib = _lib.lib()
    c = T.case(name)
    w = U._weights(name, T.case)
    H, L, C, N, B, Fin = c.cfg["hid"], c.cfg["layers"], c.cfg["out"], c.N, c.B, c.cfg["in_feats"]
    x = _x(c)
    root = (c.rootindex if rootindex is None else rootindex).to(DEV)
    yy = (c.y if y is None else y).to(DEV)
    need = lib.bgcn_lstm_train_workspace_size(N, B, Fin, H, L)
    assert need > 0
    ws = _buf(need, fill)
    bufs = {"logp": _buf(4 * B * C, fill), "status": _buf(4, fill), "loss": _buf(4, fill), "correct": _buf(4, fill),
            "pred": _buf(8 * B, fill), "skip_flag": _buf(4, fill), "x": _buf(4 * N * x.stride(0), fill)}
    shapes = {k: tuple(v.shape) for k, v in w.items()}
    for k, shp in shapes.items():
        bufs[k] = _buf(4 * int(torch.tensor(shp).prod()), fill)
    t = _lib.LstmTrainArgs()
    a = t.fwd
    U._fwd_args(a, c, w, x, root, max_len)
    for l in range(L):
        for d in range(2):
            rev = "_reverse" if d else ""
            t.d_w_ih[l][d] = bufs[f"lstm.weight_ih_l{l}{rev}"].data_ptr()
            t.d_w_hh[l][d] = bufs[f"lstm.weight_hh_l{l}{rev}"].data_ptr()
    a.y, a.logp, a.status = yy.data_ptr(), bufs["logp"].data_ptr(), bufs["status"].data_ptr()
    if states:
        bufs.update(out=_buf(4 * N * 2 * H, fill), h_n=_buf(4 * 2 * L * B * H, fill))
        a.out, a.h_n = bufs["out"].data_ptr(), bufs["h_n"].data_ptr()
    a.loss, a.correct, a.pred = bufs["loss"].data_ptr(), bufs["correct"].data_ptr(), bufs["pred"].data_ptr()
    t.d_fc_w, t.d_fc_b = bufs["fc.weight"].data_ptr(), bufs["fc.bias"].data_ptr()
    t.dx, t.skip_flag = bufs["x"].data_ptr(), bufs["skip_flag"].data_ptr()
    rc = lib.bgcn_lstm_train_grad(ctypes.addressof(t), ws.data_ptr(), ws.numel(), _lib.stream_handle())
    assert rc == 0, lib.bgcn_last_error()
    torch.cuda.synchronize()
    r = SimpleNamespace(status=int(bufs["status"].view(torch.int32)[0]),
                        skip_flag=float(bufs["skip_flag"].view(torch.float32)[0]),
                        logp=bufs["logp"].view(torch.float32)[:B * C].view(B, C).cpu(),
                        loss=bufs["loss"].view(torch.float32)[:1].cpu(),
                        correct=bufs["correct"].view(torch.int32)[:1].cpu(),
                        pred=bufs["pred"].view(torch.int64)[:B].cpu(), grads={})
    for k, shp in shapes.items():
        n = int(torch.tensor(shp).prod())
        r.grads[k] = bufs[k].view(torch.float32)[:n].view(shp).cpu()
    r.grads["x"] = bufs["x"].view(torch.float32)[:N * x.stride(0)].view(N, x.stride(0))[:, :Fin].cpu()
    if states:
        r.out, r.h_n = _states(c, bufs)
    return r


@functools.lru_cache(maxsize=None)
def _full(name):
    r = _capi(name, "zero")
    assert r.status == 0 and r.skip_flag == 0.0
    want = T.oracle(name)
    for k, g in want.grads.items():
        assert T.rel_err(r.grads[k], g) <= T.BAR, k
    return r


# ---------------------------------------------------------------- held bit for bit
@pytest.mark.parametrize("name", ["boundaries", "three_layers", "offset_strided", "t_many_trees"])
def test_the_training_forward_has_the_bits_of_evaluate(name):
    """One forward (lstm_forward and its kernels) serves both entry points.  include/bgcn.h also
    promises bgcn_lstm_eval's bits in the training call's optional ``out`` and ``h_n``: with ``out`` the
    last layer's output lives in the caller's buffer, which the backward then reads, so the gradients of
    that call must be the bits of the call without it."""
    c = T.case(name)
    r = _full(name)
    m = _new_model(c, train=False)
    logp = torch.empty(c.B, c.cfg["out"], device=DEV)
    loss, correct, pred = m.evaluate(_data(c), logp=logp, pred=True, max_len=c.max_len)
    m.check_status()
    assert torch.equal(r.logp, logp.cpu())
    assert torch.equal(r.loss[0], loss.cpu()) and int(r.correct) == int(correct)
    assert torch.equal(r.pred, pred.cpu())
    assert abs(float(loss) - float(c.ref.loss)) <= T.BAR
    # and through the module
    loss2, correct2, _ = _model(name).grad_batch(_x(c), c.rootindex.to(DEV), c.y.to(DEV), max_len=c.max_len)
    assert torch.equal(loss2, loss) and torch.equal(correct2, correct)
    # the caller's out and h_n, pre-filled with 0xFF bytes
    got = _capi(name, "ff", states=True)
    out, h_n = _eval_states(name)
    assert got.status == 0 and got.skip_flag == 0.0
    assert torch.equal(got.out, out) and torch.equal(got.h_n, h_n)
    first = int(c.rootindex[0])
    assert float(got.out[:first].abs().sum()) == 0.0   # offset_strided: the rows above the first tree
    _same_grads(got.grads, r.grads)


@pytest.mark.parametrize("name", ["boundaries", "t_rows_over_switch"])
def test_two_runs_give_the_same_bits(name):
    c = T.case(name)
    m = _model(name)
    a = m.grad_batch(_x(c), c.rootindex.to(DEV), c.y.to(DEV), max_len=c.max_len, dx=True)
    b = m.grad_batch(_x(c), c.rootindex.to(DEV), c.y.to(DEV), max_len=c.max_len, dx=True)
    m.check_status()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    _same_grads(a[2], b[2])
    assert a[2]["fc.weight"].data_ptr() != b[2]["fc.weight"].data_ptr()


@pytest.mark.parametrize("fill", ["ff", "big"])
@pytest.mark.parametrize("name", ["boundaries", "three_layers", "offset_strided"])
def test_results_do_not_depend_on_what_the_buffers_held(name, fill):
    """The workspace, the outputs and every gradient buffer of 0xFF bytes (NaN as fp32) or of 3.0e38
    give the bits of zeroed ones: nothing is read before it is written, nothing is accumulated into
    what the caller passed, the dc carry and the recurrent product are not read at a tree's last step,
    c_prev is not read at its first, and the rows above the first start are zeroed by the call."""
    want = _full(name)
    got = _capi(name, fill)
    assert got.status == 0 and got.skip_flag == 0.0
    for k in ("logp", "loss", "correct", "pred"):
        assert torch.equal(getattr(got, k), getattr(want, k)), k
    _same_grads(got.grads, want.grads)


def test_a_small_batch_after_a_large_one_on_one_module():
    c = T.case("boundaries")
    g = torch.Generator().manual_seed(78)
    lengths = [1 + b % 3 for b in range(300)]
    bx = torch.randn(sum(lengths), c.cfg["in_feats"], generator=g).to(DEV)
    broot = torch.tensor([0] + lengths[:-1]).cumsum(0).to(DEV)
    by = torch.randint(0, 4, (300,), generator=g).to(DEV)
    used, fresh = _new_model(c), _new_model(c)
    loss, _, _ = used.grad_batch(bx, broot, by, max_len=3, dx=True)
    used.check_status()
    assert bool(torch.isfinite(loss))
    ws_before = used.__dict__["_state"]["tws"]
    res = [m.grad_batch(_x(c), c.rootindex.to(DEV), c.y.to(DEV), max_len=c.max_len, dx=True) for m in (used, fresh)]
    assert used.__dict__["_state"]["tws"] is ws_before
    assert used.__dict__["_state"]["tws"].numel() > fresh.__dict__["_state"]["tws"].numel()
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    _same_grads(res[0][2], res[1][2])


def test_a_trees_dx_does_not_depend_on_its_neighbours():
    """Below the GEMM row switch a row of every GEMM is an independent k-ordered chain, a tree is one
    MFMA column of the steps, and the head works per tree.  The C ABI has no loss seed, so tree b
    alone is a batch of B copies of it: every copy's dz carries the same 1 / B, and each copy's rows
    of dx have the bits of the tree's rows in the mixed batch."""
    c = T.case("boundaries")
    m = _model("boundaries")
    x = _x(c)
    _, _, g = m.grad_batch(x, c.rootindex.to(DEV), c.y.to(DEV), max_len=c.max_len, dx=True)
    for b, (s, e) in enumerate(_ends(c)):
        n = e - s
        xs = x[s:e].repeat(c.B, 1)
        root = (torch.arange(c.B) * n).to(DEV)
        y = c.y[b].repeat(c.B).to(DEV)
        _, _, g1 = m.grad_batch(xs, root, y, max_len=n, dx=True)
        for k in range(c.B):
            assert torch.equal(g1["x"][k * n:(k + 1) * n], g["x"][s:e]), (b, k)
    m.check_status()


def test_more_step_launches_than_needed_change_nothing():
    c = T.case("boundaries")
    m = _model("boundaries")
    x, root, y = _x(c), c.rootindex.to(DEV), c.y.to(DEV)
    want = m.grad_batch(x, root, y, max_len=c.max_len, dx=True)
    for max_len in (c.max_len + 1, 3 * c.max_len):
        got = m.grad_batch(x, root, y, max_len=max_len, dx=True)
        assert torch.equal(got[0], want[0])
        _same_grads(got[2], want[2])
    got = m.grad_batch(x, root, y, dx=True)   # max_len read from rootindex
    _same_grads(got[2], want[2])
    m.check_status()


# ---------------------------------------------------------------- structure
def test_a_tree_of_one_row_feeds_both_directions():
    """One tree of one row, one layer: d h_n enters dY at the same row in both column halves, so both
    directions' input weights get a gradient, and no recurrent weight does (h_prev = 0)."""
    c = T.case("one_layer")
    assert _ends(c)[0] == (0, 1)
    lstm, fc, params = T._build(c, torch.float64)
    x = c.x[:1].double().clone().requires_grad_(True)
    _, loss = T._loop(lstm, fc, x, [(0, 1)], c.y[:1])
    loss.backward()
    m = _model("one_layer")
    got_loss, _, g = m.grad_batch(c.x[:1].float().to(DEV), torch.zeros(1, dtype=torch.int64, device=DEV),
                                  c.y[:1].to(DEV), max_len=1, dx=True)
    m.check_status()
    assert abs(float(got_loss) - float(loss)) <= T.BAR
    for k in ("lstm.weight_ih_l0", "lstm.weight_ih_l0_reverse", "fc.weight", "fc.bias"):
        assert float(params[k].grad.abs().max()) > 0
        assert T.rel_err(g[k], params[k].grad) <= T.BAR, k
    assert T.rel_err(g["x"], x.grad) <= T.BAR
    for k in ("lstm.weight_hh_l0", "lstm.weight_hh_l0_reverse"):
        assert float(g[k].abs().max()) == 0.0, k


def test_permuting_the_trees_keeps_every_weight_gradient():
    """tile_plus_one with its 33 trees permuted: the mean loss is the same function of the weights.  Not
    bitwise (the weight-gradient GEMMs sum over the rows in another order): within the parity bar."""
    c = T.case("tile_plus_one")
    want = T.oracle("tile_plus_one")
    m = _model("tile_plus_one")
    x = _x(c)
    order = torch.randperm(c.B, generator=torch.Generator().manual_seed(3)).tolist()
    ends = _ends(c)
    xp = torch.cat([x[ends[o][0]:ends[o][1]] for o in order])
    lens = [ends[o][1] - ends[o][0] for o in order]
    rootp = torch.tensor([0] + lens[:-1]).cumsum(0)
    assert not torch.equal(rootp, c.rootindex)
    loss, _, g = m.grad_batch(xp, rootp.to(DEV), c.y[order].to(DEV), max_len=c.max_len, dx=True)
    m.check_status()
    assert abs(float(loss) - float(want.loss)) <= T.BAR
    for k, ref in want.grads.items():
        if k != "x":
            assert T.rel_err(g[k], ref) <= T.BAR, k
    back = torch.cat([want.grads["x"][ends[o][0]:ends[o][1]] for o in order])
    assert T.rel_err(g["x"], back) <= T.BAR


# ---------------------------------------------------------------- validity on the device
FAULTS = ["start_0_repeats_1", "start_280_repeats_279", "first_start_negative", "last_start_is_N",
          "tree_0_over_max_len", "tree_284_over_max_len", "label_C_at_0", "label_minus_one_at_270"]


def _fault(c, kind):
    root, y, max_len = c.rootindex.clone(), c.y.clone(), c.max_len
    if kind == "start_0_repeats_1":
        root[0] = root[1]
    elif kind == "start_280_repeats_279":
        root[280] = root[279]
    elif kind == "first_start_negative":
        root[0] = -1
    elif kind == "last_start_is_N":
        root[299] = c.N
    elif kind == "tree_0_over_max_len":
        root[1], root[2] = 4, 5
        lens = [e - s for s, e in _ends(c, root)]
        assert lens[0] == 4 and max(lens[1:]) == 3 and min(lens) == 1
    elif kind == "tree_284_over_max_len":
        root[285] += 1
        root[286] += 1
        lens = [e - s for s, e in _ends(c, root)]
        assert max(lens) == 4 and lens.count(4) == 1 and lens[284] == 4 and min(lens) == 1
    elif kind == "label_C_at_0":
        y[0] = c.cfg["out"]
    elif kind == "label_minus_one_at_270":
        y[270] = -1
    else:
        raise KeyError(kind)
    return root, y, max_len


def _snapshot(m, opt):
    return [p.detach().clone() for p in m.parameters()] + [t.clone() for p in opt.params() for t in opt.state[p]]


@pytest.mark.parametrize("kind", FAULTS)
def test_an_invalid_batch_is_flagged_and_skips_the_update(kind):
    """300 trees, the fault at tree 0 or at a tree past 256 (the loops over B take steps of 256).  The
    step returns normally; the status bit and skip_flag are set, no parameter or moment changes, the
    skip count grows by one, check_status raises, and a valid batch afterwards steps normally."""
    from bigcn_amd import LSTMTrainStep, _lib
    c = T.case("t_many_trees")
    m = _new_model(c)
    step = LSTMTrainStep(m)
    step.step(_data(c), max_len=c.max_len)   # a valid step first: the moments are not zero
    assert step.check_status() == 0
    before = _snapshot(m, step.optimizer)
    assert any(float(t.abs().max()) > 0 for t in before[len(list(m.parameters())):])
    root, y, max_len = _fault(c, kind)
    loss, correct = step.step(_data(c, root, y), max_len=max_len)
    assert int(m.__dict__["_state"]["status"]) == _lib.BGCN_STATUS_SEQUENCE
    assert float(step._st["skip_flag"]) == 1.0
    for u, v in zip(_snapshot(m, step.optimizer), before):
        assert torch.equal(u, v)
    assert step.step_count == 2
    with pytest.raises(IndexError, match="1 updates skipped"):
        step.check_status()
    assert step.last_skipped == 1 and step.check_status() == 0
    loss, correct = step.step(_data(c), max_len=c.max_len)
    assert step.check_status() == 0 and float(step._st["skip_flag"]) == 0.0
    assert any(not torch.equal(u, v) for u, v in zip(_snapshot(m, step.optimizer), before))
    assert abs(float(loss) - float(c.ref.loss)) < 0.05   # one update of 5e-4 later
    # through the C ABI on buffers of NaN bits: flagged, and a bad label alone leaves the other trees' loss
    r = _capi("t_many_trees", "ff", rootindex=root, y=y, max_len=max_len)
    assert r.status == _lib.BGCN_STATUS_SEQUENCE and r.skip_flag == 1.0
    if kind.startswith("label"):
        valid = (y >= 0) & (y < c.cfg["out"])
        want = float(F.nll_loss(c.ref.logp[valid], y[valid], reduction="sum")) / c.B
        assert abs(float(r.loss) - want) <= T.BAR
        assert bool(torch.isfinite(r.grads["fc.weight"]).all())


def test_a_bad_label_keeps_no_gradient():
    """One tree, its label out of range: dz = 0, so every gradient of the call is exactly zero."""
    c = T.case("one_layer")
    m = _model("one_layer")
    x = c.x[:4].float().to(DEV)
    root = torch.zeros(1, dtype=torch.int64, device=DEV)
    _, _, g = m.grad_batch(x, root, torch.tensor([4], device=DEV), max_len=4, dx=True)
    with pytest.raises(IndexError):
        m.check_status()
    for k, v in g.items():
        assert float(v.abs().max()) == 0.0, k
    _, _, g = m.grad_batch(x, root, torch.tensor([1], device=DEV), max_len=4, dx=True)
    m.check_status()
    assert float(g["lstm.weight_hh_l0"].abs().max()) > 0


# ---------------------------------------------------------------- the step
def test_the_step_is_grad_batch_then_multi_adam():
    from bigcn_amd import LSTMTrainStep, lstm_adam
    c = T.case("boundaries")
    a, b = _new_model(c), _new_model(c)
    step = LSTMTrainStep(a)
    opt = lstm_adam(b)
    data = _data(c)
    for i in range(3):
        loss, correct, pred = step.step(data, pred=True, max_len=c.max_len)
        loss2, correct2, g = b.grad_batch(data.cls, data.rootindex, data.y, max_len=c.max_len)
        by_id = {id(p): g[n] for n, p in b.named_parameters()}
        opt.step(grads=[by_id[id(p)] for p in opt.params()])
        assert torch.equal(loss, loss2) and torch.equal(correct, correct2), i
        assert int(correct) == int(pred.eq(data.y).sum())
        for (n, p), q in zip(a.named_parameters(), b.parameters()):
            assert torch.equal(p, q), (i, n)
            assert p.grad is None
        for p, q in zip(step.optimizer.params(), opt.params()):
            for u, v in zip(step.optimizer.state[p], opt.state[q]):
                assert torch.equal(u, v), i
    assert step.step_count == 3 and step.check_status() == 0
    assert not torch.equal(a.fc.weight.cpu(), c.sd["fc.weight"].float())


@pytest.mark.parametrize("name", ["boundaries", "one_layer"])
def test_five_steps_follow_the_reference_loop(name):
    from bigcn_amd import LSTMTrainStep
    c = T.case(name)
    want = T.train_losses(c, 5, torch.float64)
    step = LSTMTrainStep(_new_model(c), lr=T.LR, weight_decay=T.WEIGHT_DECAY)
    data = _data(c)
    got = [step.step(data, max_len=c.max_len)[0] for _ in range(5)]
    got = [float(v) for v in got]
    assert step.check_status() == 0
    print(name, got, want)
    for u, v in zip(got, want):
        assert abs(u - v) <= T.BAR
    assert want[4] < want[0]
