"""GPU checks of the TreeBERT baseline's training path: bgcn_bert_train_grad (TreeBERT.grad_batch)
against the fp64 autograd restatement of the reference loop (tests/bert_train_ref.py: one
full-sequence causal encoder call per tree with all four dropout sites), properties that hold bit for
bit by construction, the C ABI called directly, validity decided on the device, and
TreeBERTTrainStep against grad_batch + bert_adam and against the reference loop with
torch.optim.Adam.

Bar: 1e-4 in the metric max|got - ref| / max|ref| per gradient tensor (loss, logp: 1e-4 absolute), the
project's gradient bar; tests/test_bert_train.py shows torch's own fp32 autograd at least 10x under
it on every case.  An all-zero reference demands exact zeros.  With BGCN_BERT_TRAIN_PARITY_OUT set,
the parity test's records go to that path (profiles/bert_train_parity.json is such a record).

None of the invalid batches reads or writes out of bounds: a flagged batch is emptied by the call."""
import ctypes
import functools
import json
import os
from types import SimpleNamespace

import pytest
import torch

import bert_ref as R
import bert_train_ref as T

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
_parity = {}


def _new_model(c):
    return R.model_for(c, DEV)


@functools.lru_cache(maxsize=None)
def _model(name):
    return _new_model(T.case(name))


def _x(c):
    wide = c.x._base if c.x._base is not None else c.x
    return wide.to(DEV)[:, :c.cfg["hidden"]]       # the case's row stride survives the copy


def _data(c, x=None, rootindex=None, y=None):
    """A PyG-like batch whose ``x [N, 2 * hidden]`` max-pools over the middle axis to the case's rows."""
    x = _x(c) if x is None else x
    g = torch.Generator().manual_seed(5)
    lower = x - torch.rand(x.size(0), x.size(1), generator=g).to(DEV)
    return SimpleNamespace(x=torch.cat((lower, x), 1).contiguous(),
                           rootindex=(c.rootindex if rootindex is None else rootindex).to(DEV),
                           y=(c.y if y is None else y).to(DEV))


def _grad(m, c, drop, seed=T.DROP_SEED, x=None, dx=True):
    p_h, p_a = T.DROPS[drop]
    return m.grad_batch(_x(c) if x is None else x, c.rootindex.to(DEV), c.y.to(DEV), dx=dx, drop_seed=seed,
                        hidden_dropout=p_h, attn_dropout=p_a)


def _same_grads(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k


# ---------------------------------------------------------------- parity
@pytest.mark.parametrize("name,drop", T.PARITY)
def test_gradients_match_the_fp64_autograd_loop(name, drop):
    c = T.case(name)
    want = T.oracle(name, drop)
    m = _model(name)
    p_h, p_a = T.DROPS[drop]
    r = m._train(_x(c), c.rootindex.to(DEV), c.y.to(DEV), dx=True, drop_seed=T.DROP_SEED, hidden_dropout=p_h,
                 attn_dropout=p_a)
    loss, correct, g = _grad(m, c, drop)
    m.check_status()
    assert torch.equal(r["loss"].view(()), loss)
    assert sorted(g) == sorted(want.grads) and not any("word_embeddings" in k for k in g)
    errs = {k: T.rel_err(g[k], want.grads[k]) for k in want.grads}
    errs_abs = {"loss": abs(float(loss) - float(want.loss)),
                "logp": float((r["logp"].double().cpu() - want.logp).abs().max())}
    worst = max(errs.values())
    print(name, drop, max(errs, key=errs.get), f"{worst:.2e}", errs_abs)
    _parity[f"{name}/{drop}"] = {
        "N": c.N, "B": c.B, "hidden": c.cfg["hidden"], "intermediate": c.cfg["intermediate"],
        "layers": c.cfg["layers"], "out_feats": c.cfg["out"], "hidden_dropout": p_h, "attn_dropout": p_a,
        "worst_rel_err": worst, "worst_tensor": max(errs, key=errs.get), "loss_abs_err": errs_abs["loss"],
        "logp_abs_err": errs_abs["logp"], "bar": T.BAR, "margin": T.BAR / max(worst, max(errs_abs.values()), 1e-30)}
    path = os.environ.get("BGCN_BERT_TRAIN_PARITY_OUT")
    if path:
        with open(path, "w") as f:
            json.dump(_parity, f, indent=1, sort_keys=True)
    for k, e in errs.items():
        assert e <= T.BAR, (k, e)
    assert errs_abs["loss"] <= T.BAR and errs_abs["logp"] <= T.BAR
    if R.pred_gap(want.logp) > 2 * T.BAR:
        assert int(correct) == int(want.pred.eq(c.y).sum())
    assert g["x"].shape == (c.N, c.cfg["hidden"])
    if name == "t_rows_over_switch":
        assert c.B >= 8192
    if name == "t_classes_1":
        assert all(float(v.abs().max()) == 0.0 for v in g.values())   # softmax = 1: dz = 0


# ---------------------------------------------------------------- the C ABI, called directly
def _buf(nbytes, fill):
    b = torch.empty((max(int(nbytes), 16) + 15) // 16 * 16, dtype=torch.uint8, device=DEV)
    return b.zero_() if fill == "zero" else b.fill_(0xFF)


def _capi(name, fill="zero", drop="p01", rootindex=None, y=None, ws_short=0, rates=None, x=None):
    """One bgcn_bert_train_grad call on a workspace, outputs and gradient buffers all pre-filled with
    ``fill`` (zero bytes, or 0xFF bytes: NaN as fp32).  Returns host copies of every output, the status
    word and the skip flag, or the error code when the call is refused."""
    from bigcn_amd import _lib
    from bigcn_amd.bert import _LAYER_FIELDS, _TOP_FIELDS, LN_EPS
    lib = _lib.lib()
    c = T.case(name)
    cfg = c.cfg
    w = {k: v.float().contiguous().to(DEV) for k, v in c.sd.items()}
    H, L, C = cfg["hidden"], cfg["layers"], cfg["out"]
    x = _x(c) if x is None else x
    N = x.size(0)
    root = (c.rootindex if rootindex is None else rootindex).to(DEV)
    B = root.numel()
    yy = (c.y if y is None else y).to(DEV)
    need = lib.bgcn_bert_train_workspace_size(N, B, H, cfg["intermediate"], L)
    assert need > 0 and need % 256 == 0
    ws = _buf(need, fill)
    bufs = {"logp": _buf(4 * B * C, fill), "status": _buf(4, fill), "loss": _buf(4, fill), "correct": _buf(4, fill),
            "pred": _buf(8 * B, fill), "skip_flag": _buf(4, fill), "x": _buf(4 * N * x.stride(0), fill)}
    names = T.grad_names(c)
    for k in names:
        bufs[k] = _buf(4 * w[k].numel(), fill)
    t = _lib.BertTrainArgs()
    a = t.fwd
    a.x, a.ldx, a.num_nodes, a.seq_start, a.num_seqs = x.data_ptr(), x.stride(0), N, root.data_ptr(), B
    a.hidden, a.heads, a.intermediate, a.num_layers = H, c.heads, cfg["intermediate"], L
    a.max_pos, a.out_feats, a.ln_eps = cfg["max_pos"], C, LN_EPS
    for field, key in _TOP_FIELDS:
        setattr(a, field, w[key].data_ptr())
        setattr(t, "d_" + field, bufs[key].data_ptr())
    for i in range(L):
        for field, key in _LAYER_FIELDS:
            setattr(a.layer[i], field, w[f"BERT.encoder.layer.{i}.{key}"].data_ptr())
            setattr(t.d_layer[i], field, bufs[f"BERT.encoder.layer.{i}.{key}"].data_ptr())
    a.y, a.logp, a.status = yy.data_ptr(), bufs["logp"].data_ptr(), bufs["status"].data_ptr()
    a.loss, a.correct, a.pred = bufs["loss"].data_ptr(), bufs["correct"].data_ptr(), bufs["pred"].data_ptr()
    t.dx, t.skip_flag, t.drop_seed = bufs["x"].data_ptr(), bufs["skip_flag"].data_ptr(), T.DROP_SEED
    t.hidden_dropout, t.attn_dropout = T.DROPS[drop] if rates is None else rates
    rc = lib.bgcn_bert_train_grad(ctypes.addressof(t), ws.data_ptr(), need - ws_short, _lib.stream_handle())
    if rc != 0:
        return rc
    torch.cuda.synchronize()
    r = SimpleNamespace(status=int(bufs["status"].view(torch.int32)[0]),
                        skip_flag=float(bufs["skip_flag"].view(torch.float32)[0]),
                        logp=bufs["logp"].view(torch.float32)[:B * C].view(B, C).cpu(),
                        loss=bufs["loss"].view(torch.float32)[:1].cpu(),
                        correct=bufs["correct"].view(torch.int32)[:1].cpu(),
                        pred=bufs["pred"].view(torch.int64)[:B].cpu(), grads={})
    for k in names:
        r.grads[k] = bufs[k].view(torch.float32)[:w[k].numel()].view(w[k].shape).cpu()
    r.grads["x"] = bufs["x"].view(torch.float32)[:N * x.stride(0)].view(N, x.stride(0))[:, :H].cpu()
    return r


@pytest.mark.parametrize("name,drop", [("t_boundaries", "p01"), ("t_boundaries", "p0"), ("t_single", "p01"),
                                       ("t_many_trees", "p01")])
def test_results_do_not_depend_on_what_the_buffers_held(name, drop):
    """The workspace, the outputs and every gradient buffer of 0xFF bytes (NaN as fp32) give the bits of
    zeroed ones: every buffer is written whole, nothing is read before it is written, nothing is
    accumulated into what the caller passed."""
    want = _capi(name, "zero", drop)
    got = _capi(name, "ff", drop)
    ref = T.oracle(name, drop)
    assert want.status == 0 and want.skip_flag == 0.0 and got.status == 0 and got.skip_flag == 0.0
    for k in ("logp", "loss", "correct", "pred"):
        assert torch.equal(getattr(got, k), getattr(want, k)), k
    _same_grads(got.grads, want.grads)
    for k, g in ref.grads.items():
        assert T.rel_err(want.grads[k], g) <= T.BAR, k


def test_a_short_workspace_and_a_bad_rate_are_refused():
    from bigcn_amd import _lib
    assert _capi("t_boundaries", ws_short=256) == -1
    assert "workspace too small" in _lib.lib().bgcn_last_error().decode()
    for rates in ((1.0, 0.1), (0.1, 1.0), (-0.1, 0.1), (0.1, -0.1), (float("nan"), 0.0)):
        assert _capi("t_boundaries", rates=rates) == -1, rates
        assert "dropout rate" in _lib.lib().bgcn_last_error().decode()
    assert _lib.lib().bgcn_bert_train_workspace_size(10, 2, 100, 256, 2) == 0   # hidden % 64
    assert _lib.lib().bgcn_bert_train_workspace_size(10, 2, 128, 256, 25) == 0  # layers


# ---------------------------------------------------------------- held bit for bit
@pytest.mark.parametrize("name", ["t_boundaries", "t_many_trees", "t_classes_63", "t_hidden_320"])
def test_the_training_forward_without_dropout_has_the_bits_of_evaluate(name):
    c = T.case(name)
    r = _capi(name, "ff", "p0")
    m = _model(name)
    logp = torch.empty(c.B, c.cfg["out"], device=DEV)
    loss, correct, pred = m.evaluate(_data(c), logp=logp, pred=True)
    m.check_status()
    assert torch.equal(r.logp, logp.cpu())
    assert torch.equal(r.loss[0], loss.cpu()) and int(r.correct) == int(correct)
    assert torch.equal(r.pred, pred.cpu())
    loss2, correct2, _ = _grad(m, c, "p0", dx=False)   # and through the module
    assert torch.equal(loss2, loss) and torch.equal(correct2, correct)


@pytest.mark.parametrize("name", ["t_boundaries", "t_rows_over_switch"])
def test_the_seed_decides_the_bits(name):
    c = T.case(name)
    m = _model(name)
    a, b = _grad(m, c, "p01"), _grad(m, c, "p01")
    other = _grad(m, c, "p01", seed=T.DROP_SEED + 1)
    m.check_status()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    _same_grads(a[2], b[2])
    assert a[2]["fc.weight"].data_ptr() != b[2]["fc.weight"].data_ptr()   # new tensors on every call
    assert not torch.equal(a[0], other[0])
    assert not torch.equal(a[2]["BERT.pooler.dense.weight"], other[2]["BERT.pooler.dense.weight"])
    assert all(p.grad is None for p in m.parameters())


@pytest.mark.parametrize("drop", ["p0", "p01"])
def test_rows_past_a_trees_first_are_never_read(drop):
    c = T.case("t_boundaries")
    m = _model("t_boundaries")
    want = _grad(m, c, drop)
    x = _x(c).clone()
    other = torch.ones(c.N, dtype=torch.bool)
    other[c.rootindex] = False
    x[other.to(DEV)] = float("nan")
    got = _grad(m, c, drop, x=x)
    m.check_status()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    _same_grads(got[2], want[2])
    assert float(got[2]["x"][other.to(DEV)].abs().max()) == 0.0


def test_permuting_the_trees_permutes_logp_exactly_without_dropout():
    """Below the GEMMs' row switch a row of every GEMM is an independent k-ordered chain and every row
    kernel works per row, so a tree's logp does not depend on its place in the batch."""
    c = T.case("t_boundaries")
    m = _model("t_boundaries")
    x = _x(c)
    kw = dict(hidden_dropout=0.0, attn_dropout=0.0)
    want = m._train(x, c.rootindex.to(DEV), c.y.to(DEV), **kw)["logp"]
    order = [3, 0, 4, 2, 1]
    ends = c.rootindex.tolist()[1:] + [c.N]
    spans = [(int(c.rootindex[o]), ends[o]) for o in order]
    xp = torch.cat([x[s:e] for s, e in spans]).contiguous()
    lens = [e - s for s, e in spans]
    rootp = torch.tensor([0] + lens[:-1]).cumsum(0)
    got = m._train(xp, rootp.to(DEV), c.y[order].to(DEV), **kw)["logp"]
    m.check_status()
    assert torch.equal(got, want[order])


# ---------------------------------------------------------------- validity on the device
FAULTS = ["start_repeats", "tree_over_max_pos", "label_C"]


def _fault(c, kind):
    """(x, rootindex, y) of an invalid batch built on the case's model sizes."""
    x, root, y = _x(c), c.rootindex.clone(), c.y.clone()
    if kind == "start_repeats":
        root[280] = root[279]
    elif kind == "tree_over_max_pos":
        n = c.cfg["max_pos"] + 1
        x = torch.randn(n + 2, c.cfg["hidden"], generator=torch.Generator().manual_seed(4)).to(DEV)
        root, y = torch.tensor([0, n, n + 1]), c.y[:3].clone()   # lengths max_pos + 1, 1, 1
    elif kind == "label_C":
        y[270] = c.cfg["out"]
    else:
        raise KeyError(kind)
    return x, root, y


def _snapshot(m, opt):
    return [p.detach().clone() for p in m.parameters()] + [t.clone() for ch in opt.chunks for p in ch.params()
                                                           for t in ch.state[p]]


@pytest.mark.parametrize("kind", FAULTS)
def test_an_invalid_batch_is_flagged_and_skips_the_update(kind):
    """The step returns normally; the status bit and skip_flag are set, no parameter or moment changes,
    the skip count grows by one, check_status raises, and a valid batch afterwards steps normally."""
    from bigcn_amd import TreeBERTTrainStep, _lib
    c = T.case("t_many_trees")
    m = _new_model(c)
    step = TreeBERTTrainStep(m, drop_seed=11)
    step.step(_data(c))   # a valid step first: the moments are not zero
    assert step.check_status() == 0
    before = _snapshot(m, step.optimizer)
    n_par = len(list(m.parameters()))
    assert any(float(t.abs().max()) > 0 for t in before[n_par:])
    x, root, y = _fault(c, kind)
    loss, correct = step.step(_data(c, x, root, y))
    assert int(m.__dict__["_state"]["status"]) == _lib.BGCN_STATUS_SEQUENCE
    assert float(step._st["skip_flag"]) == 1.0
    for u, v in zip(_snapshot(m, step.optimizer), before):
        assert torch.equal(u, v)
    assert step.step_count == 2
    with pytest.raises(IndexError, match="1 updates skipped"):
        step.check_status()
    assert step.last_skipped == 1 and step.check_status() == 0
    loss, correct = step.step(_data(c))
    assert step.check_status() == 0 and float(step._st["skip_flag"]) == 0.0
    assert bool(torch.isfinite(loss))
    assert any(not torch.equal(u, v) for u, v in zip(_snapshot(m, step.optimizer), before))
    # through the C ABI on buffers of NaN bits: flagged, and every gradient buffer written whole
    r = _capi("t_many_trees", "ff", rootindex=root, y=y, x=x)
    assert r.status == _lib.BGCN_STATUS_SEQUENCE and r.skip_flag == 1.0
    for k, v in r.grads.items():
        assert bool(torch.isfinite(v).all()), k


# ---------------------------------------------------------------- the step
def test_the_step_is_grad_batch_then_bert_adam_and_follows_the_reference_loop():
    from bigcn_amd import TreeBERTTrainStep, bert_adam
    c = T.case("t_boundaries")
    a, b = _new_model(c), _new_model(c)
    for m in (a, b):
        m.hidden_dropout = m.attn_dropout = 0.1
    step = TreeBERTTrainStep(a, lr=T.LR, weight_decay=T.WEIGHT_DECAY, drop_seed=T.DROP_SEED)
    opt = bert_adam(b, lr=T.LR, weight_decay=T.WEIGHT_DECAY)
    want, _ = T.train_losses(c, 3, torch.float64, 0.1, 0.1)
    data = _data(c)
    rows = b._root_rows(data)
    word = "BERT.embeddings.word_embeddings.weight"
    got = []
    for i in range(3):
        loss, correct, pred = step.step(data, pred=True)
        assert step.last_drop_seed == T.DROP_SEED + i
        loss2, correct2, g = b.grad_batch(rows, data.rootindex, data.y, drop_seed=T.DROP_SEED + i)
        by_id = {id(p): g.get(n) for n, p in b.named_parameters()}
        assert by_id[id(dict(b.named_parameters())[word])] is None
        opt.step(grads=[by_id[id(p)] for p in opt.params()])
        assert torch.equal(loss, loss2) and torch.equal(correct, correct2), i
        assert int(correct) == int(pred.eq(data.y).sum())
        for (n, p), q in zip(a.named_parameters(), b.parameters()):
            assert torch.equal(p, q), (i, n)
            assert p.grad is None
        got.append(float(loss))
    for p, q in zip(step.optimizer.params(), opt.params()):
        sa = next(ch.state[p] for ch in step.optimizer.chunks if p in ch.state)
        sb = next(ch.state[q] for ch in opt.chunks if q in ch.state)
        for u, v in zip(sa, sb):
            assert torch.equal(u, v)
    assert step.step_count == 3 and step.check_status() == 0
    print(got, want)
    for u, v in zip(got, want):
        assert abs(u - v) <= T.BAR
    sd = a.state_dict()
    assert torch.equal(sd[word].cpu(), c.sd[word])
    assert not torch.equal(sd["fc.weight"].cpu(), c.sd["fc.weight"])
    # the query / key tensors get zero gradients, not None: weight decay alone moves them, as torch's Adam does
    for k in ("BERT.encoder.layer.1.attention.self.query.weight", "BERT.encoder.layer.0.attention.self.key.bias"):
        p = c.sd[k].clone().requires_grad_(True)
        ref = torch.optim.Adam([p], lr=T.LR, weight_decay=T.WEIGHT_DECAY)
        for _ in range(3):
            p.grad = torch.zeros_like(p)
            ref.step()
        assert not torch.equal(sd[k].cpu(), c.sd[k])
        assert float((sd[k].cpu() - p.detach()).abs().max()) <= 1e-6   # fp32 Adam twice: a few ulps of values below 1


def test_the_chunked_optimiser_updates_more_than_128_tensors():
    from bigcn_amd import TreeBERTTrainStep
    c = T.case("t_layers_24")
    m = _new_model(c)
    step = TreeBERTTrainStep(m, drop_seed=3)
    assert len(step.optimizer.params()) == 393 and len(step.optimizer.chunks) == 4
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    step.step(_data(c))
    assert step.check_status() == 0 and step.step_count == 1
    assert len(step.grads()) == 392
    for n, p in m.named_parameters():
        assert torch.equal(p, before[n]) == ("word_embeddings" in n), n
    sd = step.optimizer.state_dict()
    assert sd["step_count"] == 1 and len(sd["exp_avg"]) == 393
    step.optimizer.load_state_dict(sd)
    assert step.step_count == 1


def test_forward_in_training_mode_and_version_2_raise():
    from bigcn_amd import TreeBERTTrainStep
    c = T.case("t_single")
    m = _new_model(c)
    assert "hidden_dropout" not in m.state_dict() and m.hidden_dropout == 0.1 and m.attn_dropout == 0.1
    m.train()
    with pytest.raises(NotImplementedError, match="training"):
        m(torch.zeros(1, 1, c.cfg["hidden"], device=DEV))
    m.version = 2
    with pytest.raises(NotImplementedError, match="out_labels"):
        TreeBERTTrainStep(m).step(_data(c))
