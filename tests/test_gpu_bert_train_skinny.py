"""GPU checks of TreeBERT's training call on the skinny fp32 GEMMs (bgcn_bert_train_grad_skinny,
``TreeBERT.grad_batch(..., gemm="skinny")``, ``TreeBERTTrainStep(model, gemm="skinny")``) against the fp64
autograd restatement of the reference loop (tests/bert_train_ref.py, used as it is: cases, oracle, BAR =
1e-4, rel_err), against the tiled path, and the properties the call keeps by construction.  The batches,
faults and helpers are tests/test_gpu_bert_train.py's.

t_rows_over_switch is left out: 8200 rows is not what a skinny path is for, and t_many_trees' 300 rows
already cross every row-block boundary of the kernels."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

import bert_train_ref as T
import test_gpu_bert_train as B0

pytestmark = pytest.mark.gpu

DEV = B0.DEV
CASES = ["t_single", "t_boundaries", "t_many_trees", "t_hidden_1024", "t_hidden_320", "t_layers_24", "t_full_width",
         "t_classes_63"]


def _train(m, c, drop, gemm="skinny", seed=T.DROP_SEED, dx=True):
    p_h, p_a = T.DROPS[drop]
    return m._train(B0._x(c), c.rootindex.to(DEV), c.y.to(DEV), dx=dx, drop_seed=seed, hidden_dropout=p_h,
                    attn_dropout=p_a, gemm=gemm)


def _named(m, r):
    g = dict(zip(m.names(), r["grads"]))
    g["x"] = r["dx"]
    return g


# ---------------------------------------------------------------- parity
@pytest.mark.parametrize("drop", list(T.DROPS))
@pytest.mark.parametrize("name", CASES)
def test_gradients_match_the_fp64_autograd_loop(name, drop):
    c = T.case(name)
    want = T.oracle(name, drop)
    m = B0._model(name)
    r = _train(m, c, drop)
    m.check_status()
    g = _named(m, r)
    assert sorted(g) == sorted(want.grads)
    errs = {k: T.rel_err(g[k], want.grads[k]) for k in want.grads}
    loss_err = abs(float(r["loss"]) - float(want.loss))
    logp_err = float((r["logp"].double().cpu() - want.logp).abs().max())
    print(name, drop, max(errs, key=errs.get), f"{max(errs.values()):.2e}", f"{loss_err:.2e}", f"{logp_err:.2e}")
    for k, e in errs.items():
        assert e <= T.BAR, (k, e)
    assert loss_err <= T.BAR and logp_err <= T.BAR
    for k, v in g.items():
        if ".query." in k or ".key." in k:
            assert float(v.abs().max()) == 0.0, k
    # through the public method: the same call
    loss, correct, g2 = m.grad_batch(B0._x(c), c.rootindex.to(DEV), c.y.to(DEV), dx=True, drop_seed=T.DROP_SEED,
                                     hidden_dropout=T.DROPS[drop][0], attn_dropout=T.DROPS[drop][1], gemm="skinny")
    assert torch.equal(loss, r["loss"].view(())) and torch.equal(correct, r["correct"].view(()))
    B0._same_grads(g2, g)


def test_the_skinny_and_the_tiled_path_agree_on_full_width():
    c = T.case("t_full_width")
    m = B0._model("t_full_width")
    a, b = _train(m, c, "p01", gemm="skinny"), _train(m, c, "p01", gemm="tiled")
    m.check_status()
    assert abs(float(a["loss"]) - float(b["loss"])) <= T.BAR
    assert float((a["logp"] - b["logp"]).abs().max()) <= T.BAR
    ga, gb = _named(m, a), _named(m, b)
    for k in gb:
        assert T.rel_err(ga[k], gb[k]) <= T.BAR, k


# ---------------------------------------------------------------- the C ABI, called directly
def _capi(name, fill, drop="p01", rootindex=None, y=None, x=None):
    """One bgcn_bert_train_grad_skinny call on a workspace, outputs and gradient buffers pre-filled with ``fill``
    ("zero", or "ff": NaN as fp32); host copies of every output."""
    from bigcn_amd import _lib
    from bigcn_amd.bert import _LAYER_FIELDS, _TOP_FIELDS, LN_EPS
    lib = _lib.lib()
    c = T.case(name)
    cfg = c.cfg
    w = {k: v.float().contiguous().to(DEV) for k, v in c.sd.items()}
    H, L, C = cfg["hidden"], cfg["layers"], cfg["out"]
    x = B0._x(c) if x is None else x
    N = x.size(0)
    root = (c.rootindex if rootindex is None else rootindex).to(DEV)
    B = root.numel()
    yy = (c.y if y is None else y).to(DEV)
    need = lib.bgcn_bert_train_skinny_workspace_size(N, B, H, cfg["intermediate"], L)
    assert need > 0 and need % 256 == 0
    ws = B0._buf(need, fill)
    bufs = {"logp": B0._buf(4 * B * C, fill), "status": B0._buf(4, fill), "loss": B0._buf(4, fill),
            "correct": B0._buf(4, fill), "pred": B0._buf(8 * B, fill), "skip_flag": B0._buf(4, fill),
            "x": B0._buf(4 * N * x.stride(0), fill)}
    names = T.grad_names(c)
    for k in names:
        bufs[k] = B0._buf(4 * w[k].numel(), fill)
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
    t.hidden_dropout, t.attn_dropout = T.DROPS[drop]
    assert lib.bgcn_bert_train_grad_skinny(ctypes.addressof(t), ws.data_ptr(), need, _lib.stream_handle()) == 0
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


@pytest.mark.parametrize("name", ["t_boundaries", "t_many_trees"])
def test_results_do_not_depend_on_what_the_buffers_held(name):
    want = _capi(name, "zero")
    got = _capi(name, "ff")
    again = _capi(name, "ff")
    ref = T.oracle(name, "p01")
    for r in (want, got, again):
        assert r.status == 0 and r.skip_flag == 0.0
    for k in ("logp", "loss", "correct", "pred"):
        assert torch.equal(getattr(got, k), getattr(want, k)) and torch.equal(getattr(again, k), getattr(got, k)), k
    B0._same_grads(got.grads, want.grads)
    B0._same_grads(again.grads, got.grads)
    for k, g in ref.grads.items():
        assert T.rel_err(want.grads[k], g) <= T.BAR, k


def test_one_seed_gives_one_set_of_bits():
    c = T.case("t_full_width")
    m = B0._model("t_full_width")
    a, b = _train(m, c, "p01"), _train(m, c, "p01")
    other = _train(m, c, "p01", seed=T.DROP_SEED + 1)
    m.check_status()
    assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["logp"], b["logp"])
    B0._same_grads(_named(m, a), _named(m, b))
    assert not torch.equal(a["loss"], other["loss"])


def test_permuting_the_trees_permutes_logp_exactly_without_dropout():
    """The split of every product is a function of the weight's shape, never of B, every row of a product
    is its own chain and every row kernel works per row: a tree's logp does not depend on its place."""
    c = T.case("t_boundaries")
    m = B0._model("t_boundaries")
    x = B0._x(c)
    kw = dict(hidden_dropout=0.0, attn_dropout=0.0, gemm="skinny")
    want = m._train(x, c.rootindex.to(DEV), c.y.to(DEV), **kw)["logp"]
    order = [3, 0, 4, 2, 1]
    ends = c.rootindex.tolist()[1:] + [c.N]
    spans = [(int(c.rootindex[o]), ends[o]) for o in order]
    xp = torch.cat([x[s:e] for s, e in spans]).contiguous()
    lens = [e - s for s, e in spans]
    rootp = torch.tensor([0] + lens[:-1]).cumsum(0)
    got = m._train(xp, rootp.to(DEV), c.y[order].to(DEV), **kw)["logp"]
    alone = m._train(xp[:lens[0]].contiguous(), rootp[:1].to(DEV), c.y[order][:1].to(DEV), **kw)["logp"]
    m.check_status()
    assert torch.equal(got, want[order])
    assert torch.equal(alone[0], want[order[0]])      # B = 1 against B = 5


# ---------------------------------------------------------------- validity on the device
@pytest.mark.parametrize("kind", B0.FAULTS)
def test_an_invalid_batch_is_flagged_and_skips_the_update(kind):
    from bigcn_amd import TreeBERTTrainStep, _lib
    c = T.case("t_many_trees")
    m = B0._new_model(c)
    step = TreeBERTTrainStep(m, drop_seed=11, gemm="skinny")
    step.step(B0._data(c))   # a valid step first: the moments are not zero
    assert step.check_status() == 0
    before = B0._snapshot(m, step.optimizer)
    x, root, y = B0._fault(c, kind)
    step.step(B0._data(c, x, root, y))
    assert int(m.__dict__["_state"]["status"]) == _lib.BGCN_STATUS_SEQUENCE
    assert float(step._st["skip_flag"]) == 1.0
    for u, v in zip(B0._snapshot(m, step.optimizer), before):
        assert torch.equal(u, v)
    assert step.step_count == 2
    with pytest.raises(IndexError, match="1 updates skipped"):
        step.check_status()
    assert step.last_skipped == 1 and step.check_status() == 0
    loss, _ = step.step(B0._data(c))
    assert step.check_status() == 0 and float(step._st["skip_flag"]) == 0.0 and bool(torch.isfinite(loss))
    assert any(not torch.equal(u, v) for u, v in zip(B0._snapshot(m, step.optimizer), before))
    # through the C ABI on buffers of NaN bits: flagged, and every gradient buffer written whole
    r = _capi("t_many_trees", "ff", rootindex=root, y=y, x=x)
    assert r.status == _lib.BGCN_STATUS_SEQUENCE and r.skip_flag == 1.0
    for k, v in r.grads.items():
        assert bool(torch.isfinite(v).all()), k


# ---------------------------------------------------------------- the step
def test_the_skinny_step_follows_the_reference_loop():
    from bigcn_amd import TreeBERTTrainStep
    c = T.case("t_boundaries")
    m = B0._new_model(c)
    m.hidden_dropout = m.attn_dropout = 0.1
    step = TreeBERTTrainStep(m, lr=T.LR, weight_decay=T.WEIGHT_DECAY, drop_seed=T.DROP_SEED, gemm="skinny")
    want, _ = T.train_losses(c, 3, torch.float64, 0.1, 0.1)
    data = B0._data(c)
    got = []
    for i in range(3):
        loss, correct = step.step(data)
        assert step.last_drop_seed == T.DROP_SEED + i
        got.append(float(loss))
    assert step.step_count == 3 and step.check_status() == 0
    print(got, want)
    for u, v in zip(got, want):
        assert abs(u - v) <= T.BAR
    assert all(p.grad is None for p in m.parameters())


def test_the_tiled_keyword_is_the_step_without_it():
    from bigcn_amd import TreeBERTTrainStep
    c = T.case("t_boundaries")
    a, b = B0._new_model(c), B0._new_model(c)
    plain = TreeBERTTrainStep(a, drop_seed=5)
    tiled = TreeBERTTrainStep(b, drop_seed=5, gemm="tiled")
    assert plain.gemm == "tiled"
    data = B0._data(c)
    for _ in range(2):
        la, lb = plain.step(data), tiled.step(data)
        assert torch.equal(la[0], lb[0]) and torch.equal(la[1], lb[1])
    for (n, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(p, q), n
    assert plain.check_status() == 0 and tiled.check_status() == 0


def test_another_keyword_raises():
    from bigcn_amd import TreeBERTTrainStep
    c = T.case("t_single")
    m = B0._model("t_single")
    with pytest.raises(ValueError, match="gemm"):
        TreeBERTTrainStep(m, gemm="fast")
    with pytest.raises(ValueError, match="gemm"):
        m.grad_batch(B0._x(c), c.rootindex.to(DEV), c.y.to(DEV), gemm="fast")
