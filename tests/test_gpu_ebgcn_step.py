"""GPU checks of EBGCN's training-loop body: the loss kernel (bgcn_ebgcn_train_loss) against torch in fp64,
and EBGCNTrainStep (train forward + loss kernel + backward + MultiAdam, no host sync) against the fp64
reference trajectory of tests/ebgcn_step_ref.py (tests/test_ebgcn_step_ref.py shows on the CPU that fp32
arithmetic alone stays inside these bars on the fixture with the noise seed recorded in ebgcn_step_ref, and
why the fixture's own draw is not used: its third step has a LeakyReLU argument at 1e-9 of the largest, a coin
toss in fp32 that moved d TDrumorGCN.conv1.bias to 1.5e-4 of its maximum on the MI355X).
Bars: the project's standing |a - b| <= 1e-4 max|b| for the loss, every gradient and every parameter after
every update, as tests/test_gpu_trajectory.py.

One gradient is zero in exact arithmetic: conv1.bias of a direction whose edge inference is off (the bias is
a per-column constant that bn1's batch statistics remove, and the readout's root rows are detached); its
fp64 value is rounding noise (~1e-17), which no scale of its own can bound.  It is a column sum of the same
d conv1-output that d conv1.lin.weight = dZ^T X is formed from, so it is held to 1e-4 of that gradient's
maximum instead.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import ebgcn_step_ref as R
import ebgcn_train_ref as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4


def _close(got, want, what, scale=None):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = float((got - want).abs().max())
    scale = float(want.abs().max()) if scale is None else scale
    print(f"{what}: max err {err:.3e}, scale {scale:.3e}")
    assert err <= TOL * scale, f"{what}: {err} vs {TOL} * {scale}"


# ------------------------------------------------------------------------------------------ the loss kernel
def _loss_call(logp, y, td, bu, w_td=0.2, w_bu=0.3, status=0, want_pred=True):
    from bigcn_amd import _lib
    from bigcn_amd._lib import check, ptr, stream_handle
    B, C = logp.shape
    out = {"loss": torch.full((1,), float("nan"), device=DEV), "correct": torch.full((1,), -1, dtype=torch.int32, device=DEV),
           "pred": torch.full((B,), -1, dtype=torch.int64, device=DEV) if want_pred else None,
           "dlogp": torch.full((B, C), float("nan"), device=DEV),
           "status": torch.full((1,), status, dtype=torch.int32, device=DEV),
           "skip": torch.full((1,), float("nan"), device=DEV), "seen": torch.zeros(1, dtype=torch.int32, device=DEV)}
    check(_lib.lib().bgcn_ebgcn_train_loss(ptr(logp), ptr(y), B, C, ptr(td), ptr(bu), w_td, w_bu, ptr(out["loss"]),
                                           ptr(out["correct"]), ptr(out["pred"]), ptr(out["dlogp"]),
                                           ptr(out["status"]), ptr(out["skip"]), ptr(out["seen"]), stream_handle()))
    return out


def _loss_inputs(B, C, seed=0):
    g = torch.Generator().manual_seed(100 * B + C + seed)
    logp = F.log_softmax(torch.randn(B, C, generator=g) * 2, dim=1)
    logp[0, :] = logp[0, C - 1]                  # a row with a tied maximum (every class): torch.max gives index 0
    if B > 2:
        logp[2, C - 1] = logp[2].max()           # a tie between the maximum and the last class
    y = torch.randint(0, C, (B,), generator=g)
    y[0] = 0
    return logp.to(DEV), y.to(DEV), torch.rand((), generator=g).to(DEV), torch.rand((), generator=g).to(DEV)


@pytest.mark.parametrize("with_td,with_bu", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("C", [2, 4, 16])
@pytest.mark.parametrize("B", [1, 3, 130])
def test_loss_kernel_matches_torch(B, C, with_td, with_bu):
    logp, y, td, bu = _loss_inputs(B, C)
    td, bu = td if with_td else None, bu if with_bu else None
    out = _loss_call(logp, y, td, bu)
    lp = logp.double().requires_grad_(True)
    want = F.nll_loss(lp, y)
    nll = want
    if td is not None:
        want = want + 0.2 * td.double()
    if bu is not None:
        want = want + 0.3 * bu.double()
    _close(out["loss"].view(()), want, "loss")
    (dl,) = torch.autograd.grad(nll, lp)
    _close(out["dlogp"], dl, "dlogp")
    assert int(((out["dlogp"] != 0).sum(dim=1) == 1).sum()) == B   # -1/B at the label, exact zeros elsewhere
    _, pred = logp.max(dim=-1)
    assert torch.equal(out["pred"], pred) and int(out["pred"][0]) == 0
    assert int(out["correct"]) == int(pred.eq(y).sum())
    assert int(out["status"]) == 0 and float(out["skip"]) == 0.0 and int(out["seen"]) == 0
    again = _loss_call(logp, y, td, bu)                               # two calls: equal bits
    for k in ("loss", "dlogp"):
        assert torch.equal(out[k].view(torch.int32), again[k].view(torch.int32)), k
    assert int(_loss_call(logp, y, td, bu, want_pred=False)["correct"]) == int(out["correct"])


@pytest.mark.parametrize("bad", [-1, "C"])
def test_loss_kernel_flags_a_label_out_of_range(bad):
    B, C = 130, 4
    logp, y, td, bu = _loss_inputs(B, C)
    y = y.clone()
    y[77] = C if bad == "C" else bad
    out = _loss_call(logp, y, td, None)
    assert int(out["status"]) == 2 and float(out["skip"]) != 0.0 and int(out["seen"]) == 2
    ok = torch.ones(B, dtype=torch.bool, device=DEV)
    ok[77] = False
    want = -(logp.double()[ok].gather(1, y[ok].view(-1, 1)).sum()) / B + 0.2 * td.double()   # that tree left out
    _close(out["loss"].view(()), want, "loss without the invalid tree")
    assert bool((out["dlogp"][77] == 0).all()) and int((out["dlogp"] != 0).sum()) == B - 1
    _, pred = logp.max(dim=-1)
    assert torch.equal(out["pred"], pred) and int(out["correct"]) == int(pred[ok].eq(y[ok]).sum())


def test_loss_kernel_turns_a_status_on_entry_into_the_skip_flag():
    logp, y, td, bu = _loss_inputs(3, 4)
    for status in (1, 16, 1 | 16):
        out = _loss_call(logp, y, td, bu, status=status)
        assert int(out["status"]) == status and float(out["skip"]) != 0.0 and int(out["seen"]) == status
    out = _loss_call(logp, y, td, bu, status=0)
    assert float(out["skip"]) == 0.0


# ------------------------------------------------------------------------------------------------ the step
@functools.lru_cache(maxsize=None)
def _fixture():
    return T.load_npz(R.MODEL_FIXTURE)


@functools.lru_cache(maxsize=None)
def _reference(steps, td, bu):
    """The fp64 trajectory, computed once and left unchanged."""
    return R.trajectory(_fixture(), torch.float64, steps, td, bu)


def _case(td=True, bu=True):
    from bigcn_amd import EBGCN, EBGCNTrainStep
    import argparse
    z = _fixture()
    args = R.args_of(z, td, bu, DEV)
    model = EBGCN(args)
    model.load_state_dict(T.group(z, "sd"), strict=True)
    model = model.to(DEV).train()
    data = argparse.Namespace(**{k: z[k].to(DEV) for k in ("x", "edge_index", "BU_edge_index", "batch", "rootindex", "y")})
    ntd, nbu = R.noise_of(z)                           # ebgcn_step_ref.NOISE_SEED, and why it is not the fixture's
    noise = (ntd.to(DEV) if td else None, nbu.to(DEV) if bu else None)
    return z, model, EBGCNTrainStep(model, args=args), data, noise


def _bits(model, step):
    out = {k: p.detach().clone() for k, p in model.named_parameters()}
    for k, p in model.named_parameters():
        m, v = step.optimizer.state[p]
        out["m:" + k], out["v:" + k] = m.clone(), v.clone()
    return out


def _same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


def _check_step(model, got_loss, got_correct, want, zero_scale_of=()):
    """Every figure is printed before the first one is asserted."""
    bad = []

    def close(*a, **kw):
        try:
            _close(*a, **kw)
        except AssertionError as e:
            bad.append(str(e))

    close(got_loss, want["loss"], "loss")
    params = dict(model.named_parameters())
    for k, g in want["grads"].items():
        if g is None:
            assert params[k].grad is None, k
        elif k in zero_scale_of:
            close(params[k].grad, g, "d " + k + " (zero in exact arithmetic)",
                  scale=float(want["grads"][zero_scale_of[k]].abs().max()))
        else:
            close(params[k].grad, g, "d " + k)
    for k, p in want["params"].items():
        close(params[k], p, k)
    assert not bad, bad
    assert int(got_correct) == want["correct"]


def test_three_steps_track_the_fp64_trajectory():
    z, model, step, data, noise = _case()
    want, none = _reference(3, True, True)
    assert len(none) == 42
    start = {k: p.detach().clone() for k, p in model.named_parameters()}
    for t in range(3):
        loss, correct = step.step(data, noise=noise)
        assert loss.dim() == 0 and correct.dim() == 0 and loss.dtype == torch.float32 and correct.dtype == torch.int32
        _check_step(model, loss, correct, want[t])
    assert step.step_count == 3 and step.check_status() == 0
    now = dict(model.named_parameters())
    for k in none:                                     # no gradient: the initial bits, no weight decay either
        assert torch.equal(now[k].view(torch.int32), start[k].view(torch.int32)), k
        m, v = step.optimizer.state[now[k]]
        assert not bool(m.any()) and not bool(v.any()), k
    assert [g["lr"] for g in step.optimizer.param_groups] == [R.LR, R.LR / 5, R.LR / 5, R.LR, R.LR]
    assert len(step.optimizer.params()) == 68 and step.optimizer.weight_decay == R.L2
    loss, correct, pred = step.step(data, noise=noise, pred=True)
    assert pred.shape == data.y.shape and int(pred.eq(data.y).sum()) == int(correct)


@pytest.mark.parametrize("td,bu", [(True, False), (False, True)])
def test_one_step_with_edge_inference_off_in_one_direction(td, bu):
    z, model, step, data, noise = _case(td, bu)
    want, none = _reference(1, td, bu)
    off = "BUrumorGCN" if td else "TDrumorGCN"
    assert len(none) == 21 + 27 and sum(k.startswith(off) for k in none) == 27
    start = {k: p.detach().clone() for k, p in model.named_parameters()}
    loss, correct = step.step(data, noise=noise)
    _check_step(model, loss, correct, want[0], zero_scale_of={off + ".conv1.bias": off + ".conv1.lin.weight"})
    now = dict(model.named_parameters())
    for k in none:                                     # the off direction's per-edge networks, fc1 and fc2 among them
        assert torch.equal(now[k].view(torch.int32), start[k].view(torch.int32)), k
    assert step.check_status() == 0


@pytest.mark.parametrize("what", ["edge", "root", "label"])
@pytest.mark.parametrize("td,bu", [(True, True), (False, False)])
def test_an_invalid_batch_skips_the_update_and_the_next_valid_one_updates(what, td, bu):
    """With both directions' edge inference off only the graph builds see a bad edge."""
    import argparse
    z, model, step, data, noise = _case(td, bu)
    step.step(data, noise=noise)                       # moments away from zero
    assert step.check_status() == 0
    before = _bits(model, step)
    bad = argparse.Namespace(**vars(data))
    N = data.x.size(0)
    if what == "edge":
        bad.edge_index = data.edge_index.clone()
        bad.edge_index[1, 3] = N + 5
        bad.BU_edge_index = data.BU_edge_index.clone()
        bad.BU_edge_index[0, 3] = N + 5
    elif what == "root":
        bad.rootindex = data.rootindex.clone()
        bad.rootindex[2] = N
    else:
        bad.y = data.y.clone()
        bad.y[1] = 4
    step.step(bad, noise=noise)
    assert step.step_count == 2
    _same_bits(before, _bits(model, step))
    text = "label outside" if what == "label" else "edge, root or tree index out of range"
    with pytest.raises(IndexError, match=text):
        step.check_status()
    assert step.last_skipped == 1
    assert step.check_status() == 0                    # the check clears what it reported
    step.step(data, noise=noise)
    after = _bits(model, step)
    assert step.step_count == 3 and step.check_status() == 0
    moved = [k for k in before if not torch.equal(before[k], after[k])]
    assert len(moved) == 3 * (68 - 21 * (int(td) + int(bu)) - 27 * (2 - int(td) - int(bu)))


def test_no_host_sync_inside_a_step():
    z, model, step, data, noise = _case()
    step.step(data, noise=noise)                       # warm-up: the table upload, the workspaces
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("error")
        sync_checked = True
    except Exception:       # this torch build has no such mode: the steps still run, unchecked
        sync_checked = False
    try:
        for _ in range(2):
            loss, correct, pred = step.step(data, noise=noise, pred=True)   # a host sync in here raises
        if sync_checked:
            with pytest.raises(RuntimeError):
                loss.item()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    print("sync debug mode checked:", sync_checked)
    assert step.check_status() == 0 and step.step_count == 3


def test_two_fresh_models_end_with_equal_bits():
    runs = []
    for _ in range(2):
        z, model, step, data, noise = _case()
        losses = [step.step(data, noise=noise)[0].clone() for _ in range(2)]
        assert step.check_status() == 0
        runs.append((_bits(model, step), losses))
    _same_bits(runs[0][0], runs[1][0])
    for a, b in zip(runs[0][1], runs[1][1]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
