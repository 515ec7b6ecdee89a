"""GPU checks of the train-mode bn1 + conv2 lin without the dense concat (``bgcn_ebgcn_conv2_lin_train_fwd`` /
``_bwd``, ``ebgcn_conv2_lin_train``), of ``gcn_aggregate`` and of ``EBGCN.train_forward`` on them, against the
fp64 DENSE restatement (tests/ebgcn_bn1_ref.py ``dense_reference``: ``bn_train`` over the materialised
concat, relu, ``F.linear``, autograd; tests/test_ebgcn_bn1_train.py pins the factored algebra to it).
Bar: the project's standing max|a - b| <= 1e-4 max|b| per tensor, no element left out."""
import argparse
import functools
import os

import pytest
import torch
import torch.nn.functional as F

import ebgcn_bn1_ref as R
import ebgcn_train_ref as T
from oracle import bigcn_oracle as O

from bigcn_amd import ebgcn_conv2_lin_train, gcn_aggregate

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_FIXTURE = os.path.join(ROOT, "tests", "golden", "train_ebgcn_model.npz")
DEV = "cuda:0"
TOL = 1e-4
TENSORS = ("z2", "dh1", "dW2", "dgamma", "dbeta", "running_mean", "running_var")


def _close(got, want, what):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err, scale = float((got - want).abs().max()), float(want.abs().max())
    print(f"{what}: max err {err:.3e}, max |ref| {scale:.3e}")
    assert err <= TOL * scale, f"{what}: {err} vs {TOL} * {scale}"


@functools.lru_cache(maxsize=None)
def _reference(N, B, F_in, momentum=T.BN_MOMENTUM):
    return R.dense_reference(R.make_case(N, B, F_in), momentum)


def _bn1(case, **kw):
    C = case["gamma"].numel()
    bn = torch.nn.BatchNorm1d(C, **kw)
    with torch.no_grad():
        bn.weight.copy_(case["gamma"])
        bn.bias.copy_(case["beta"])
        if bn.running_mean is not None:
            bn.running_mean.copy_(case["running_mean"])
            bn.running_var.copy_(case["running_var"])
            bn.num_batches_tracked.copy_(case["num_batches_tracked"])
    return bn.to(DEV).train()


def _run(case, bn=None, h1=None, x=None, batch=None, rootindex=None, up=None):
    """One forward + backward of the op: the tensors of TENSORS, num_batches_tracked, the status word."""
    bn = _bn1(case) if bn is None else bn
    h1 = (case["h1"].to(DEV) if h1 is None else h1).requires_grad_(True)
    x = case["x"].to(DEV) if x is None else x
    batch = case["batch"] if batch is None else batch
    rootindex = case["rootindex"] if rootindex is None else rootindex
    up = case["up"] if up is None else up
    W2 = case["W2"].to(DEV).requires_grad_(True)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    z2 = ebgcn_conv2_lin_train(h1, x, batch.to(DEV), rootindex.to(DEV), W2, bn, status=status)
    dh1, dW2, dgamma, dbeta = torch.autograd.grad((up.to(DEV) * z2).sum(), [h1, W2, bn.weight, bn.bias])
    return dict(z2=z2.detach(), dh1=dh1, dW2=dW2, dgamma=dgamma, dbeta=dbeta, running_mean=bn.running_mean,
                running_var=bn.running_var, num_batches_tracked=bn.num_batches_tracked, status=int(status.item()))


@pytest.mark.parametrize("N,B,F_in", R.SHAPES)
def test_matches_the_dense_restatement(N, B, F_in):
    case, ref = R.make_case(N, B, F_in), _reference(N, B, F_in)
    # relu's mask jumps at y = 0: the case keeps every pre-activation away from it (checked in fp64)
    assert float(ref["y"].abs().min()) >= R.MARGIN * float(ref["y"].abs().max())
    got = _run(case)
    assert got["status"] == 0
    for k in TENSORS:
        _close(got[k], ref[k], f"{k} N={N} B={B} F={F_in}")
    assert int(got["num_batches_tracked"]) == int(ref["num_batches_tracked"]) == int(case["num_batches_tracked"]) + 1


@pytest.mark.parametrize("N,B,F_in", [(1031, 130, 300), (64, 4, 8)])
def test_z2_has_the_bits_of_the_eval_kernel_on_the_returned_fold(N, B, F_in):
    from bigcn_amd import _lib, ops
    case = R.make_case(N, B, F_in)
    h1, x = case["h1"].to(DEV), case["x"].to(DEV)
    batch, rootindex, W2 = case["batch"].to(DEV), case["rootindex"].to(DEV), case["W2"].to(DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    meta = {"eps": T.BN_EPS, "status": status}
    z2 = ops._Conv2LinTrainFn.apply(meta, h1, W2, case["gamma"].to(DEV), case["beta"].to(DEV), x, batch, rootindex)
    g, t = meta["bn_g"].contiguous(), meta["bn_t"].contiguous()
    want = torch.empty(N, 64, dtype=torch.float32, device=DEV)
    L = _lib.lib()
    ws = _lib.workspace(L.bgcn_ebgcn_conv2_lin_workspace_size(N, B, F_in), DEV)
    _lib.check(L.bgcn_ebgcn_conv2_lin(h1.data_ptr(), 64, x.data_ptr(), F_in, batch.data_ptr(), rootindex.data_ptr(), N, B,
                                      F_in, 64, W2.data_ptr(), g.data_ptr(), t.data_ptr(), want.data_ptr(), 64,
                                      status.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_handle()))
    assert int(status.item()) == 0 and int(meta["num_valid"].item()) == N
    assert torch.equal(z2, want)


def test_strided_views_give_the_bits_of_contiguous_copies():
    N, B, F_in = 257, 3, 68
    case = R.make_case(N, B, F_in)
    a = _run(case)
    hbuf = torch.full((N, 72), 7.0, device=DEV)
    xbuf = torch.full((N, F_in + 4), 7.0, device=DEV)
    hbuf[:, :64] = case["h1"].to(DEV)
    xbuf[:, :F_in] = case["x"].to(DEV)
    hv, xv = hbuf[:, :64].detach(), xbuf[:, :F_in]
    assert hv.stride(0) == 72 and xv.stride(0) == F_in + 4
    b = _run(case, h1=hv, x=xv)
    for k in TENSORS:
        assert torch.equal(a[k], b[k]), k


def test_a_shuffled_batch_vector_gives_the_permuted_result():
    N, B, F_in = 1031, 130, 300
    case, ref = R.make_case(N, B, F_in), _reference(N, B, F_in)
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(5))
    inv = torch.empty(N, dtype=torch.int64)
    inv[perm] = torch.arange(N)
    batch = case["batch"][perm]
    assert bool((batch[1:] < batch[:-1]).any())
    got = _run(case, h1=case["h1"][perm].to(DEV), x=case["x"][perm].to(DEV), batch=batch,
               rootindex=inv[case["rootindex"]], up=case["up"][perm])
    assert got["status"] == 0
    _close(got["z2"], ref["z2"][perm], "z2, nodes permuted")
    _close(got["dh1"], ref["dh1"][perm], "dh1, nodes permuted")
    for k in TENSORS[2:]:
        _close(got[k], ref[k], k + ", nodes permuted")


def test_two_calls_give_equal_bits():
    case = R.make_case(1031, 130, 300)
    a, b = _run(case), _run(case)
    for k in TENSORS + ("num_batches_tracked",):
        assert torch.equal(a[k], b[k]), k


def test_out_of_range_indices_are_flagged_zeroed_and_left_out():
    """The (257, 3, 68) case with five invalid nodes appended: three in a fourth tree whose rootindex is N,
    one with the tree id B, one with -1 (which also makes the batch vector non-monotone).  The valid part is
    the case itself, so everything else is the restatement on the batch with those nodes removed."""
    N0, B0, F_in = 257, 3, 68
    case, ref = R.make_case(N0, B0, F_in), _reference(N0, B0, F_in)
    N, B = N0 + 5, B0 + 1
    g = torch.Generator().manual_seed(11)
    h1 = torch.cat((case["h1"], torch.randn(5, 64, generator=g) * 50))
    x = torch.cat((case["x"], torch.rand(5, F_in, generator=g) * 50))
    up = torch.cat((case["up"], torch.randn(5, 64, generator=g) * 50))
    batch = torch.cat((case["batch"], torch.tensor([B0, B0, B0, B, -1])))
    rootindex = torch.cat((case["rootindex"], torch.tensor([N])))
    got = _run(case, h1=h1.to(DEV), x=x.to(DEV), batch=batch, rootindex=rootindex, up=up)
    assert got["status"] & 1
    assert bool((got["z2"][N0:] == 0).all()) and bool((got["dh1"][N0:] == 0).all())
    _close(got["z2"][:N0], ref["z2"], "z2 of the valid nodes")
    _close(got["dh1"][:N0], ref["dh1"], "dh1 of the valid nodes")
    for k in TENSORS[2:]:
        _close(got[k], ref[k], k + " over the valid nodes")
    assert int(got["num_batches_tracked"]) == int(case["num_batches_tracked"]) + 1


def test_a_batch_without_a_valid_node_gives_zeros_and_blends_nothing():
    N, B, F_in = 64, 4, 8
    case = R.make_case(N, B, F_in)
    bn = _bn1(case)
    before = {k: v.clone() for k, v in bn.state_dict().items()}
    got = _run(case, bn=bn, batch=torch.full((N,), B), rootindex=case["rootindex"])
    assert got["status"] & 1
    for k in TENSORS[:5]:
        assert bool((got[k] == 0).all()), k
    for k, v in bn.state_dict().items():
        assert torch.equal(v, before[k]), k
    # every rootindex out of range: the same
    got = _run(case, bn=bn, rootindex=torch.tensor([N, -1, N + 3, N]))
    assert got["status"] & 1 and bool((got["z2"] == 0).all()) and bool((got["dh1"] == 0).all())
    for k, v in bn.state_dict().items():
        assert torch.equal(v, before[k]), k


def test_cumulative_average_and_no_running_statistics():
    N, B, F_in = 257, 3, 68
    case = R.make_case(N, B, F_in)
    ref = _reference(N, B, F_in, None)
    got = _run(case, bn=_bn1(case, momentum=None))
    for k in TENSORS:
        _close(got[k], ref[k], k + " momentum=None")
    assert int(got["num_batches_tracked"]) == int(case["num_batches_tracked"]) + 1
    bn = _bn1(case, track_running_stats=False)
    assert bn.running_mean is None
    got = _run(case, bn=bn)
    for k in TENSORS[:5]:
        _close(got[k], ref[k], k + " track_running_stats=False")
    assert bn.running_mean is None and bn.num_batches_tracked is None


def test_refusals():
    N, B, F_in = 5, 3, 4
    case = R.make_case(N, B, F_in)
    bn = _bn1(case)
    before = {k: v.clone() for k, v in bn.state_dict().items()}
    h1, x, W2 = case["h1"].to(DEV), case["x"].to(DEV), case["W2"].to(DEV)
    batch, rootindex = case["batch"].to(DEV), case["rootindex"].to(DEV)
    with pytest.raises(ValueError, match="requires_grad"):
        ebgcn_conv2_lin_train(h1, x.clone().requires_grad_(True), batch, rootindex, W2, bn)
    for bad in (dict(h1=h1[:, :32]), dict(x=x[:4]), dict(batch=batch[:4]), dict(W2=W2[:, :64]), dict(W2=W2[:32]),
                dict(x=torch.zeros(N, 6, device=DEV), W2=torch.zeros(64, 70, device=DEV))):
        kw = dict(h1=h1, x=x, batch=batch, W2=W2)
        kw.update(bad)
        with pytest.raises(ValueError):
            ebgcn_conv2_lin_train(kw["h1"], kw["x"], kw["batch"], rootindex, kw["W2"], bn)
    with pytest.raises(ValueError):
        ebgcn_conv2_lin_train(h1, x, batch, rootindex, W2, torch.nn.BatchNorm1d(64 + F_in + 4).to(DEV))
    with pytest.raises(ValueError):
        ebgcn_conv2_lin_train(h1, x, batch, rootindex, W2, None)
    for k, v in bn.state_dict().items():
        assert torch.equal(v, before[k]), k


# ----------------------------------------------------------------------------- gcn_aggregate
def _graph_case(name):
    g = torch.Generator().manual_seed(3)
    N, K = 9, 12
    ei = {"no edges": torch.zeros(2, 0, dtype=torch.int64),
          "one edge": torch.tensor([[2], [5]]),
          "a repeated edge": torch.tensor([[0, 0, 1, 0, 3, 7, 7], [1, 2, 3, 1, 4, 8, 8]])}[name]
    E = ei.size(1)
    return (N, ei, torch.randn(N, K, generator=g), torch.randn(64, K, generator=g) * 0.3, torch.randn(64, generator=g),
            torch.rand(E, generator=g) * 0.8 + 0.1, torch.randn(N, 64, generator=g))


@pytest.mark.parametrize("name", ["no edges", "one edge", "a repeated edge"])
def test_gcn_aggregate_is_the_aggregation_half_of_gcn_conv(name):
    from bigcn_amd import gcn_conv, ops
    N, ei, x, W, b, ew, up = _graph_case(name)
    xd, Wd, eid, upd = x.to(DEV), W.to(DEV), ei.to(DEV), up.to(DEV)
    ew1, ew2 = ew.to(DEV).requires_grad_(True), ew.to(DEV).requires_grad_(True)
    b1, b2 = b.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    want = gcn_conv(xd, eid, Wd, b1, edge_weight=ew1)
    z = ops._linear(xd, Wd).requires_grad_(True)
    out = gcn_aggregate(z, eid, b2, edge_weight=ew2)
    assert torch.equal(out, want)
    dz, db, dew = torch.autograd.grad((upd * out).sum(), [z, b2, ew2])
    db_conv, dew_conv = torch.autograd.grad((upd * want).sum(), [b1, ew1])
    assert torch.equal(db, db_conv) and torch.equal(dew, dew_conv)
    # fp64 oracle: the aggregation of a given z is gcn_conv with the identity as its weight
    z64 = (x.double() @ W.double().t()).requires_grad_(True)
    b64, ew64 = b.double().requires_grad_(True), ew.double().requires_grad_(True)
    ref = O.gcn_conv(z64, ei, torch.eye(64, dtype=torch.float64), b64, edge_weight=ew64)
    rdz, rdb, rdew = torch.autograd.grad((up.double() * ref).sum(), [z64, b64, ew64])
    _close(out, ref, "A z + b")
    _close(dz, rdz, "d z")
    _close(db, rdb, "d bias")
    if ei.size(1):
        _close(dew, rdew, "d edge_weight")
    else:
        assert dew.shape == (0,)
    # without edge weights, and without a bias
    _close(gcn_aggregate(z.detach(), eid), O.gcn_conv(z64.detach(), ei, torch.eye(64, dtype=torch.float64), None),
           "A z")


# ----------------------------------------------------------------------------- model level
def _args(F_in, K, td=True, bu=True, C=4):
    return argparse.Namespace(input_features=F_in, hidden_features=64, output_features=64, num_class=C, edge_num=K,
                              edge_infer_td=td, edge_infer_bu=bu, device=DEV)


def test_train_forward_on_the_rewired_path_matches_the_restatement():
    """tests/test_gpu_ebgcn_train.py's comparison on the model fixture, repeated here so that this file
    covers ``_train_encode`` on ``ebgcn_conv2_lin_train`` + ``gcn_aggregate``."""
    from bigcn_amd import EBGCN
    z = T.load_npz(MODEL_FIXTURE)
    model = EBGCN(_args(64, int(z["edge_num"])))
    model.load_state_dict(T.group(z, "sd"), strict=True)
    model = model.to(DEV).train()
    data = argparse.Namespace(**{k: z[k].to(DEV) for k in ("x", "edge_index", "BU_edge_index", "batch", "rootindex", "y")})
    noise = (z["noise_td"], z["noise_bu"])
    logp, td, bu = model.train_forward(data, noise=tuple(n.to(DEV) for n in noise))
    (F.nll_loss(logp, data.y) + 0.2 * (td + bu)).backward()
    sd64 = T.with_grad(T.group(z, "sd"), torch.float64)
    new = {}
    rlogp, rtd, rbu = T.forward_train(sd64, z["x"].double(), z["edge_index"], z["BU_edge_index"], z["batch"],
                                      z["rootindex"], tuple(n.double() for n in noise), new_buffers=new)
    have, none, _ = T.grads_of(F.nll_loss(rlogp, z["y"]) + 0.2 * (rtd + rbu), sd64)
    _close(logp, rlogp, "log-probs")
    _close(td, rtd, "TD edge loss")
    _close(bu, rbu, "BU edge loss")
    got = {k: p.grad for k, p in model.named_parameters()}
    assert sorted(k for k, g in got.items() if g is None) == none
    for k, g in have.items():
        _close(got[k], g, "d " + k)
    after = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    for k, v in new.items():
        if v.is_floating_point():
            _close(after[k], v, k)
        else:
            assert int(after[k]) == int(v), k


def test_nothing_of_size_n_by_f_is_allocated():
    """F = 5000, N = 600, B = 6: over forward + backward the block allocates less than N F 4 bytes on top of
    its inputs - the dense concat alone is that large.  A bound from the sizes, not a measurement."""
    N, B, F_in = 600, 6, 5000
    g = torch.Generator().manual_seed(1)
    h1 = (torch.randn(N, 64, generator=g) * 0.7).to(DEV).requires_grad_(True)
    x = (torch.rand(N, F_in, generator=g) * (torch.rand(N, F_in, generator=g) < 0.1)).to(DEV)
    batch = torch.arange(N, device=DEV) // (N // B)
    rootindex = torch.arange(B, device=DEV) * (N // B)
    W2 = (torch.randn(64, 64 + F_in, generator=g) * 0.02).to(DEV).requires_grad_(True)
    up = torch.randn(N, 64, generator=g).to(DEV)
    bn = torch.nn.BatchNorm1d(64 + F_in).to(DEV).train()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    z2 = ebgcn_conv2_lin_train(h1, x, batch, rootindex, W2, bn)
    (up * z2).sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"peak above the inputs: {peak} bytes, N F 4 = {N * F_in * 4}")
    assert h1.grad is not None and W2.grad is not None and bool(torch.isfinite(W2.grad).all())
    assert peak < N * F_in * 4
