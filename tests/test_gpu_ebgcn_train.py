"""GPU checks of the EBGCN training path: the fp32 HIP kernels (bgcn_edge_infer_train_fwd / _bwd) and
``EBGCN.train_forward`` against the fp64 restatement (tests/ebgcn_train_ref.py, itself pinned to
reference-produced fixtures by tests/test_ebgcn_train.py).
Bar: the project's standing |a - b| <= 1e-4 max|b| per tensor, for outputs, gradients and buffers."""
import argparse
import functools
import glob
import os

import pytest
import torch
import torch.nn.functional as F

import ebgcn_train_ref as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE_FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "train_ebgcn_edge_*.npz")))
EDGE_NAMES = [os.path.basename(p)[len("train_ebgcn_edge_"):-len(".npz")] for p in EDGE_FIXTURES]
MODEL_FIXTURE = os.path.join(ROOT, "tests", "golden", "train_ebgcn_model.npz")
DEV = "cuda:0"
TOL = 1e-4
SHAPES = [(1, 1, 50), (33, 2, 50), (33, 3, 2), (1000, 3, 50), (2100, 1, 2)]   # (E, K, N)


def _close(got, want, what):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err, scale = float((got - want).abs().max()), float(want.abs().max())
    print(f"{what}: max err {err:.3e}, max |ref| {scale:.3e}")
    assert err <= TOL * scale, f"{what}: {err} vs {TOL} * {scale}"


def _args(F_in=32, K=2, td=True, bu=True, C=4):
    return argparse.Namespace(input_features=F_in, hidden_features=64, output_features=64, num_class=C, edge_num=K,
                              edge_infer_td=td, edge_infer_bu=bu, device=DEV)


def _randomised(module, seed):
    """Parameters away from the default init, as the fixtures' (with it every edge_pred is ~0.506)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, m in module.named_modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                c = m.num_features
                m.running_mean.copy_(torch.randn(c, generator=g) * 0.3)
                m.running_var.copy_(torch.rand(c, generator=g) * 1.5 + 0.5)
                m.weight.copy_(torch.rand(c, generator=g) + 0.5)
                m.bias.copy_(torch.randn(c, generator=g) * 0.3)
                m.num_batches_tracked.fill_(seed)
            elif isinstance(m, torch.nn.Conv1d):
                m.weight.mul_(3.0)
                if m.bias is not None:
                    m.bias.copy_(torch.randn(1, generator=g) * 0.2)
            elif name in ("fc1", "fc2"):
                m.weight.mul_(4.0)
    return module


def _state64(module, prefix=""):
    return {prefix + k: v.detach().cpu() for k, v in module.state_dict().items()}


def _direction(K):
    """A fresh randomised direction in train mode on the device, and its state before any forward."""
    from bigcn_amd.ebgcn import TDrumorGCN
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(200 + K)
        m = _randomised(TDrumorGCN(_args(K=K)), 200 + K).train()
    return m.to(DEV), _state64(m, "TDrumorGCN.")


@functools.lru_cache(maxsize=None)
def _inputs(E, K, N):
    g = torch.Generator().manual_seed(1000 * E + 10 * K + N)
    h = torch.randn(N, 64, generator=g) * 0.7
    ei = torch.randint(0, N, (2, E), generator=g)
    ei[0, 0] = 0                # a row index of 0: reads the LAST node
    if E > 2:
        ei[1, 1] = 0
        ei[1, 2] = ei[0, 2]     # a == b: D has an exact-zero diagonal, sign(0) = 0
    return h, ei, torch.randn(E, 64, generator=g), torch.randn(E, generator=g), torch.randn((), generator=g)


@functools.lru_cache(maxsize=None)
def _reference(E, K, N):
    """The fp64 restatement of one shape, computed once: outputs, gradients, buffers."""
    _, sd = _direction(K)
    h, ei, noise, c, g = _inputs(E, K, N)
    sd64 = T.with_grad(sd, torch.float64)
    h64 = h.double().requires_grad_(True)
    new = {}
    loss, pred = T.edge_infer_train(sd64, "TDrumorGCN", h64, ei, noise.double(), new)
    have, none, (gh,) = T.grads_of((c.double() * pred).sum() + g.double() * loss, sd64, [h64])
    return loss.detach(), pred.detach(), gh, have, none, new


def _run(m, E, K, N):
    from bigcn_amd import edge_infer_train
    h, ei, noise, c, g = _inputs(E, K, N)
    hd = h.to(DEV).requires_grad_(True)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    loss, pred = edge_infer_train(hd, ei.to(DEV), m, noise=noise.to(DEV), status=status)
    params = dict(m.named_parameters())
    names = [k for k in params if k.startswith("sim_network.") or k == "fc1.weight"]
    grads = torch.autograd.grad((c.to(DEV) * pred).sum() + g.to(DEV) * loss, [hd] + [params[k] for k in names])
    return loss, pred, grads[0], dict(zip(names, grads[1:])), status


@pytest.mark.parametrize("E,K,N", SHAPES)
def test_edge_infer_train_matches_restatement(E, K, N):
    """(1, 1, 50): BatchNorm over 64 values; (33, 2, 50): one edge tile + 1; (33, 3, 2): every index
    wraps and many a == b; (1000, 3, 50): many blocks' partials, ~40 edge ends per node in dh;
    (2100, 1, 2): two hubs of ~2100 edge ends each, more than one LDS chunk of the dh ranking."""
    m, sd = _direction(K)
    rloss, rpred, rgh, rhave, rnone, rnew = _reference(E, K, N)
    loss, pred, gh, grads, status = _run(m, E, K, N)
    assert int(status.item()) == 0
    assert loss.dim() == 0 and pred.shape == (E,) and loss.grad_fn is not None and pred.grad_fn is not None
    _close(pred, rpred, f"edge_pred E={E} K={K} N={N}")
    _close(loss, rloss, "edge_loss")
    _close(gh, rgh, "d h")
    assert sorted("TDrumorGCN." + k for k in grads) == sorted(rhave)
    for k, g in grads.items():
        _close(g, rhave["TDrumorGCN." + k], "d " + k)
    # the five norms' buffers after the forward
    after = _state64(m, "TDrumorGCN.")
    assert len(rnew) == 15
    for k, v in rnew.items():
        if v.is_floating_point():
            _close(after[k], v, k)
        else:
            assert int(after[k]) == int(v) == int(sd[k]) + 1, k
    # nothing else moved
    for k, v in sd.items():
        if k not in rnew:
            assert torch.equal(after[k], v), k


def test_bayesian_networks_and_fc2_get_no_gradient():
    m, _ = _direction(2)
    m.zero_grad(set_to_none=True)
    from bigcn_amd import edge_infer_train
    h, ei, noise, c, g = _inputs(33, 2, 50)
    hd = h.to(DEV).requires_grad_(True)
    loss, pred = edge_infer_train(hd, ei.to(DEV), m, noise=noise.to(DEV))
    ((c.to(DEV) * pred).sum() + loss).backward()
    got = sorted(k for k, p in m.named_parameters() if p.grad is not None)
    assert got == sorted(k for k, _ in m.named_parameters() if k.startswith("sim_network.") or k == "fc1.weight")
    assert len(got) == 6 and hd.grad is not None
    for k, p in m.named_parameters():
        if k.startswith(("W_mean", "W_bias", "B_mean", "B_bias", "fc2")):
            assert p.grad is None, k


def test_two_runs_give_equal_bits():
    E, K, N = 1000, 3, 50
    a = _run(_direction(K)[0], E, K, N)
    b = _run(_direction(K)[0], E, K, N)
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(x, y)
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), k


def test_own_noise_draw_and_refusals():
    from bigcn_amd import edge_infer_train
    m, _ = _direction(2)
    h, ei, _, _, _ = _inputs(33, 2, 50)
    gen = torch.Generator(device=DEV).manual_seed(5)
    l1, p1 = edge_infer_train(h.to(DEV), ei.to(DEV), m, generator=gen)
    gen.manual_seed(5)
    l2, p2 = edge_infer_train(h.to(DEV), ei.to(DEV), m, generator=gen)
    assert torch.equal(p1, p2) and torch.equal(l1, l2) and bool(torch.isfinite(l1))
    with pytest.raises(ValueError):
        edge_infer_train(h.to(DEV), torch.zeros(2, 0, dtype=torch.int64, device=DEV), m)
    m.W_bias.W_biasnorm0.momentum = None
    with pytest.raises(ValueError, match="momentum"):
        edge_infer_train(h.to(DEV), ei.to(DEV), m)
    # the module method dispatches on the mode; ops.edge_infer still refuses a training module
    from bigcn_amd import edge_infer
    m2, _ = _direction(2)
    loss, pred = m2.edge_infer(h.to(DEV), ei.to(DEV))
    assert loss is not None and loss.dim() == 0 and pred.shape == (33,)
    with pytest.raises(NotImplementedError, match="inference-only"):
        edge_infer(h.to(DEV), ei.to(DEV), m2)
    assert m2.eval().edge_infer(h.to(DEV), ei.to(DEV))[0] is None


def test_out_of_range_index_is_flagged_zeroed_and_excluded():
    """Three bad edges among 40: flagged, edge_pred 0, and everything else is what the restatement
    gives on the 37 remaining edges (statistics, loss, gradients)."""
    from bigcn_amd import edge_infer_train
    K, N, E = 2, 50, 40
    m, sd = _direction(K)
    h, ei, noise, c, g = _inputs(E, K, N)
    ei = ei.clone()
    bad = torch.tensor([3, 17, 39])
    ei[0, 3], ei[1, 17], ei[0, 39] = N, -1, N + 7
    keep = torch.ones(E, dtype=torch.bool)
    keep[bad] = False
    hd = h.to(DEV).requires_grad_(True)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    loss, pred = edge_infer_train(hd, ei.to(DEV), m, noise=noise.to(DEV), status=status)
    params = dict(m.named_parameters())
    names = [k for k in params if k.startswith("sim_network.") or k == "fc1.weight"]
    grads = torch.autograd.grad((c.to(DEV) * pred).sum() + g.to(DEV) * loss, [hd] + [params[k] for k in names])
    assert int(status.item()) & 1
    assert bool((pred[bad.to(DEV)] == 0).all())
    sd64 = T.with_grad(sd, torch.float64)
    h64 = h.double().requires_grad_(True)
    new = {}
    rloss, rpred = T.edge_infer_train(sd64, "TDrumorGCN", h64, ei[:, keep], noise[keep].double(), new)
    have, _, (gh,) = T.grads_of((c[keep].double() * rpred).sum() + g.double() * rloss, sd64, [h64])
    _close(pred[keep.to(DEV)], rpred, "edge_pred of the valid edges")
    _close(loss, rloss, "edge_loss over the valid edges")
    _close(grads[0], gh, "d h")
    for k, gr in zip(names, grads[1:]):
        _close(gr, have["TDrumorGCN." + k], "d " + k)
    after = _state64(m, "TDrumorGCN.")
    for k, v in new.items():
        if v.is_floating_point():
            _close(after[k], v, k)


def test_a_batch_without_a_valid_edge_blends_nothing():
    from bigcn_amd import edge_infer_train
    m, sd = _direction(2)
    h, ei, noise, _, _ = _inputs(33, 2, 50)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    loss, pred = edge_infer_train(h.to(DEV), (ei + 50).to(DEV), m, noise=noise.to(DEV), status=status)
    assert int(status.item()) & 1 and bool((pred == 0).all()) and float(loss) == 0.0
    after = _state64(m, "TDrumorGCN.")
    for k, v in sd.items():
        assert torch.equal(after[k], v), k


@pytest.mark.parametrize("path", EDGE_FIXTURES, ids=EDGE_NAMES)
def test_edge_fixtures(path):
    """The reference's own fp32 results (restatement-vs-reference error ~2e-6, far below the bar)."""
    from bigcn_amd import edge_infer_train
    from bigcn_amd.ebgcn import TDrumorGCN
    z = T.load_npz(path)
    m = TDrumorGCN(_args(F_in=64, K=int(z["edge_num"])))
    m.load_state_dict({k[len("TDrumorGCN."):]: v for k, v in T.group(z, "sd").items()}, strict=True)
    m = m.to(DEV).train()
    hd = z["h"].to(DEV).requires_grad_(True)
    loss, pred = edge_infer_train(hd, z["edge_index"].to(DEV), m, noise=z["noise"].to(DEV))
    ((z["c"].to(DEV) * pred).sum() + z["g"].to(DEV) * loss).backward()
    _close(pred, z["edge_pred"], "edge_pred")
    _close(loss, z["edge_loss"], "edge_loss")
    _close(hd.grad, z["grad_h"], "d h")
    want = T.group(z, "grad")
    for k, p in m.named_parameters():
        if p.grad is not None:
            _close(p.grad, want["TDrumorGCN." + k], "d " + k)
        else:
            assert not (k.startswith("sim_network.") or k == "fc1.weight"), k
    after = _state64(m, "TDrumorGCN.")
    for k, v in T.group(z, "after").items():
        if v.is_floating_point():
            _close(after[k], v, k)
        else:
            assert int(after[k]) == int(v), k


def _model_case(td=True, bu=True):
    from bigcn_amd import EBGCN
    z = T.load_npz(MODEL_FIXTURE)
    model = EBGCN(_args(F_in=64, K=int(z["edge_num"]), td=td, bu=bu))
    model.load_state_dict(T.group(z, "sd"), strict=True)
    model = model.to(DEV).train()
    data = argparse.Namespace(**{k: z[k].to(DEV) for k in ("x", "edge_index", "BU_edge_index", "batch", "rootindex", "y")})
    return z, model, data


def test_train_forward_matches_restatement_on_the_model_fixture():
    z, model, data = _model_case()
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
    _close(logp, z["logp"], "log-probs vs the reference's")
    got = {k: p.grad for k, p in model.named_parameters()}
    assert sorted(k for k, g in got.items() if g is None) == none and len(none) == 42
    for k, g in have.items():
        _close(got[k], g, "d " + k)
    after = _state64(model)
    for k, v in new.items():
        if v.is_floating_point():
            _close(after[k], v, k)
        else:
            assert int(after[k]) == int(v), k
    with pytest.raises(NotImplementedError, match="inference-only"):
        model(data)


def test_train_forward_with_a_direction_off_and_a_one_node_batch():
    z, model, data = _model_case(bu=False)
    noise = (z["noise_td"].to(DEV), None)
    logp, td, bu = model.train_forward(data, noise=noise)
    assert bu is None and td is not None
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in T.group(z, "sd").items()}
    rlogp, rtd, rbu = T.forward_train(sd64, z["x"].double(), z["edge_index"], z["BU_edge_index"], z["batch"],
                                      z["rootindex"], (z["noise_td"].double(), None), infer_bu=False)
    assert rbu is None
    _close(logp, rlogp, "log-probs, BU conv2 unweighted")
    _close(td, rtd, "TD edge loss")
    # one node, no edges: bn1 is skipped (and untouched), both directions run without edge inference
    z, model, data = _model_case(td=False, bu=False)
    before = _state64(model)
    one = argparse.Namespace(x=data.x[:1], edge_index=data.edge_index[:, :0], BU_edge_index=data.edge_index[:, :0],
                             batch=data.batch[:1], rootindex=data.rootindex[:1])
    logp, td, bu = model.train_forward(one)
    assert td is None and bu is None and logp.shape == (1, 4)
    rlogp, _, _ = T.forward_train(sd64, z["x"][:1].double(), z["edge_index"][:, :0], z["edge_index"][:, :0],
                                  z["batch"][:1], z["rootindex"][:1], (None, None), infer_td=False, infer_bu=False)
    _close(logp, rlogp, "log-probs of a one-node batch")
    after = _state64(model)
    for k in before:
        assert torch.equal(before[k], after[k]), k
