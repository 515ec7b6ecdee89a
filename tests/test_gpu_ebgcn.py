"""GPU checks of the EBGCN inference path: the fp32 HIP kernels against the fp64 restatement
(tests/ebgcn_ref.py, itself pinned to reference-produced fixtures by tests/test_ebgcn.py).
Bar: the project's standing |a - b| <= 1e-4 max|b| per tensor."""
import argparse
import functools
import glob
import os

import pytest
import torch

import ebgcn_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "ebgcn_*.npz")))
NAMES = [os.path.basename(p)[len("ebgcn_"):-len(".npz")] for p in FIXTURES]
DEV = "cuda:0"
TOL = 1e-4


def _close(got, want, what):
    got, want = got.double().cpu(), want.double().cpu()
    assert got.shape == want.shape, what
    if want.numel() == 0:
        return
    err, scale = float((got - want).abs().max()), float(want.abs().max())
    print(f"{what}: max err {err:.3e}, max |ref| {scale:.3e}")
    assert err <= TOL * scale, f"{what}: {err} vs {TOL} * {scale}"


def _args(F=32, K=2, td=True, bu=True, C=4):
    return argparse.Namespace(input_features=F, hidden_features=64, output_features=64, num_class=C, edge_num=K,
                              edge_infer_td=td, edge_infer_bu=bu, device=DEV)


def _randomised(module, seed):
    """Parameters away from the default init (with it every edge_pred is ~0.506)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, m in module.named_modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                c = m.num_features
                m.running_mean.copy_(torch.randn(c, generator=g) * 0.3)
                m.running_var.copy_(torch.rand(c, generator=g) * 1.5 + 0.5)
                m.weight.copy_(torch.rand(c, generator=g) + 0.5)
                m.bias.copy_(torch.randn(c, generator=g) * 0.3)
            elif isinstance(m, torch.nn.Conv1d):
                m.weight.mul_(3.0)
                if m.bias is not None:
                    m.bias.copy_(torch.randn(1, generator=g) * 0.2)
            elif name == "fc1":
                m.weight.mul_(4.0)
    return module


@functools.lru_cache(maxsize=None)
def _direction(K):
    from bigcn_amd.ebgcn import TDrumorGCN
    with torch.random.fork_rng(devices=[]):      # the module's own init draws from the global generator
        torch.manual_seed(100 + K)
        m = _randomised(TDrumorGCN(_args(K=K)), 100 + K).eval()
    sd64 = {"TDrumorGCN." + k: (v.double() if v.is_floating_point() else v) for k, v in m.state_dict().items()}
    return m.to(DEV), sd64


@functools.lru_cache(maxsize=None)
def _nodes(N):
    return torch.randn(N, 64, generator=torch.Generator().manual_seed(N)) * 0.7


def _edges(E, N, seed):
    ei = torch.randint(0, N, (2, E), generator=torch.Generator().manual_seed(seed))
    if E:
        ei[0, 0] = 0            # a row index of 0: reads the LAST node
    if E > 1:
        ei[1, 1] = 0
    return ei


@pytest.mark.parametrize("E,K,N", [(1, 1, 50), (33, 2, 50), (33, 3, 2), (1000, 3, 50), (64, 2, 50), (31, 1, 7)])
def test_edge_infer_matches_restatement(E, K, N):
    """E = 33 is one edge tile (32) + 1; N = 2 makes every index wrap or hit node 0."""
    from bigcn_amd import edge_infer
    m, sd64 = _direction(K)
    h, ei = _nodes(N), _edges(E, N, E + K)
    got = edge_infer(h.to(DEV), ei.to(DEV), m, validate=True)
    assert got.shape == (E,) and got.dtype == torch.float32 and got.grad_fn is None
    want = R.edge_pred(sd64, "TDrumorGCN", h.double(), ei)
    assert float(want.max() - want.min()) > 0.1 or E < 8    # the reference values vary (N = 2: four distinct edges)
    _close(got, want, f"edge_pred E={E} K={K} N={N}")


def test_edge_infer_index_zero_reads_the_last_node():
    from bigcn_amd import edge_infer
    m, sd64 = _direction(2)
    N = 9
    h = _nodes(N)
    ei = torch.tensor([[0, 1, 0], [1, 0, 0]])
    got = edge_infer(h.to(DEV), ei.to(DEV), m, validate=True)
    # the same rows named without an index 0: id N is row N - 1, the last node
    want = R.edge_pred(sd64, "TDrumorGCN", h.double(), torch.tensor([[N, 1, N], [1, N, N]]))
    _close(got, want, "index 0 wraps to the last node")


def test_edge_infer_empty_and_deterministic():
    from bigcn_amd import edge_infer
    m, _ = _direction(2)
    h = _nodes(50).to(DEV)
    out = edge_infer(h, torch.zeros(2, 0, dtype=torch.int64, device=DEV), m)
    assert out.shape == (0,) and out.dtype == torch.float32
    ei = _edges(1000, 50, 5).to(DEV)
    a, b = edge_infer(h, ei, m), edge_infer(h, ei, m)
    assert torch.equal(a, b)


def test_edge_infer_out_of_range_index_is_flagged_not_read():
    from bigcn_amd import edge_infer
    m, sd64 = _direction(2)
    h = _nodes(50)
    ei = _edges(40, 50, 9)
    bad = ei.clone()
    bad[1, 7], bad[0, 20] = 50, -1
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = edge_infer(h.to(DEV), bad.to(DEV), m, status=status)
    assert int(status.item()) == 1
    assert float(got[7]) == 0.0 and float(got[20]) == 0.0
    keep = torch.ones(40, dtype=torch.bool)
    keep[7] = keep[20] = False
    _close(got.cpu()[keep], R.edge_pred(sd64, "TDrumorGCN", h.double(), ei)[keep], "valid edges beside bad ones")
    with pytest.raises(IndexError):
        edge_infer(h.to(DEV), bad.to(DEV), m, validate=True)


@pytest.mark.parametrize("F,B", [(32, 1), (32, 5), (300, 5), (300, 1)])
def test_conv2_lin_matches_restatement(F, B):
    from bigcn_amd.ops import ebgcn_conv2_lin
    g = torch.Generator().manual_seed(F + B)
    sizes = [7, 70, 3, 11, 40][:B]
    N = sum(sizes)
    batch = torch.repeat_interleave(torch.arange(B), torch.tensor(sizes))
    offs = torch.cumsum(torch.tensor([0] + sizes[:-1]), 0)
    rootindex = offs + torch.tensor([s // 2 for s in sizes])      # roots inside their trees, not first
    h1 = torch.randn(N, 64, generator=g)
    x = (torch.rand(N, F, generator=g) < 0.2).float() * torch.randint(1, 4, (N, F), generator=g)
    w2 = torch.randn(64, 64 + F, generator=g) * 0.2
    bn = _randomised(torch.nn.Sequential(torch.nn.BatchNorm1d(64 + F)), F)[0].eval()
    sd64 = {"bn1." + k: v.double() for k, v in bn.state_dict().items() if v.is_floating_point()}
    cat = torch.cat((h1, x[rootindex[batch]]), 1).double()
    want = torch.relu(R.bn_eval(cat, sd64, "bn1")) @ w2.double().t()
    got = ebgcn_conv2_lin(h1.to(DEV), x.to(DEV), batch.to(DEV), rootindex.to(DEV), w2.to(DEV), bn.to(DEV),
                          validate=True)
    _close(got, want, f"z2 F={F} B={B}")
    # bn1 skipped (what a one-node batch takes)
    got = ebgcn_conv2_lin(h1.to(DEV), x.to(DEV), batch.to(DEV), rootindex.to(DEV), w2.to(DEV), None, validate=True)
    _close(got, torch.relu(cat) @ w2.double().t(), f"z2 without bn1 F={F} B={B}")


@functools.lru_cache(maxsize=None)
def _fixture_reference(path):
    sd, b, cfg, exp = R.load_fixture(path, torch.float64)
    return R.fixture_forward(sd, b, cfg), exp


@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_eval_forward_matches_restatement_on_fixtures(path):
    from bigcn_amd import EBGCN
    from bigcn_amd.data import Batch
    sd, b, cfg, _ = R.load_fixture(path)
    (want_logp, want_td, want_bu), exp = _fixture_reference(path)
    model = EBGCN(_args(b["x"].size(1), cfg["edge_num"], bool(cfg["edge_infer_td"]), bool(cfg["edge_infer_bu"]),
                        cfg["num_class"]))
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV).eval()
    data = Batch(num_graphs=int(b["rootindex"].numel()), **b).to(DEV)
    logp, td_loss, bu_loss = model(data)
    assert td_loss is None and bu_loss is None
    assert logp.grad_fn is None and not logp.requires_grad
    for name, got, want in (("td", model.last_edge_pred[0], want_td), ("bu", model.last_edge_pred[1], want_bu)):
        if want is None:
            assert got is None
        else:
            _close(got, want, f"{name}_edge_pred")
    _close(logp, want_logp, "log-probs")
    assert torch.equal(logp.argmax(1).cpu(), want_logp.argmax(1))
    assert torch.equal(logp.argmax(1).cpu(), exp["logp"].argmax(1))    # and the reference's own decision


def test_single_direction_module_and_training_mode():
    from bigcn_amd import EBGCN
    from bigcn_amd.data import Batch
    path = FIXTURES[NAMES.index("mixed")]
    sd, b, cfg, _ = R.load_fixture(path)
    model = EBGCN(_args(b["x"].size(1), cfg["edge_num"]))
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV).eval()
    data = Batch(num_graphs=int(b["rootindex"].numel()), **b).to(DEV)
    sd64, b64, _, _ = R.load_fixture(path, torch.float64)
    want, _ = R.direction(sd64, "BUrumorGCN", b64["x"], b64["BU_edge_index"], b64["batch"], b64["rootindex"], True)
    out, loss = model.BUrumorGCN(data)
    assert loss is None and out.grad_fn is None
    _close(out, want, "BU readout")
    model.train()
    with pytest.raises(NotImplementedError, match="inference-only"):
        model(data)
