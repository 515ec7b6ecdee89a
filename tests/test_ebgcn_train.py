"""CPU checks of the EBGCN training path: the plain-torch restatement (tests/ebgcn_train_ref.py)
agrees in fp32 with what the reference's own classes computed in train() mode (fixtures of
tools/gen_ebgcn_train_golden.py), the new C entry points refuse bad arguments before any device
work, and the module has ``train_forward`` while ``forward`` still refuses training mode.

One difference from the reference is deliberate and pinned here.  With current PyTorch the
reference gives ``fc2.weight`` a gradient (KLDivLoss differentiates its target) and the four
Bayesian networks all-zero gradients (``torch.normal``'s derivative is zeros).  This project treats
``p_y`` as a constant target: those 21 parameters get no gradient at all.  Every other gradient is
the reference's."""
import argparse
import ctypes
import glob
import os
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

import ebgcn_train_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE_FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "train_ebgcn_edge_*.npz")))
EDGE_NAMES = [os.path.basename(p)[len("train_ebgcn_edge_"):-len(".npz")] for p in EDGE_FIXTURES]
MODEL_FIXTURE = os.path.join(ROOT, "tests", "golden", "train_ebgcn_model.npz")

# Restatement (fp32) vs the reference-produced fp32 fixtures, per tensor max|a - b| / max|b|:
# the arithmetic is the same and only the order of the sums differs (einsum against Conv1d, the
# BatchNorm's own reductions).  Measured once over the three fixtures, the largest per kind:
#   outputs (edge_pred, edge_loss, log-probs)   2.08e-7
#   gradients (h and every parameter)           1.75e-6
#   updated buffers                             9.13e-8
# The bar is ten times the largest.
RESTATEMENT_BAR = 1.75e-5


def _err(got, want):
    got, want = got.detach().double(), want.double()
    return float((got - want).abs().max()) / float(want.abs().max())


def _bayesian(key):
    return ".fc2." in key or ".W_mean." in key or ".W_bias." in key or ".B_mean." in key or ".B_bias." in key


def test_fixture_set():
    assert EDGE_NAMES == ["k2", "k3"] and os.path.exists(MODEL_FIXTURE)
    for p in EDGE_FIXTURES + [MODEL_FIXTURE]:
        assert os.path.getsize(p) < (1 << 20)


@pytest.mark.parametrize("path", EDGE_FIXTURES, ids=EDGE_NAMES)
def test_edge_fixture_conditions(path):
    """The conditions that keep a wrong kernel from passing, on the reference's stored values."""
    z = T.load_npz(path)
    pred, std, ei = z["edge_pred"], z["std"], z["edge_index"]
    assert float(pred.min()) <= 0.2 and float(pred.max()) >= 0.8
    assert float((std == 0).float().mean()) >= 0.1 and float((std > 0).float().mean()) >= 0.1
    assert int(z["pre_sign_counts"].min()) > 0
    assert float(z["target_gap"]) > 0.05
    assert bool((ei[0] == ei[1]).any()) and bool((ei == 0).any())
    # what the reference leaves without information: zeros for the four Bayesian networks
    assert len(z["zero_grad"]) == 20


@pytest.mark.parametrize("path", EDGE_FIXTURES, ids=EDGE_NAMES)
def test_restatement_matches_reference_edge_fixture(path):
    z = T.load_npz(path)
    sd = T.with_grad(T.group(z, "sd"), torch.float32)
    h = z["h"].clone().requires_grad_(True)
    new, det = {}, {}
    loss, pred = T.edge_infer_train(sd, "TDrumorGCN", h, z["edge_index"], z["noise"], new, det)
    worst = {"out": max(_err(pred, z["edge_pred"]), _err(loss, z["edge_loss"])), "grad": 0.0, "buf": 0.0}
    # the stored conditions are the restatement's too
    assert float((det["std"] == 0).float().mean()) >= 0.1 and float((det["p_y"] - det["softmax_p"]).abs().max()) > 0.05
    assert bool((det["pre_activation"] > 0).any()) and bool((det["pre_activation"] < 0).any())
    have, none, (gh,) = T.grads_of((z["c"] * pred).sum() + z["g"] * loss, sd, [h])
    worst["grad"] = _err(gh, z["grad_h"])
    want = T.group(z, "grad")
    for k, g in have.items():
        worst["grad"] = max(worst["grad"], _err(g, want[k]))
    # gradients reach the sim network and fc1 only
    assert sorted(have) == sorted(k for k in want if not _bayesian(k))
    assert len(have) == 6 and all(".sim_network." in k or k.endswith("fc1.weight") for k in have)
    assert sorted(k for k in none if _bayesian(k)) == sorted(k for k in sd if _bayesian(k) and sd[k].requires_grad)
    for k, v in T.group(z, "after").items():
        if v.is_floating_point():
            worst["buf"] = max(worst["buf"], _err(new[k], v))
        else:
            assert int(new[k]) == int(v) == int(sd[k]) + 1
    print(f"restatement vs reference: {worst}")
    assert max(worst.values()) <= RESTATEMENT_BAR


def test_restatement_matches_reference_model_fixture():
    z = T.load_npz(MODEL_FIXTURE)
    sd = T.with_grad(T.group(z, "sd"), torch.float32)
    new = {}
    logp, td, bu = T.forward_train(sd, z["x"], z["edge_index"], z["BU_edge_index"], z["batch"], z["rootindex"],
                                   (z["noise_td"], z["noise_bu"]), new_buffers=new)
    worst = {"out": max(_err(logp, z["logp"]), _err(td, z["td_loss"]), _err(bu, z["bu_loss"])), "grad": 0.0, "buf": 0.0}
    have, none, _ = T.grads_of(F.nll_loss(logp, z["y"]) + 0.2 * (td + bu), sd)
    want = T.group(z, "grad")
    assert sorted(have) == sorted(k for k in want if not _bayesian(k))
    assert sorted(none) == sorted(k for k in want if _bayesian(k)) and len(none) == 42
    for k, g in have.items():
        worst["grad"] = max(worst["grad"], _err(g, want[k]))
    for k, v in T.group(z, "after").items():
        if v.is_floating_point():
            worst["buf"] = max(worst["buf"], _err(new[k], v))
        else:
            assert int(new[k]) == int(v)
    print(f"restatement vs reference (model): {worst}")
    assert max(worst.values()) <= RESTATEMENT_BAR


def test_c_entry_points_refuse_bad_arguments_without_a_gpu():
    """rc -1 and a message, before any device work (the pointers are never dereferenced)."""
    from bigcn_amd import _lib
    lib = _lib.load_library()
    p = 4096   # a non-null, 16-byte aligned stand-in for every pointer
    N, E = 10, 5
    ws = lib.bgcn_edge_infer_train_workspace_size(N, E)
    assert ws >= 4 * (4 * E * 64 + 2 * E * 64)
    assert lib.bgcn_edge_infer_train_workspace_size(N, 0) == 0

    def fill(a, hid=64, K=2, E=E):
        for name, ctype in a._fields_:
            if ctype is ctypes.c_void_p:
                setattr(a, name, p)
        a.ldh, a.num_nodes, a.hid, a.num_edges, a.edge_num = 64, N, hid, E, K
        return a

    def fwd(ws_bytes=ws, **kw):
        a = fill(_lib.EdgeTrainFwdArgs(), **kw)
        for net in a.net:
            net.conv_w = net.norm_weight = net.norm_bias = net.out_w = net.out_b = p
            net.eps = 1e-5
        return lib.bgcn_edge_infer_train_fwd(ctypes.addressof(a), p, ws_bytes, None)

    def bwd(ws_bytes=ws, **kw):
        a = fill(_lib.EdgeTrainBwdArgs(), **kw)
        a.ldd = 64
        a.sim.conv_w = a.sim.norm_weight = a.sim.norm_bias = a.sim.out_w = p
        return lib.bgcn_edge_infer_train_bwd(ctypes.addressof(a), p, ws_bytes, None)

    for call in (fwd, bwd):
        assert call(hid=32) == -1 and b"hidden size must be 64" in lib.bgcn_last_error()
        assert call(K=0) == -1 and b"edge_num" in lib.bgcn_last_error()
        assert call(K=9) == -1 and b"edge_num" in lib.bgcn_last_error()
        assert call(E=0) == -1 and b"at least one edge" in lib.bgcn_last_error()
        assert call(ws_bytes=256) == -1 and b"workspace too small" in lib.bgcn_last_error()
    assert lib.bgcn_edge_infer_train_fwd(None, p, ws, None) == -1
    assert lib.bgcn_abi_version() == 12


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_ctypes_structs_match_the_header(tmp_path):
    from bigcn_amd import _lib
    structs = {"bgcn_edge_net": _lib.EdgeNet, "bgcn_edge_train_fwd_args": _lib.EdgeTrainFwdArgs,
               "bgcn_edge_train_bwd_args": _lib.EdgeTrainBwdArgs}
    header = os.path.join(ROOT, "include", "bgcn.h")
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{header}"', "int main(void) {"]
    for cname, py in structs.items():
        lines.append(f'printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for fname, _ in py._fields_:
            lines.append(f'printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0; }")
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {tuple(line.split()[:2]): int(line.split()[2]) for line in out if line}
    for cname, py in structs.items():
        assert got[(cname, "sizeof")] == ctypes.sizeof(py), cname
        for fname, _ in py._fields_:
            assert got[(cname, fname)] == getattr(py, fname).offset, (cname, fname)


def test_train_forward_exists_and_forward_still_refuses():
    import bigcn_amd
    from bigcn_amd import EBGCN, _lib
    assert "edge_infer_train" in bigcn_amd.__all__ and callable(bigcn_amd.edge_infer_train)
    for name in ("bgcn_edge_infer_train_workspace_size", "bgcn_edge_infer_train_fwd", "bgcn_edge_infer_train_bwd"):
        assert name in _lib.EXPORTED_SYMBOLS and name in _lib._SIGS
    args = argparse.Namespace(input_features=32, hidden_features=64, output_features=64, num_class=4, edge_num=2,
                              edge_infer_td=True, edge_infer_bu=True, device="cpu")
    model = EBGCN(args).train()
    assert callable(model.train_forward)
    with pytest.raises(NotImplementedError, match="inference-only"):
        model(argparse.Namespace())
    with pytest.raises(NotImplementedError, match="train_forward"):
        model(argparse.Namespace())
    # the op refuses what it cannot do before touching a device
    d = model.TDrumorGCN
    d.sim_network.sim_valnorm0.momentum = None
    with pytest.raises(ValueError, match="momentum"):
        bigcn_amd.edge_infer_train(torch.zeros(4, 64), torch.zeros(2, 3, dtype=torch.int64), d)
