"""CPU checks of the EBGCN inference path: the module's state_dict is the reference's (strict
load of reference-produced fixtures), the plain-torch restatement (tests/ebgcn_ref.py) agrees
with what the reference's own classes computed, and the new C entry points refuse bad
arguments before any device work."""
import argparse
import glob
import os

import pytest
import torch

import ebgcn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "ebgcn_*.npz")))
NAMES = [os.path.basename(p)[len("ebgcn_"):-len(".npz")] for p in FIXTURES]

# Restatement (fp32) vs the reference-produced fp32 fixtures: the arithmetic is the same and only
# the summation order differs (einsum / matmul against Conv1d and Linear, the folded order of
# the BatchNorm terms).  Measured once over the four fixtures: max |restatement - fixture| is
# 2.98e-7 for edge_pred (values in [0, 1]) and 1.19e-7 for the log-probs (|logp| up to 2.1); the
# bar is ten times the larger of the two.
RESTATEMENT_BAR = 2.98e-6


def _args(cfg, F):
    return argparse.Namespace(input_features=F, hidden_features=64, output_features=64, num_class=cfg["num_class"],
                              edge_num=cfg["edge_num"], edge_infer_td=bool(cfg["edge_infer_td"]),
                              edge_infer_bu=bool(cfg["edge_infer_bu"]), device="cpu")


def test_fixture_set():
    assert NAMES == ["mixed", "nobu", "single", "star40"]


@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_reference_state_dict_loads_strictly(path):
    from bigcn_amd import EBGCN
    sd, b, cfg, _ = R.load_fixture(path)
    assert len(sd) == 104
    model = EBGCN(_args(cfg, b["x"].size(1)))
    own = model.state_dict()
    assert list(own) == list(sd)                      # key for key, in order
    for k in sd:
        assert own[k].shape == sd[k].shape and own[k].dtype == sd[k].dtype, k
    model.load_state_dict(sd, strict=True)
    for k, v in model.state_dict().items():
        assert torch.equal(v, sd[k]), k


@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_restatement_matches_reference_fixture(path):
    """fp32 restatement vs the reference's fp32 outputs.  Measured maxima (all fixtures):
    edge_pred 2.98e-7, log-probs 1.19e-7; bar RESTATEMENT_BAR = 2.98e-6 (10x the larger)."""
    sd, b, cfg, exp = R.load_fixture(path)
    logp, td, bu = R.fixture_forward(sd, b, cfg)
    # the conditions on the fixtures themselves: edge weights that vary, decisions that are not ties
    preds = torch.cat((exp["td_edge_pred"], exp["bu_edge_pred"]))
    if b["edge_index"].size(1):
        assert preds.numel() and float(preds.min()) <= 0.2 and float(preds.max()) >= 0.8
    top = exp["logp"].sort(dim=1).values
    assert float((top[:, -1] - top[:, -2]).min()) > 1e-3
    for name, got, flag in (("td", td, cfg["edge_infer_td"]), ("bu", bu, cfg["edge_infer_bu"])):
        want = exp[name + "_edge_pred"]
        if not flag:
            assert got is None and want.numel() == 0
            continue
        assert got.shape == want.shape == (b["edge_index"].size(1),)
        err = float((got - want).abs().max()) if want.numel() else 0.0
        print(f"{name}_edge_pred max err {err:.3e}")
        assert err <= RESTATEMENT_BAR
    err = float((logp - exp["logp"]).abs().max())
    print(f"logp max err {err:.3e} (max |logp| {float(exp['logp'].abs().max()):.3f})")
    assert err <= RESTATEMENT_BAR
    assert torch.equal(logp.argmax(1), exp["logp"].argmax(1))


def test_training_mode_is_refused():
    from bigcn_amd import EBGCN
    cfg = {"num_class": 4, "edge_num": 2, "edge_infer_td": 1, "edge_infer_bu": 1}
    model = EBGCN(_args(cfg, 32)).train()
    with pytest.raises(NotImplementedError, match="inference-only"):
        model(argparse.Namespace())
    with pytest.raises(NotImplementedError, match="inference-only"):
        model.TDrumorGCN(argparse.Namespace())


def test_unsupported_configurations_are_refused():
    from bigcn_amd import EBGCN
    base = {"num_class": 4, "edge_num": 2, "edge_infer_td": 1, "edge_infer_bu": 1}
    for change in ({"edge_num": 0}, {"edge_num": 9}, {"num_class": 17}):
        with pytest.raises(ValueError):
            EBGCN(_args({**base, **change}, 32))
    with pytest.raises(ValueError):
        EBGCN(_args(base, 30))                        # F not a multiple of 4
    a = _args(base, 32)
    a.hidden_features = 32
    with pytest.raises(ValueError):
        EBGCN(a)


def test_c_entry_points_refuse_bad_arguments_without_a_gpu():
    """rc -1 and a message, before any device work (the pointers are never dereferenced)."""
    from bigcn_amd import _lib
    lib = _lib.load_library()
    p = 4096   # a non-null, 16-byte aligned stand-in for every pointer

    def edge(hid=64, K=2, h=p, pred=p, status=p):
        return lib.bgcn_edge_infer(h, 64, 10, hid, p, 5, p, p, p, p, p, p, K, pred, status, None)

    assert edge(hid=32) == -1 and b"hidden size must be 64" in lib.bgcn_last_error()
    assert edge(K=0) == -1 and b"edge_num" in lib.bgcn_last_error()
    assert edge(K=9) == -1 and b"edge_num" in lib.bgcn_last_error()
    assert edge(h=None) == -1 and b"null pointer" in lib.bgcn_last_error()
    assert edge(pred=None) == -1 and b"null pointer" in lib.bgcn_last_error()
    assert edge(status=None) == -1 and b"null pointer" in lib.bgcn_last_error()

    ws = lib.bgcn_ebgcn_conv2_lin_workspace_size(10, 2, 32)
    assert ws >= 4 * (2 * 32 + 10 * 64 + 2 * 64)

    def lin(F=32, hid=64, h1=p, ws_ptr=p, ws_bytes=ws, z2=p):
        return lib.bgcn_ebgcn_conv2_lin(h1, 64, p, max(F, 4), p, p, 10, 2, F, hid, p, p, p, z2, 64, p, ws_ptr,
                                        ws_bytes, None)

    assert lin(hid=128) == -1 and b"hidden size must be 64" in lib.bgcn_last_error()
    assert lin(F=30) == -1 and b"multiple of 4" in lib.bgcn_last_error()
    assert lin(F=0) == -1 and b"multiple of 4" in lib.bgcn_last_error()
    assert lin(h1=None) == -1 and b"null pointer" in lib.bgcn_last_error()
    assert lin(z2=None) == -1 and b"null pointer" in lib.bgcn_last_error()
    assert lin(ws_ptr=None) == -1 and b"workspace" in lib.bgcn_last_error()
    assert lin(ws_bytes=16) == -1 and b"workspace" in lib.bgcn_last_error()
    assert lib.bgcn_bn_fold(None, p, p, p, 1e-5, 64, p, p, None) == -1 and b"null pointer" in lib.bgcn_last_error()
    assert lib.bgcn_bn_fold(p, p, p, p, 1e-5, 0, p, p, None) == -1


def test_binding_lists_the_new_entry_points():
    from bigcn_amd import _lib
    for name in ("bgcn_bn_fold", "bgcn_edge_infer", "bgcn_ebgcn_conv2_lin_workspace_size", "bgcn_ebgcn_conv2_lin"):
        assert name in _lib.EXPORTED_SYMBOLS and name in _lib._SIGS
    import bigcn_amd
    assert "EBGCN" in bigcn_amd.__all__ and "edge_infer" in bigcn_amd.__all__
    assert _lib.BGCN_EDGE_INFER_TILE == 32
