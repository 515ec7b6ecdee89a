"""CPU checks of the train-mode bn1 + conv2 lin without the dense concat: in fp64 the factored
restatement (tests/ebgcn_bn1_ref.py: per-tree weighted statistics, the folded forward, the closed-form
backward) equals the dense one (``ebgcn_train_ref.bn_train`` over the materialised concat, relu,
``F.linear``, autograd) to 1e-12 relative, on the kernel tests' shapes and on the trained-model fixture
through ``forward_train``.  This pins the algebra; it does not depend on the kernels.  The new C entry
points refuse bad arguments before any device work."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

import ebgcn_bn1_ref as R
import ebgcn_train_ref as T
from oracle import bigcn_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_FIXTURE = os.path.join(ROOT, "tests", "golden", "train_ebgcn_model.npz")
BAR = 1e-12


def _rel(got, want):
    return float((got.double() - want.double()).abs().max() / want.double().abs().max().clamp(min=1e-300))


@pytest.mark.parametrize("momentum", [T.BN_MOMENTUM, None], ids=["momentum", "cumulative"])
@pytest.mark.parametrize("N,B,F_in", R.SHAPES)
def test_factored_form_equals_the_dense_one_in_fp64(N, B, F_in, momentum):
    case = R.make_case(N, B, F_in)
    ref = R.dense_reference(case, momentum)
    # the cases' margin around relu's kink (the GPU tests rely on it)
    assert float(ref["y"].abs().min()) >= R.MARGIN * float(ref["y"].abs().max())
    assert bool((case["x"][:, 1] == 0).all()) and float((case["x"] == 0).float().mean()) > 0.85
    c = {k: (v.double() if v.is_floating_point() else v) for k, v in case.items()}
    z2, saved = R.forward(c["h1"], c["x"], c["batch"], c["rootindex"], c["W2"], c["gamma"], c["beta"])
    grads = R.backward(saved, c["up"])
    rm, rv, nbt = R.blend(saved, c["running_mean"], c["running_var"], c["num_batches_tracked"], momentum)
    got = dict(z2=z2, dh1=grads[0], dW2=grads[1], dgamma=grads[2], dbeta=grads[3], running_mean=rm, running_var=rv)
    for k, v in got.items():
        assert v.shape == ref[k].shape, k
        assert _rel(v, ref[k]) <= BAR, (k, _rel(v, ref[k]))
    assert int(nbt) == int(ref["num_batches_tracked"]) == int(case["num_batches_tracked"]) + 1
    # the column that is zero in every root row has var = 0: y = beta through the 1 / sqrt(eps) path
    assert float(saved["var"][R.H + 1]) == 0.0
    assert torch.equal(saved["y_x"][:, 1], c["beta"][R.H + 1].expand(B))


def test_factored_form_inside_forward_train_on_the_model_fixture(monkeypatch):
    """The whole training forward with each direction's block replaced by the factored form: outputs,
    every gradient and every buffer equal the dense restatement's."""
    z = T.load_npz(MODEL_FIXTURE)
    noise = (z["noise_td"].double(), z["noise_bu"].double())
    args = (z["x"].double(), z["edge_index"], z["BU_edge_index"], z["batch"], z["rootindex"], noise)

    def run():
        sd = T.with_grad(T.group(z, "sd"), torch.float64)
        new = {}
        logp, td, bu = T.forward_train(sd, *args, new_buffers=new)
        have, none, _ = T.grads_of(F.nll_loss(logp, z["y"]) + 0.2 * (td + bu), sd)
        return logp.detach(), td.detach(), bu.detach(), have, none, new

    want = run()

    def direction_factored(sd, d, x, edge_index, batch, rootindex, infer, noise, new_buffers):
        h1 = O.gcn_conv(x, edge_index, sd[d + ".conv1.lin.weight"], sd[d + ".conv1.bias"])
        loss, pred = T.edge_infer_train(sd, d, h1, edge_index, noise, new_buffers)
        saved = {}
        z2 = R.Factored.apply(h1, sd[d + ".conv2.lin.weight"], sd[d + ".bn1.weight"], sd[d + ".bn1.bias"], x, batch,
                              rootindex, saved)
        rm, rv, nbt = R.blend(saved, sd[d + ".bn1.running_mean"], sd[d + ".bn1.running_var"],
                              sd[d + ".bn1.num_batches_tracked"])
        new_buffers.update({d + ".bn1.running_mean": rm, d + ".bn1.running_var": rv,
                            d + ".bn1.num_batches_tracked": nbt})
        # conv2's aggregation of a given lin output: gcn_conv with the identity as its weight
        eye = torch.eye(R.H, dtype=z2.dtype)
        h2 = F.relu(O.gcn_conv(z2, edge_index, eye, sd[d + ".conv2.bias"], edge_weight=pred))
        root_of_node = rootindex[batch]
        return O.scatter_mean(torch.cat((h2, h1.detach()[root_of_node]), 1), batch, dim=0), loss

    monkeypatch.setattr(T, "direction_train", direction_factored)
    got = run()
    for k in range(3):
        assert _rel(got[k], want[k]) <= BAR, k
    assert got[4] == want[4] and sorted(got[3]) == sorted(want[3])
    for k, g in want[3].items():
        assert _rel(got[3][k], g) <= BAR, (k, _rel(got[3][k], g))
    assert sorted(got[5]) == sorted(want[5])
    for k, v in want[5].items():
        if v.is_floating_point():
            assert _rel(got[5][k], v) <= BAR, k
        else:
            assert int(got[5][k]) == int(v), k


def test_entry_points_refuse_bad_arguments_before_any_device_work():
    """Fake 16-byte-aligned addresses that are never dereferenced, as tests/test_capi.py does."""
    from bigcn_amd import _lib
    lib = _lib.load_library()
    fake = 0x10000
    N, B, Fi = 43, 3, 8

    def fill(a):
        for k, (name, tp) in enumerate(a._fields_):
            if tp is ctypes.c_void_p:
                setattr(a, name, fake + 0x1000 * k)
        a.ldh, a.ldx, a.num_nodes, a.num_graphs, a.in_feats, a.hid, a.eps = 64, Fi, N, B, Fi, 64, 1e-5
        return a

    def fwd_args():
        a = fill(_lib.Conv2LinTrainFwdArgs())
        a.ldz = 64
        return a

    def bwd_args():
        a = fill(_lib.Conv2LinTrainBwdArgs())
        a.lddz = a.ldd = 64
        return a

    need = lib.bgcn_ebgcn_conv2_lin_train_workspace_size(N, B, Fi)
    assert need > lib.bgcn_ebgcn_conv2_lin_workspace_size(N, B, Fi)
    assert lib.bgcn_ebgcn_conv2_lin_train_workspace_size(0, B, Fi) == 0
    ws = fake + 0x100000

    for make, call in ((fwd_args, lib.bgcn_ebgcn_conv2_lin_train_fwd), (bwd_args, lib.bgcn_ebgcn_conv2_lin_train_bwd)):
        def rejected(a, text, ws=ws, ws_bytes=need):
            assert call(ctypes.addressof(a), ws, ws_bytes, None) == -1
            assert text in lib.bgcn_last_error(), lib.bgcn_last_error()

        assert call(None, ws, need, None) == -1
        a = make()
        a.hid = 32
        rejected(a, b"hidden size must be 64")
        a = make()
        a.in_feats = a.ldx = 6
        rejected(a, b"in_feats must be a positive multiple of 4")
        a = make()
        a.ldh = 66
        rejected(a, b"leading dimensions")
        a = make()
        a.ldx = Fi - 4
        rejected(a, b"leading dimensions")
        for name, tp in make()._fields_:
            if tp is ctypes.c_void_p:
                a = make()
                setattr(a, name, None)
                rejected(a, b"null pointer")
        a = make()
        a.h1 = fake + 4
        rejected(a, b"16-byte aligned")
        rejected(make(), b"workspace too small", ws_bytes=need - 1)
        rejected(make(), b"workspace too small", ws=None)
