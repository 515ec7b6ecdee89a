"""CPU checks of the LSTM baseline's training path (bgcn_lstm_train_grad, LSTM.grad_batch,
LSTMTrainStep): the GPU tests' bar is feasible (torch's own fp32 autograd sits at least 10x under it
on every case and tensor), the C struct and its ctypes mirror agree, the entry point rejects bad
arguments before any device work, and the Python surface is what the documents say."""
import ctypes
import os
import shutil
import subprocess

import pytest
import torch

import lstm_ref as R
import lstm_train_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bgcn.h")


@pytest.mark.parametrize("name", T.PARITY_CASES)
def test_the_gradient_bar_is_feasible(name):
    """The reference's own arithmetic (torch fp32 autograd, CPU) against the fp64 oracle in the metric
    max|got - ref| / max|ref|: at least 10x under the 1e-4 bar for every gradient tensor and x.grad,
    and 10x under the absolute 1e-4 for loss and logp."""
    c = T.case(name)
    want = T.oracle(name)
    got = T.grads_of(c, torch.float32)
    assert sorted(got.grads) == sorted(T.names(c.cfg["layers"]) + ["x"])
    worst = 0.0
    for k, g in got.grads.items():
        e = T.rel_err(g, want.grads[k])
        worst = max(worst, e)
        print(f"{name} {k}: fp32 vs fp64 {e:.3e} (max|ref| {float(want.grads[k].abs().max()):.3e})")
        assert e <= T.BAR / 10, (k, e)
    assert abs(float(got.loss) - float(want.loss)) <= T.BAR / 10
    assert float((got.logp.double() - want.logp).abs().max()) <= T.BAR / 10
    # the oracle's forward is lstm_ref's
    assert float((want.logp - c.ref.logp).abs().max()) < 1e-12
    print(name, "worst", worst)


def test_the_training_cases_are_a_table_of_their_own():
    assert not set(T.TRAIN_CASES) & (set(R.CASES) | set(R.EDGE_CASES))
    seeds = [c["seed"] for c in T.TRAIN_CASES.values()]
    assert len(set(seeds)) == len(seeds) and min(seeds) > max(c["seed"] for c in R.EDGE_CASES.values())
    c = T.case("t_many_trees")
    assert c.B == 300 and max(c.cfg["lengths"]) == 3
    assert T.case("t_rows_over_switch").N == 8217
    assert T.case("t_largest").cfg["hid"] * T.case("t_largest").cfg["layers"] * 2 == 8192
    assert T.case("t_one_class").cfg["out"] == 1 and T.case("t_classes_63").cfg["out"] == 63
    assert T.case("t_hid_128").cfg["hid"] == 128 and T.case("t_hid_256").cfg["hid"] == 256


@pytest.mark.parametrize("name", ["boundaries", "one_layer"])
def test_the_five_step_loss_bar_is_feasible(name):
    """Five iterations of the reference loop with torch.optim.Adam (lr 5e-4, weight decay 1e-4): torch's
    fp32 losses stay at least 10x under the GPU test's 1e-4 of the fp64 loop's."""
    c = T.case(name)
    want = T.train_losses(c, 5, torch.float64)
    got = T.train_losses(c, 5, torch.float32)
    print(name, want, got)
    assert want[4] < want[0]
    for a, b in zip(got, want):
        assert abs(a - b) <= T.BAR / 10


def test_binding_lists_the_new_symbols():
    from bigcn_amd import _lib
    for name in ("bgcn_lstm_train_workspace_size", "bgcn_lstm_train_grad"):
        assert name in _lib.EXPORTED_SYMBOLS and name in _lib._SIGS
        assert hasattr(_lib.load_library(), name)
    assert _lib.load_library().bgcn_abi_version() == 12


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_struct_layout_matches_header(tmp_path):
    from bigcn_amd import _lib
    cname, py = "bgcn_lstm_train_args", _lib.LstmTrainArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {",
             f'printf("sizeof %zu\\n", sizeof({cname}));']
    for fname, _ in py._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append(f'printf("d_w_hh_1_1 %zu\\n", offsetof({cname}, d_w_hh[1][1]));')
    lines.append(f'printf("fwd_status %zu\\n", offsetof({cname}, fwd.status));')
    lines.append("return 0; }")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(c)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = dict((line.split()[0], int(line.split()[1])) for line in out if line)
    assert got["sizeof"] == ctypes.sizeof(py)
    for fname, _ in py._fields_:
        assert got[fname] == getattr(py, fname).offset, fname
    assert got["d_w_hh_1_1"] == py.d_w_hh.offset + (1 * 2 + 1) * ctypes.sizeof(ctypes.c_void_p)
    assert got["fwd_status"] == py.fwd.offset + _lib.LstmArgs.status.offset
    assert py.fwd.offset == 0 and ctypes.sizeof(py) > ctypes.sizeof(_lib.LstmArgs)


def test_workspace_size():
    from bigcn_amd import _lib
    lib = _lib.load_library()
    ws, ev = lib.bgcn_lstm_train_workspace_size, lib.bgcn_lstm_workspace_size
    assert ws(1000, 24, 768, 768, 2) > ws(100, 24, 768, 768, 2) > 0
    # per layer the gates [N, 8H], the outputs and the cell states [N, 2H] each
    assert ws(1000, 24, 768, 768, 2) >= 4 * 1000 * 768 * 2 * (8 + 2 + 2)
    assert ws(1000, 24, 768, 768, 2) > ev(1000, 24, 768, 768, 2)
    assert ws(1000, 24, 5000, 64, 3) > ws(1000, 24, 5000, 64, 2)
    for bad in ((0, 1, 768, 768, 2), (10, 0, 768, 768, 2), (10, 2, 770, 768, 2), (10, 2, 768, 96, 2),
                (10, 2, 768, 32, 2), (10, 2, 768, 1088, 2), (10, 2, 768, 768, 0), (10, 2, 768, 768, 5)):
        assert ws(*bad) == 0, bad


def test_bad_arguments_fail_before_any_device_work():
    """Fake 16-byte-aligned addresses that are never dereferenced: every rejection happens on the host."""
    from bigcn_amd import _lib
    lib = _lib.load_library()
    fake = 0x10000

    def plausible():
        t = _lib.LstmTrainArgs()
        a = t.fwd
        a.x, a.ldx, a.num_nodes, a.in_feats, a.hid, a.num_layers, a.out_feats = fake, 20, 10, 20, 64, 2, 4
        a.seq_start, a.num_seqs, a.max_len = fake + 0x100, 2, 8
        for l in range(2):
            for d in range(2):
                a.w_ih[l][d] = fake + 0x1000 * (1 + 2 * l + d)
                a.w_hh[l][d] = fake + 0x1000 * (5 + 2 * l + d)
                t.d_w_ih[l][d] = fake + 0x1000 * (17 + 2 * l + d)
                t.d_w_hh[l][d] = fake + 0x1000 * (21 + 2 * l + d)
        a.fc_w, a.fc_b, a.logp, a.status = fake + 0x9000, fake + 0xa000, fake + 0xb000, fake + 0xc000
        a.y = fake + 0xd000
        t.d_fc_w, t.d_fc_b, t.skip_flag = fake + 0xe000, fake + 0xf000, fake + 0x10000
        return t

    def rejected(t, text, ws=None, ws_bytes=0):
        assert lib.bgcn_lstm_train_grad(ctypes.addressof(t), ws, ws_bytes, None) == -1
        assert text in lib.bgcn_last_error(), lib.bgcn_last_error()

    assert lib.bgcn_lstm_train_grad(None, None, 0, None) == -1
    rejected(_lib.LstmTrainArgs(), b"unsupported shape")
    rejected(plausible(), b"workspace too small")
    for field, value, text in (("in_feats", 22, b"unsupported shape"), ("hid", 96, b"unsupported shape"),
                               ("hid", 2048, b"unsupported shape"), ("num_layers", 5, b"unsupported shape"),
                               ("out_feats", 0, b"out_feats"), ("out_feats", 65, b"out_feats"),
                               ("max_len", 0, b"max_len"), ("seq_start", None, b"null pointer"),
                               ("logp", None, b"null pointer"), ("status", None, b"null pointer"),
                               ("y", None, b"null pointer"),
                               ("ldx", 18, b"16-byte"), ("x", fake + 4, b"16-byte"), ("fc_w", fake + 0x9004, b"16-byte")):
        t = plausible()
        setattr(t.fwd, field, value)
        rejected(t, text)
    for field, value, text in (("d_fc_w", None, b"null pointer"), ("d_fc_b", None, b"null pointer"),
                               ("skip_flag", None, b"null pointer"), ("dx", fake + 0x20004, b"16-byte")):
        t = plausible()
        setattr(t, field, value)
        rejected(t, text)
    t = plausible()
    t.fwd.w_hh[1][1] = None
    rejected(t, b"LSTM weight")
    t = plausible()
    t.d_w_ih[1][0] = None
    rejected(t, b"LSTM weight gradient")
    t = plausible()
    t.d_w_hh[0][1] = fake + 0x30004
    rejected(t, b"LSTM weight gradient")
    need = lib.bgcn_lstm_train_workspace_size(10, 2, 20, 64, 2)
    rejected(plausible(), b"workspace too small", fake + 0x100000, need - 256)


def test_forward_still_raises_in_training_mode_and_points_to_the_step():
    from bigcn_amd import LSTM, _lib
    m = LSTM(20, 64, 4, 1, version=2)
    with pytest.raises(NotImplementedError, match="training") as e:
        m(torch.zeros(3, 20))
    assert "LSTMTrainStep" in str(e.value)
    with pytest.raises(_lib.BGCNError):
        m.grad_batch(torch.zeros(3, 20), torch.tensor([0]), torch.tensor([1]), max_len=3)


@pytest.mark.parametrize("layers", [1, 2, 4])
def test_lstm_adam_is_one_group_over_every_tensor(layers):
    import bigcn_amd
    from bigcn_amd import LSTM, LSTMTrainStep, MultiAdam, lstm_adam
    m = LSTM(20, 64, 4, layers)
    opt = lstm_adam(m)
    assert isinstance(opt, MultiAdam) and len(opt.param_groups) == 1
    g = opt.param_groups[0]
    assert len(g["params"]) == 4 * layers + 2
    assert {id(p) for p in g["params"]} == {id(p) for p in m.parameters()}
    assert g["lr"] == 5e-4 and opt.weight_decay == 1e-4 and opt.betas == (0.9, 0.999) and opt.eps == 1e-8
    assert sorted(m.names()) == sorted(m.state_dict())
    for n, t in zip(m.names(), m._tensors()):
        assert t is dict(m.named_parameters())[n]
    step = LSTMTrainStep(m)
    assert step.step_count == 0 and step.check_status() == 0
    assert LSTMTrainStep(m, optimizer=opt).optimizer is opt
    for name in ("LSTMTrainStep", "lstm_adam"):
        assert name in bigcn_amd.__all__
