"""CPU checks of the LSTM baseline (bigcn_amd.lstm, bgcn_lstm_eval): the module's state_dict is the
reference's key for key, the C ABI and its ctypes mirror agree, the entry points reject bad
arguments before any device work, and the restatement tests/lstm_ref.py is what torch computes.
The last test shows that the GPU tests' 1e-4 bar is feasible: the reference's own fp32 arithmetic
sits at least 10x under it on every case."""
import ctypes
import os
import shutil
import subprocess

import pytest
import torch

import lstm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bgcn.h")


@pytest.mark.parametrize("cfg", [(768, 768, 4, 2), (5000, 64, 64, 2), (20, 64, 4, 1), (20, 64, 4, 3)])
def test_state_dict_is_the_references(cfg):
    from bigcn_amd import LSTM
    in_feats, hid, out, layers = cfg
    lstm, fc = R.build(in_feats, hid, out, layers, torch.float32)
    want = R.state_dict(lstm, fc)
    model = LSTM(in_feats, hid, out, layers)
    got = model.state_dict()
    assert list(got) == list(want)
    assert {k: tuple(v.shape) for k, v in got.items()} == {k: tuple(v.shape) for k, v in want.items()}
    model.load_state_dict(want, strict=True)
    for k, v in model.state_dict().items():
        assert torch.equal(v, want[k]), k


def test_constructor_is_the_references():
    from bigcn_amd import LSTM
    m = LSTM()
    assert (m.in_feats, m.hid_feats, m.out_feats, m.num_layers, m.pooling, m.version) == (768, 768, 4, 2, 'max', 0)
    m = LSTM(5000, 64, 64, 2, None)   # the Twitter15/16 call, positional
    assert m.fc.in_features == 256 and m.fc.out_features == 64 and m.device is None


def test_training_mode_and_cpu_tensors_raise():
    from bigcn_amd import LSTM, _lib
    m = LSTM(20, 64, 4, 1, version=2)
    with pytest.raises(NotImplementedError, match="training"):
        m(torch.zeros(3, 20))
    m.eval()
    with pytest.raises(_lib.BGCNError):
        m(torch.zeros(3, 20))
    with pytest.raises(_lib.BGCNError):
        m.forward_batch(torch.zeros(3, 20), torch.tensor([0]), max_len=3)


def test_binding_lists_the_new_symbols_and_constants():
    import re
    from bigcn_amd import _lib
    for name in ("bgcn_lstm_workspace_size", "bgcn_lstm_eval"):
        assert name in _lib.EXPORTED_SYMBOLS and name in _lib._SIGS
        assert hasattr(_lib.load_library(), name)
    text = open(HEADER).read()
    for name in ("BGCN_STATUS_SEQUENCE", "BGCN_LSTM_SEQ_TILE"):
        m = re.search(rf"#define {name} (\d+)", text)
        assert m and int(m.group(1)) == getattr(_lib, name), name
    assert R.SEQ_TILE == _lib.BGCN_LSTM_SEQ_TILE
    # the next unused status bit
    bits = [int(v) for v in re.findall(r"#define BGCN_STATUS_\w+ (\d+)", text)]
    assert _lib.BGCN_STATUS_SEQUENCE == 2 * max(b for b in bits if b != _lib.BGCN_STATUS_SEQUENCE)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_struct_layout_matches_header(tmp_path):
    from bigcn_amd import _lib
    cname, py = "bgcn_lstm_args", _lib.LstmArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {",
             f'printf("sizeof %zu\\n", sizeof({cname}));']
    for fname, _ in py._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append(f'printf("w_ih_1_1 %zu\\n", offsetof({cname}, w_ih[1][1]));')
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
    assert got["w_ih_1_1"] == py.w_ih.offset + (1 * 2 + 1) * ctypes.sizeof(ctypes.c_void_p)   # [layer][direction]


def test_workspace_size():
    from bigcn_amd import _lib
    ws = _lib.load_library().bgcn_lstm_workspace_size
    assert ws(1000, 24, 768, 768, 2) > ws(100, 24, 768, 768, 2) > 0
    # G [N, 8H] and the layers' outputs [N, 2H]
    assert ws(1000, 24, 768, 768, 2) >= 4 * 1000 * 768 * (8 + 2 * 2)
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
        a = _lib.LstmArgs()
        a.x, a.ldx, a.num_nodes, a.in_feats, a.hid, a.num_layers, a.out_feats = fake, 20, 10, 20, 64, 2, 4
        a.seq_start, a.num_seqs, a.max_len = fake + 0x100, 2, 8
        for l in range(2):
            for d in range(2):
                a.w_ih[l][d] = fake + 0x1000 * (1 + 2 * l + d)
                a.w_hh[l][d] = fake + 0x1000 * (5 + 2 * l + d)
        a.fc_w, a.fc_b, a.logp, a.status = fake + 0x9000, fake + 0xa000, fake + 0xb000, fake + 0xc000
        return a

    def rejected(a, text, ws=None, ws_bytes=0):
        assert lib.bgcn_lstm_eval(ctypes.addressof(a), ws, ws_bytes, None) == -1
        assert text in lib.bgcn_last_error(), lib.bgcn_last_error()

    assert lib.bgcn_lstm_eval(None, None, 0, None) == -1
    rejected(_lib.LstmArgs(), b"unsupported shape")
    rejected(plausible(), b"workspace too small")
    for field, value, text in (("in_feats", 22, b"unsupported shape"), ("hid", 96, b"unsupported shape"),
                               ("hid", 2048, b"unsupported shape"), ("num_layers", 5, b"unsupported shape"),
                               ("out_feats", 0, b"out_feats"), ("out_feats", 65, b"out_feats"),
                               ("max_len", 0, b"max_len"), ("seq_start", None, b"null pointer"),
                               ("logp", None, b"null pointer"), ("status", None, b"null pointer"),
                               ("ldx", 18, b"16-byte"), ("x", fake + 4, b"16-byte"), ("fc_w", fake + 0x9004, b"16-byte")):
        a = plausible()
        setattr(a, field, value)
        rejected(a, text)
    a = plausible()
    a.w_hh[1][1] = None
    rejected(a, b"LSTM weight")
    # a workspace short of the last array (the size is rounded up to 256 bytes)
    need = lib.bgcn_lstm_workspace_size(10, 2, 20, 64, 2)
    rejected(plausible(), b"workspace too small", fake + 0x100000, need - 256)


def test_max_sequence_len():
    from bigcn_amd.lstm import max_sequence_len
    assert max_sequence_len(torch.tensor([0, 3, 4]), 10) == 6
    assert max_sequence_len([0], 1) == 1
    assert max_sequence_len(torch.tensor([2, 9]), 10) == 7     # rows 0, 1 belong to no tree
    assert max_sequence_len([0, 5, 5], 6) == 5                  # an empty tree: flagged by the call
    assert max_sequence_len([4, 2], 3) == 1                     # never below one step


def _case(name):
    return R.case(name) if name in R.CASES else R.edge_case(name)


def test_edge_cases_are_a_table_of_their_own():
    """CASES keeps its eight names (a case's seed is its position among them, and
    profiles/lstm_parity.json records those data); the edge cases carry explicit, distinct seeds."""
    assert sorted(R.CASES) == ["boundaries", "offset_strided", "one_layer", "pheme", "saturated", "three_layers",
                               "tile_plus_one", "twitter"]
    assert not set(R.CASES) & set(R.EDGE_CASES)
    seeds = [c["seed"] for c in R.EDGE_CASES.values()]
    assert len(set(seeds)) == len(seeds) and min(seeds) > len(R.CASES)
    c = R.edge_case("many_trees")
    assert c.B == 300 and c.N == 600 and -(-c.B // R.SEQ_TILE) == 10
    c = R.edge_case("rows_over_switch")
    assert c.B == 126 and c.N == 8217 and c.max_len == 129
    c = R.edge_case("offset_many")
    assert int(c.rootindex[0]) == 5 and c.B == 40 > R.SEQ_TILE
    assert R.edge_case("largest").ref.h_n.numel() // 3 == 8192


@pytest.mark.parametrize("name", ["boundaries", "three_layers", "offset_strided", "many_trees", "offset_many"])
def test_oracle_loop_equals_a_packed_run(name):
    c = _case(name)
    lstm, fc = R.build(c.cfg["in_feats"], c.cfg["hid"], c.cfg["out"], c.cfg["layers"], torch.float64, c.seed,
                       c.weight_factor)
    rows, hn, logp = R.run_packed(lstm, fc, c.x, c.rootindex)
    first = int(c.rootindex[0])
    assert float((c.ref.out[first:] - rows).abs().max()) < 1e-12
    assert float(c.ref.out[:first].abs().sum()) == 0.0
    assert float((c.ref.h_n - hn).abs().max()) < 1e-12
    assert float((c.ref.logp - logp).abs().max()) < 1e-12
    # a forward direction's final state is its output at the tree's last row, a reverse one's at its first
    H, L = c.cfg["hid"], c.cfg["layers"]
    ends = c.rootindex.tolist()[1:] + [c.N]
    for b, (s, e) in enumerate(zip(c.rootindex.tolist(), ends)):
        for l in range(L):
            assert torch.equal(c.ref.h_n[2 * l, b], c.ref.layer_out[l][e - 1, :H])
            assert torch.equal(c.ref.h_n[2 * l + 1, b], c.ref.layer_out[l][s, H:])


@pytest.mark.parametrize("name", sorted(R.CASES) + sorted(R.EDGE_CASES))
def test_the_bar_is_feasible(name):
    """Torch's own fp32 CPU LSTM is within 1e-5 of the fp64 oracle on the outputs and logp of every
    GPU case (the saturated variant at its recorded factor), so the reference's arithmetic alone
    sits 10x under the GPU tests' 1e-4 bar; and at least 90 % of the trees have a top-two logit gap
    over 1e-3, where predictions are compared.  The edge cases (tests/test_gpu_lstm_edges.py) hold
    h_n to 1e-5 as well."""
    c = _case(name)
    lstm, fc = R.build(c.cfg["in_feats"], c.cfg["hid"], c.cfg["out"], c.cfg["layers"], torch.float32, c.seed,
                       c.weight_factor)
    got = R.run(lstm, fc, c.x, c.rootindex, c.y)
    for what in ("out", "logp", "h_n"):
        err = float((getattr(got, what).double() - getattr(c.ref, what)).abs().max())
        print(f"{name} {what}: fp32 vs fp64 {err:.3e}")
        # (h_n also holds the first layer's states, whose 5000-term sums reach 1.04e-5 in torch's fp32
        # on the Twitter configuration: printed, and held to the bar itself)
        assert err <= (1e-5 if what != "h_n" or name in R.EDGE_CASES else 1e-4), (what, err)
    assert abs(float(got.loss) - float(c.ref.loss)) <= 1e-5
    assert float(R.margin_ok(c.ref.logp).float().mean()) >= 0.9


@pytest.mark.parametrize("name", ["many_trees", "rows_over_switch", "classes_63"])
def test_edge_cases_that_compare_predictions_keep_their_margin(name):
    """A condition on the inputs (the seed), not on the kernels: where the GPU test compares pred with
    the oracle's, at least 90 % of the trees have a top-two gap over 1e-3 in the fp64 oracle alone."""
    c = R.edge_case(name)
    share = float(R.margin_ok(c.ref.logp).float().mean())
    print(name, "margin share", share)
    assert share >= 0.9
