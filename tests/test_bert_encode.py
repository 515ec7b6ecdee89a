"""CPU checks of the PHEME feature extraction (bigcn_amd.TweetEncoder, bgcn_bert_encode): the plain-torch
restatement tests/bert_encode_ref.py against ``transformers`` where it is installed, the conditions that
keep the GPU tests' bar meaningful, and the bindings."""
import ctypes
import os
import re

import pytest
import torch

import bert_encode_ref as E
import bert_ref as R

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bgcn.h")


# ---------------------------------------------------------------- 1. the restatement against transformers
@pytest.mark.parametrize("T", [1, 33, 64])
def test_restatement_matches_transformers_in_fp64(T):
    """getPHEMEgraph.py:114-115 on a BertModel built locally from a BertConfig (nothing is downloaded)."""
    transformers = pytest.importorskip("transformers")
    cfg = transformers.BertConfig(vocab_size=16, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
                                  intermediate_size=128, max_position_embeddings=192)
    model = transformers.BertModel(cfg).double().eval()
    sd = {k: v.double() for k, v in E.make_state_dict(128, 128, 2, 192, 16, seed=5, weight_factor=6.0).items()}
    model.load_state_dict(sd, strict=True)
    ids = E.make_ids(3, T, 16, torch.Generator().manual_seed(T))
    with torch.no_grad():
        emb = model.embeddings(ids)
        cls = model(ids).pooler_output
    ref = E.run(sd, ids, 2, 2)
    errs = (float((emb - ref.embeddings).abs().max()), float((cls - ref.cls).abs().max()))
    print(T, errs)
    assert max(errs) <= 1e-12


# ---------------------------------------------------------------- 2. the cases
@pytest.mark.parametrize("name", sorted(E.CASES))
def test_case_fp32_restatement_is_well_inside_the_bar(name):
    """torch's own fp32 arithmetic is within BAR / 4 of the fp64 oracle on every output: the GPU tests'
    bar then measures the kernels, not the case's conditioning."""
    c = E.case(name)
    f = E.run(c.sd, c.ids, c.cfg["layers"], c.heads, torch.float32)
    errs = {k: float((getattr(f, k).double() - getattr(c.ref, k)).abs().max()) for k in ("embeddings", "cls", "hidden")}
    print(name, errs, "top score", c.ref.top_score)
    assert max(errs.values()) <= E.BAR / 4
    assert torch.isfinite(c.ref.hidden).all()


def test_cases_hold_padding_runs_and_the_last_token():
    for name in sorted(E.CASES):
        c = E.case(name)
        V = c.cfg["vocab"]
        assert int(c.ids.min()) >= 0 and int(c.ids.max()) == V - 1
        if c.cfg["T"] > 2:
            assert bool((c.ids[:, -2:] == 0).all()), name


def test_sharp_case_moves_the_running_maximum():
    """Rows whose largest score lies in a later key tile by more than TILE_GAP (the sum over tile 0 is
    rescaled by less than exp(-10)), and rows the other way."""
    gap = E.case("sharp").ref.tile_gap[0]
    assert int((gap > E.TILE_GAP).sum()) >= 8 and int((gap < -E.TILE_GAP).sum()) >= 8


def test_switch_cases_sit_at_the_gemm_switch():
    a, b = E.case("rows_at_switch"), E.case("rows_under_switch")
    assert a.ids.numel() == 8192 and b.ids.numel() == 8192 - 128
    assert torch.equal(a.ids[:63], b.ids) and all(torch.equal(a.sd[k], b.sd[k]) for k in a.sd)
    assert a.cfg["hidden"] % 128 == 0 and a.cfg["intermediate"] % 128 == 0   # the six-product kernel's shapes


# ---------------------------------------------------------------- 3. bindings
def _bert_model_shapes(hidden, heads, inter, layers, max_pos, vocab):
    transformers = pytest.importorskip("transformers")
    cfg = transformers.BertConfig(vocab_size=vocab, hidden_size=hidden, num_hidden_layers=layers,
                                  num_attention_heads=heads, intermediate_size=inter, max_position_embeddings=max_pos)
    return {k: tuple(v.shape) for k, v in transformers.BertModel(cfg).state_dict().items()}


def test_state_dict_is_bert_models():
    from bigcn_amd import TweetEncoder
    m = TweetEncoder(hidden=128, heads=2, intermediate=256, num_layers=2, max_pos=40, vocab=24)
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    want = _bert_model_shapes(128, 2, 256, 2, 40, 24)
    assert got == want


def test_default_module_has_bert_base_names_and_shapes():
    from bigcn_amd import TweetEncoder
    with torch.device("meta"):
        m = TweetEncoder()
    sd = m.state_dict()
    assert len(sd) == 5 + 12 * 16 + 2
    assert tuple(sd["embeddings.word_embeddings.weight"].shape) == (30522, 768)
    assert tuple(sd["embeddings.position_embeddings.weight"].shape) == (512, 768)
    assert tuple(sd["encoder.layer.11.intermediate.dense.weight"].shape) == (3072, 768)
    assert tuple(sd["pooler.dense.bias"].shape) == (768,)
    assert list(sd)[0] == "embeddings.word_embeddings.weight" and list(sd)[-1] == "pooler.dense.bias"
    assert m.names()[0] == "embeddings.word_embeddings.weight" and len(m.names()) == 7 + 12 * 16


def test_strict_loading_of_a_stripped_treebert_state_dict():
    from bigcn_amd import TweetEncoder
    sd = R.make_state_dict(128, 128, 2, 64, 4, seed=3)
    own = {k[len("BERT."):]: v for k, v in sd.items() if k.startswith("BERT.")}
    m = TweetEncoder(hidden=128, heads=2, intermediate=128, num_layers=2, max_pos=64, vocab=R.VOCAB)
    m.load_state_dict(own, strict=True)
    assert torch.equal(m.state_dict()["encoder.layer.1.output.dense.bias"], sd["BERT.encoder.layer.1.output.dense.bias"])
    # an older transformers also saved this buffer
    m.load_state_dict(dict(own, **{"embeddings.position_ids": torch.arange(64).unsqueeze(0)}), strict=True)
    with pytest.raises(RuntimeError):
        m.load_state_dict(sd, strict=True)   # the prefixed names are not this module's


def test_from_treebert_shares_storage():
    from bigcn_amd import TreeBERT, TweetEncoder
    t = TreeBERT(hidden=64, heads=1, intermediate=64, num_layers=1, max_pos=8, vocab=12)
    e = TweetEncoder.from_treebert(t)
    assert (e.hidden, e.heads, e.intermediate, e.num_layers, e.max_pos, e.vocab) == (64, 1, 64, 1, 8, 12)
    tp = dict(t.named_parameters())
    for k, p in e.named_parameters():
        assert p is tp["BERT." + k], k
    assert set("BERT." + k for k in e.state_dict()) == set(k for k in t.state_dict() if k.startswith("BERT."))
    with torch.no_grad():
        t.BERT.pooler.dense.bias.fill_(3.0)
    assert float(e.pooler.dense.bias.detach()[0]) == 3.0


def test_symbols_struct_and_status_bit():
    import bigcn_amd
    from bigcn_amd import _lib
    assert "TweetEncoder" in bigcn_amd.__all__
    for name in ("bgcn_bert_encode_workspace_size", "bgcn_bert_encode"):
        assert name in _lib.EXPORTED_SYMBOLS and name in _lib._SIGS
    text = open(HEADER).read()
    m = re.search(r"#define BGCN_STATUS_TOKEN (\w+)", text)
    assert m and int(m.group(1), 0) == _lib.BGCN_STATUS_TOKEN == 512
    taken = [int(v, 0) for v in re.findall(r"#define BGCN_STATUS_\w+ (\w+)", text)]
    assert len(set(taken)) == len(taken) and all(b & (b - 1) == 0 for b in taken)   # one bit each, none given twice
    with pytest.raises(IndexError, match="token id"):
        _lib.raise_on_status(_lib.BGCN_STATUS_TOKEN, bits=_lib.BGCN_STATUS_TOKEN)
    _lib.raise_on_status(_lib.BGCN_STATUS_TOKEN)    # not among the default bits


def test_struct_layout_matches_header(tmp_path):
    import shutil
    import subprocess
    from bigcn_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    py = _lib.BertEncodeArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {",
             'printf("sizeof %zu\\n", sizeof(bgcn_bert_encode_args));']
    lines += [f'printf("{f} %zu\\n", offsetof(bgcn_bert_encode_args, {f}));' for f, _ in py._fields_]
    lines.append("return 0; }")
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split()
    got = dict(zip(out[::2], map(int, out[1::2])))
    assert got["sizeof"] == ctypes.sizeof(py)
    for f, _ in py._fields_:
        assert got[f] == getattr(py, f).offset, f


def test_workspace_size_and_argument_checks_without_a_gpu():
    """bgcn_bert_encode returns BGCN_EINVAL with its message before any HIP call: the pointers are fake
    16-byte-aligned addresses that are never dereferenced."""
    from bigcn_amd import _lib
    lib = _lib.load_library()
    size = lib.bgcn_bert_encode_workspace_size
    H, I, L, n, T = 128, 256, 2, 3, 70
    assert size(n, T, H, I, L, 0) >= 4 * n * T * (7 * H + I)
    assert size(n, T, H, I, L, 0) == size(n, T, H, I, L, 1)
    for bad in ((0, T, H, I, L), (n, 0, H, I, L), (n, 513, H, I, L), (n, T, 96, I, L), (n, T, 2048, I, L),
                (n, T, H, 100, L), (n, T, H, I, 0), (n, T, H, I, 25), (65536, T, H, I, L)):
        assert size(*bad, 0) == 0, bad
    fake = 0x10000

    def plausible():
        a = _lib.BertEncodeArgs()
        a.input_ids, a.num_seqs, a.seq_len, a.vocab = fake, n, T, 16
        a.hidden, a.heads, a.intermediate, a.num_layers, a.max_pos, a.ln_eps = H, 2, I, L, 192, 1e-12
        for k, (f, _) in enumerate(_lib.BertEncodeArgs._fields_):
            if f in ("word_emb", "pos_emb", "type_emb", "emb_ln_w", "emb_ln_b", "pooler_w", "pooler_b"):
                setattr(a, f, fake + 0x100 * k)
        for layer in range(L):
            for k, (f, _) in enumerate(_lib.BertLayer._fields_):
                setattr(a.layer[layer], f, fake + 0x4000 + 0x1000 * layer + 0x40 * k)
        a.embeddings, a.ld_embeddings, a.cls, a.status = fake + 0x8000, H, fake + 0x9000, fake + 0xa000
        return a

    def rejected(a, text, ws=fake + 0x100000, ws_bytes=1 << 40):
        assert lib.bgcn_bert_encode(ctypes.addressof(a), ws, ws_bytes, None) == -1
        assert text in lib.bgcn_last_error(), lib.bgcn_last_error()

    assert lib.bgcn_bert_encode(None, None, 0, None) == -1
    rejected(plausible(), b"workspace too small", ws=None, ws_bytes=0)
    rejected(plausible(), b"workspace too small", ws_bytes=size(n, T, H, I, L, 0) - 1)
    for field, value, text in (("hidden", 96, b"unsupported shape"), ("heads", 3, b"unsupported shape"),
                               ("intermediate", 100, b"unsupported shape"), ("num_layers", 25, b"unsupported shape"),
                               ("num_seqs", 0, b"unsupported shape"), ("num_seqs", 65536, b"unsupported shape"),
                               ("max_pos", 513, b"unsupported shape"), ("seq_len", 0, b"unsupported shape"),
                               ("seq_len", 193, b"seq_len must be in [1, max_pos]"), ("vocab", 0, b"vocab"),
                               ("input_ids", None, b"null pointer"), ("status", None, b"null pointer"),
                               ("word_emb", None, b"null or unaligned BERT weight"),
                               ("pos_emb", fake + 4, b"null or unaligned BERT weight"),
                               ("pooler_w", None, b"null or unaligned BERT weight"),
                               ("cls", None, b"null output"), ("cls", fake + 0x9004, b"16-byte aligned"),
                               ("embeddings", fake + 0x8008, b"16-byte aligned"), ("ld_embeddings", H - 4, b"16-byte aligned"),
                               ("ld_embeddings", H + 2, b"16-byte aligned"),
                               ("hidden_out", fake + 0xb000, b"hidden_out needs last_layer_full")):
        a = plausible()
        setattr(a, field, value)
        rejected(a, text)
    a = plausible()
    a.layer[1].o_ln_b = None
    rejected(a, b"null or unaligned BERT weight")
    a = plausible()
    a.layer[0].k_w = fake + 8
    rejected(a, b"null or unaligned BERT weight")
    a = plausible()
    a.hidden_out, a.last_layer_full = fake + 0xb004, 1
    rejected(a, b"16-byte aligned")
    a = plausible()
    a.embed_only, a.embeddings = 1, None
    rejected(a, b"null output")
    a = plausible()
    a.embed_only, a.last_layer_full, a.hidden_out = 1, 1, fake + 0xb000
    rejected(a, b"hidden_out needs last_layer_full")


def test_python_input_checks_without_a_gpu():
    from bigcn_amd import TweetEncoder, _lib
    m = TweetEncoder(hidden=64, heads=1, intermediate=64, num_layers=1, max_pos=8, vocab=12)
    with pytest.raises(_lib.BGCNError, match="device tensors"):
        m.encode(torch.zeros(2, 4, dtype=torch.int64))
    with pytest.raises(_lib.BGCNError, match="device tensors"):
        m.features(torch.zeros(2, 4, dtype=torch.int64))
    for bad in (torch.zeros(4, dtype=torch.int64), torch.zeros(2, 4), torch.zeros(0, 4, dtype=torch.int64),
                torch.zeros(2, 0, dtype=torch.int64), torch.zeros(2, 9, dtype=torch.int64)):
        with pytest.raises(ValueError):
            m.encode(bad)
        with pytest.raises(ValueError):
            m.embed(bad)
    m.check_status()   # nothing ran: nothing to report, no device needed
