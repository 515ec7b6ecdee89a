"""CPU checks of the TreeBERT baseline (bigcn_amd.bert, bgcn_bert_eval): the restatement
tests/bert_ref.py is what ``transformers``' ``BertModel`` computes, the module's state_dict is the
reference's key for key, the C ABI and its ctypes mirror agree, the entry point rejects bad arguments
before any device work, and the conditions the GPU tests lean on hold in the oracle alone (the class
reads the root row only, attention is neither uniform nor one-hot, the rankings' gaps, and torch's
own fp32 sits 10x under the GPU tests' 1e-4 bar), over the cases of test_gpu_bert.py and the edge
cases of test_gpu_bert_edges.py alike (plus the edge cases' own: prediction gaps, sharp_tiles' cross-tile
score gaps)."""
import ctypes
import os
import shutil
import subprocess

import pytest
import torch

import bert_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bgcn.h")
ALL = sorted(R.CASES)
EDGES = sorted(R.EDGE_CASES)
INTERNAL = os.path.join(ROOT, "bigcn_amd", "csrc", "bgcn_internal.h")
# worst |restatement - transformers| in fp64 over the cases, measured when this test was written:
# last_hidden_state 6.4e-15, pooler_output 4.0e-15, summed attentions 1.4e-14.  The bar is 100x the worst.
TRANSFORMERS_BAR = 100 * 1.4e-14


@pytest.mark.parametrize("name", ALL)
def test_restatement_is_what_transformers_computes(name):
    """fp64 against fp64: ``BertModel(BertConfig(..., is_decoder=True, attn_implementation="eager"))``
    built from a config (no download) and loaded with the case's weights, one ``inputs_embeds`` call per
    tree as the reference makes it: ``last_hidden_state``, ``pooler_output`` and the attentions summed as
    ``explain_PHEME.py:590`` sums them.  Measured worst differences: see TRANSFORMERS_BAR."""
    tr = pytest.importorskip("transformers")
    c = R.case(name)
    cfg = tr.BertConfig(vocab_size=R.VOCAB, hidden_size=c.cfg["hidden"], num_hidden_layers=c.cfg["layers"],
                        num_attention_heads=c.heads, intermediate_size=c.cfg["intermediate"], hidden_act="gelu",
                        max_position_embeddings=c.cfg["max_pos"], is_decoder=True, attn_implementation="eager")
    bert = tr.BertModel(cfg).double().eval()
    missing = bert.load_state_dict({k[5:]: v.double() for k, v in c.sd.items() if k.startswith("BERT.")}, strict=False)
    assert not missing.unexpected_keys and all("position_ids" in k for k in missing.missing_keys)
    roots = c.rootindex.tolist()
    worst = {"hidden": 0.0, "pooled": 0.0, "attn": 0.0}
    with torch.no_grad():
        for b, r in enumerate(roots):
            end = c.N if b == c.B - 1 else roots[b + 1]
            out = bert(inputs_embeds=c.x[r:end].double().unsqueeze(0), output_attentions=True)
            attn = sum(a.sum(-2).sum(1)[0] for a in out.attentions)
            worst["hidden"] = max(worst["hidden"], float((out.last_hidden_state[0] - c.ref.hidden[r:end]).abs().max()))
            worst["pooled"] = max(worst["pooled"], float((out.pooler_output[0] - c.ref.pooled[b]).abs().max()))
            worst["attn"] = max(worst["attn"], float((attn - c.ref.attn_sum[r:end]).abs().max()))
    print(name, worst)
    assert max(worst.values()) <= TRANSFORMERS_BAR, worst


def test_state_dict_is_the_references():
    """Names and shapes against a reference-shaped module (BertModel where importable, else the
    oracle's own table of them); a strict load both ways; an old checkpoint's position_ids is dropped."""
    from bigcn_amd import TreeBERT
    sizes = dict(hidden=128, heads=2, intermediate=256, num_layers=2, max_pos=32, vocab=R.VOCAB)
    model = TreeBERT(256 * 768, 64, 64, None, **sizes)
    got = model.state_dict()
    want = R.make_state_dict(128, 256, 2, 32, 4, seed=5)
    assert sorted(got) == sorted(want)
    assert {k: tuple(v.shape) for k, v in got.items()} == {k: tuple(v.shape) for k, v in want.items()}
    try:
        import transformers as tr
    except ImportError:
        tr = None
    if tr is not None:
        cfg = tr.BertConfig(vocab_size=R.VOCAB, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
                            intermediate_size=256, max_position_embeddings=32, is_decoder=True)
        holder = torch.nn.Module()
        holder.BERT, holder.fc = tr.BertModel(cfg), torch.nn.Linear(128, 4)
        theirs = {k: v for k, v in holder.state_dict().items() if "position_ids" not in k}
        assert list(got) == list(theirs)
        assert {k: tuple(v.shape) for k, v in got.items()} == {k: tuple(v.shape) for k, v in theirs.items()}
        holder.load_state_dict(got, strict=not any("position_ids" in k for k in holder.state_dict()))
        model.load_state_dict(holder.state_dict(), strict=True)
    model.load_state_dict(want, strict=True)
    for k, v in model.state_dict().items():
        assert torch.equal(v, want[k]), k
    old = dict(want)
    old["BERT.embeddings.position_ids"] = torch.arange(32).unsqueeze(0)
    model.load_state_dict(old, strict=True)
    assert "BERT.embeddings.position_ids" not in model.state_dict()


def test_constructor_and_initialisation():
    from bigcn_amd import TreeBERT
    m = TreeBERT(256 * 768, 64, 64, None, 'mean', 2, hidden=64, heads=1, intermediate=64, num_layers=1, max_pos=8,
                 vocab=R.VOCAB)
    assert (m.in_feats, m.hid_feats, m.out_feats, m.device, m.pooling, m.version) == (256 * 768, 64, 64, None, 'mean', 2)
    assert m.fc.in_features == 64 and m.fc.out_features == 4     # the reference's head: Linear(hidden, 4)
    sd = m.state_dict()
    for k, v in sd.items():
        if "LayerNorm.weight" in k:
            assert torch.equal(v, torch.ones_like(v)), k
        elif k.startswith("BERT.") and k.endswith(".bias"):
            assert torch.equal(v, torch.zeros_like(v)), k
    w = sd["BERT.encoder.layer.0.intermediate.dense.weight"]
    assert 0.015 < float(w.std()) < 0.025
    import bigcn_amd.bert as mod
    assert "transformers" not in vars(mod)


def test_training_mode_version_2_and_cpu_tensors_raise():
    from bigcn_amd import TreeBERT, _lib
    m = TreeBERT(hidden=64, heads=1, intermediate=64, num_layers=1, max_pos=8, vocab=R.VOCAB)
    with pytest.raises(NotImplementedError, match="training"):
        m(torch.zeros(3, 2, 64))
    m.eval()
    with pytest.raises(_lib.BGCNError):
        m(torch.zeros(3, 2, 64))
    with pytest.raises(_lib.BGCNError):
        m.forward_batch(torch.zeros(3, 64), torch.tensor([0]))
    m.version = 2
    with pytest.raises(NotImplementedError, match="more than one node"):
        m.evaluate(None)


def test_binding_lists_the_new_symbols_and_constants():
    import re
    from bigcn_amd import _lib
    for name in ("bgcn_bert_workspace_size", "bgcn_bert_eval"):
        assert name in _lib.EXPORTED_SYMBOLS and name in _lib._SIGS
        assert hasattr(_lib.load_library(), name)
    text = open(HEADER).read()
    for name in ("BGCN_BERT_MAX_LAYERS", "BGCN_BERT_QUERY_TILE"):
        m = re.search(rf"#define {name} (\d+)", text)
        assert m and int(m.group(1)) == getattr(_lib, name), name
    assert R.QUERY_TILE == _lib.BGCN_BERT_QUERY_TILE
    assert re.search(r"#define BGCN_ABI_VERSION 12\b", text)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_struct_layout_matches_header(tmp_path):
    from bigcn_amd import _lib
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {",
             'printf("sizeof %zu\\n", sizeof(bgcn_bert_args));', 'printf("layer_size %zu\\n", sizeof(bgcn_bert_layer));']
    for fname, _ in _lib.BertArgs._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(bgcn_bert_args, {fname}));')
    for fname, _ in _lib.BertLayer._fields_:
        lines.append(f'printf("layer.{fname} %zu\\n", offsetof(bgcn_bert_layer, {fname}));')
    lines.append("return 0; }")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(c)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = dict((line.split()[0], int(line.split()[1])) for line in out if line)
    assert got["sizeof"] == ctypes.sizeof(_lib.BertArgs) and got["layer_size"] == ctypes.sizeof(_lib.BertLayer)
    for fname, _ in _lib.BertArgs._fields_:
        assert got[fname] == getattr(_lib.BertArgs, fname).offset, fname
    for fname, _ in _lib.BertLayer._fields_:
        assert got["layer." + fname] == getattr(_lib.BertLayer, fname).offset, fname


def test_workspace_size():
    from bigcn_amd import _lib
    ws = _lib.load_library().bgcn_bert_workspace_size
    root, full = ws(1000, 24, 768, 3072, 12, 0), ws(1000, 24, 768, 3072, 12, 1)
    assert 0 < root < full
    assert root < 4 * 24 * (5 * 768 + 3072) + 64 * 1024          # the root-only form holds [B, .] buffers only
    assert full >= 4 * 1000 * (7 * 768 + 3072 + 16 * 12)         # h, a, t, ctx, q | k | v, intermediate, partials
    assert ws(1000, 24, 768, 3072, 1, 1) == full                 # the layers share the buffers
    for bad in ((0, 1, 768, 3072, 12), (10, 0, 768, 3072, 12), (10, 2, 96, 3072, 12), (10, 2, 32, 64, 1),
                (10, 2, 1088, 3072, 12), (10, 2, 768, 3080, 12), (10, 2, 768, 32, 12), (10, 2, 768, 4160, 12),
                (10, 2, 768, 3072, 0), (10, 2, 768, 3072, 25)):
        assert ws(*bad, 0) == 0 and ws(*bad, 1) == 0, bad


def test_bad_arguments_fail_before_any_device_work():
    """Fake 16-byte-aligned addresses that are never dereferenced: every rejection happens on the host."""
    from bigcn_amd import _lib
    lib = _lib.load_library()
    fake = 0x10000

    def plausible(full=False):
        a = _lib.BertArgs()
        a.x, a.ldx, a.num_nodes, a.seq_start, a.num_seqs = fake, 128, 10, fake + 0x100, 2
        a.hidden, a.heads, a.intermediate, a.num_layers, a.max_pos, a.out_feats, a.ln_eps = 128, 2, 256, 2, 512, 4, 1e-12
        nxt = iter(range(1, 1000))
        for f in ("pos_emb", "type_emb", "emb_ln_w", "emb_ln_b", "pooler_w", "pooler_b", "fc_w", "fc_b"):
            setattr(a, f, fake + 0x1000 * next(nxt))
        for l in range(2):
            for f, _ in _lib.BertLayer._fields_:
                setattr(a.layer[l], f, fake + 0x1000 * next(nxt))
        a.logp, a.status = fake + 0x1000 * next(nxt), fake + 0x1000 * next(nxt)
        if full:
            a.hidden_out = fake + 0x1000 * next(nxt)
        return a

    def rejected(a, text, ws=None, ws_bytes=0):
        assert lib.bgcn_bert_eval(ctypes.addressof(a), ws, ws_bytes, None) == -1
        assert text in lib.bgcn_last_error(), lib.bgcn_last_error()

    assert lib.bgcn_bert_eval(None, None, 0, None) == -1
    rejected(_lib.BertArgs(), b"unsupported shape")
    rejected(plausible(), b"workspace too small")
    for field, value in (("hidden", 96), ("hidden", 192), ("hidden", 1088), ("heads", 3), ("intermediate", 200),
                         ("intermediate", 32), ("intermediate", 4160), ("num_layers", 0), ("num_layers", 25),
                         ("max_pos", 0), ("max_pos", 513), ("out_feats", 0), ("out_feats", 65), ("num_nodes", 0),
                         ("num_seqs", 0)):
        a = plausible()
        setattr(a, field, value)
        rejected(a, b"unsupported shape")
    for field, value, text in (("x", None, b"null pointer"), ("seq_start", None, b"null pointer"),
                               ("logp", None, b"null pointer"), ("status", None, b"null pointer"),
                               ("ldx", 126, b"16-byte"), ("ldx", 130, b"16-byte"), ("x", fake + 4, b"16-byte"),
                               ("pos_emb", None, b"BERT weight"), ("type_emb", fake + 8, b"BERT weight"),
                               ("fc_w", fake + 0x7004, b"BERT weight"), ("pooler_b", None, b"BERT weight"),
                               ("logp", fake + 0x100004, b"16-byte"), ("hidden_out", fake + 0x200004, b"16-byte"),
                               ("hidden_sum", fake + 0x200008, b"16-byte"), ("attn_sum", fake + 0x20000c, b"16-byte")):
        a = plausible()
        setattr(a, field, value)
        rejected(a, text)
    for f, _ in _lib.BertLayer._fields_:
        a = plausible()
        setattr(a.layer[1], f, None)
        rejected(a, b"BERT weight")
        setattr(a.layer[1], f, fake + 0x300004)
        rejected(a, b"BERT weight")
    # one byte short, in both forms; a misaligned workspace
    for full in (False, True):
        need = lib.bgcn_bert_workspace_size(10, 2, 128, 256, 2, int(full))
        rejected(plausible(full), b"workspace too small", fake + 0x1000000, need - 1)
    rejected(plausible(), b"16-byte", fake + 0x1000004, 1 << 30)


def _case(name):
    return R.case(name) if name in R.CASES else R.edge_case(name)


@pytest.mark.parametrize("name", ALL + EDGES)
def test_the_class_reads_the_root_row_only(name):
    """Replacing every non-root row leaves the oracle's logp exactly unchanged."""
    c = _case(name)
    x = torch.randn(c.x.shape, generator=torch.Generator().manual_seed(77)) * 3.0
    x[c.rootindex] = c.x[c.rootindex]
    got = R.run(c.sd, x, c.rootindex, c.cfg["layers"], c.heads, c.y)
    assert torch.equal(got.logp, c.ref.logp) and torch.equal(got.pred, c.ref.pred)
    assert float(got.loss) == float(c.ref.loss)
    if c.N > c.B + c.first:
        assert not torch.equal(got.hidden, c.ref.hidden)


def test_cases_are_the_table():
    assert ALL == ["boundaries", "cap", "full_width", "many", "offset_strided", "sharp", "single"]
    assert R.CASES["boundaries"]["lengths"] == [1, 2, 31, 32, 33, 63, 64, 65]
    assert R.CASES["cap"]["lengths"] == [512, 511] and R.CASES["cap"]["max_pos"] == 512
    c = R.case("offset_strided")
    assert int(c.rootindex[0]) == 2 and c.x.stride(0) > c.cfg["hidden"]
    c = R.case("many")
    assert c.B == 130 and set(c.cfg["lengths"]) == {1, 2}
    c = R.case("full_width")
    assert (c.cfg["hidden"], c.heads, c.cfg["intermediate"], c.cfg["layers"], c.B, c.N) == (768, 12, 3072, 2, 3, 40)
    assert R.case("single").N == 1
    assert R.case("sharp").ref.top_score > 88.0     # exp(88.8) overflows fp32


@pytest.mark.parametrize("name", [n for n in ALL if n not in ("single", "many")] +
                         ["heads3_tiles", "sharp_tiles", "short_pos", "hidden_1024", "rows_over_switch"])
def test_attention_is_neither_uniform_nor_one_hot(name):
    """The spread condition: among the oracle's attention rows with at least 8 keys there are rows
    whose largest probability is above 0.5 and rows where it is below."""
    rm = _case(name).ref.row_max
    hi, lo = int((rm > 0.5).sum()), int((rm < 0.5).sum())
    print(name, "rows", rm.numel(), "above", hi, "below", lo)
    assert hi > 0 and lo > 0


@pytest.mark.parametrize("name", ALL + EDGES)
def test_the_bar_is_feasible(name):
    """Torch's own fp32 CPU evaluation of the restatement is within 1e-5 of the fp64 oracle on hidden,
    hidden_sum / hidden, logp and the loss, and within 1e-5 max(1, |ref|) on attn_sum, for every GPU
    case at its recorded weight_factor: the arithmetic alone sits 10x under the GPU tests' 1e-4 bar."""
    c = _case(name)
    got = R.run(c.sd, c.x, c.rootindex, c.cfg["layers"], c.heads, c.y, dtype=torch.float32)
    errs = {"hidden": float((got.hidden.double() - c.ref.hidden).abs().max()),
            "hidden_sum/hidden": float((got.hidden_sum.double() - c.ref.hidden_sum).abs().max()) / c.cfg["hidden"],
            "logp": float((got.logp.double() - c.ref.logp).abs().max()),
            "loss": abs(float(got.loss) - float(c.ref.loss)),
            "attn_sum": float(((got.attn_sum.double() - c.ref.attn_sum).abs() / c.ref.attn_sum.abs().clamp(min=1)).max())}
    print(name, {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= 1e-5, errs


@pytest.mark.parametrize("name", ALL + EDGES)
def test_rankings_leave_few_positions_out(name):
    """A condition on the inputs (the seeds): at most 5 % of a case's ranking positions lie within 2e-4
    of a neighbour in the oracle's sorted values, where the GPU test does not compare the order."""
    c = _case(name)
    out = total = 0
    for lst in (c.ref.rank_hidden, c.ref.rank_attn):
        for _, v in lst:
            ok = R.rank_compared(v)
            out += int((~ok).sum())
            total += ok.numel()
    print(name, "left out", out, "of", total)
    assert out <= R.RANK_SKIP * total


def test_edge_cases_are_the_table():
    """N, B, heads and the size each edge case exists for, the limits read from the sources."""
    import re
    from bigcn_amd import _lib
    assert EDGES == ["classes_1", "classes_63", "classes_64", "heads3_tiles", "hidden_1024", "hidden_320", "layers_24",
                     "many_trees", "rows_over_switch", "sharp_tiles", "short_pos"]
    assert len({c["seed"] for c in R.EDGE_CASES.values()}) == len(EDGES)
    table = {"many_trees": (603, 300, 1), "heads3_tiles": (200, 4, 3), "sharp_tiles": (170, 2, 2),
             "hidden_1024": (45, 2, 16), "hidden_320": (37, 2, 5), "layers_24": (43, 3, 1), "classes_1": (20, 5, 2),
             "classes_63": (20, 5, 2), "classes_64": (20, 5, 2), "short_pos": (87, 3, 2),
             "rows_over_switch": (8217, 127, 2)}
    for name, want in table.items():
        c = R.edge_case(name)
        assert (c.N, c.B, c.heads) == want, name
    cfg = R.EDGE_CASES
    c = R.edge_case("many_trees")
    assert c.B > 256 and c.first == 3 and set(cfg["many_trees"]["lengths"]) == {1, 2, 3}     # k_bert_setup's stride
    assert cfg["heads3_tiles"]["lengths"] == [70, 33, 1, 96] and (96 - 1) // R.QUERY_TILE == 2
    assert cfg["sharp_tiles"]["lengths"] == [70, 100] and cfg["sharp_tiles"]["qk_factor"] > 1
    bert = open(os.path.join(ROOT, "bigcn_amd", "csrc", "bgcn_bert.hip")).read()
    assert cfg["hidden_1024"]["hidden"] == int(re.search(r"kMaxHidden = (\d+);", bert).group(1))
    assert cfg["hidden_320"]["hidden"] % 256 == 64 and cfg["hidden_320"]["intermediate"] == 4096
    assert _lib.load_library().bgcn_bert_workspace_size(37, 2, 320, 4096 + 64, 1, 1) == 0    # 4096 is the largest
    assert cfg["layers_24"]["layers"] == _lib.BGCN_BERT_MAX_LAYERS
    assert int(re.search(r"#define BGCN_BERT_MAX_LAYERS (\d+)", open(HEADER).read()).group(1)) == 24
    lstm_h = open(os.path.join(ROOT, "bigcn_amd", "csrc", "bgcn_lstm.h")).read()
    assert cfg["classes_64"]["out"] == int(re.search(r"kMaxOut = (\d+);", lstm_h).group(1))
    assert (cfg["classes_1"]["out"], cfg["classes_63"]["out"]) == (1, 63)
    c = R.edge_case("short_pos")
    assert c.cfg["max_pos"] == 40 == max(c.cfg["lengths"]) and 40 % 32 and c.sd[
        "BERT.embeddings.position_embeddings.weight"].size(0) == 40
    x6 = int(re.search(r"kX6MinRows = (\d+);", open(INTERNAL).read()).group(1))
    c = R.edge_case("rows_over_switch")
    assert c.N >= x6 > c.B and c.cfg["hidden"] % 128 == 0 and c.cfg["intermediate"] % 128 == 0
    under = [n for n in ALL + EDGES if n != "rows_over_switch"]
    assert all(_case(n).N < x6 for n in under)         # every other case runs the exact-fp32 GEMM alone


@pytest.mark.parametrize("name", EDGES)
def test_predictions_have_a_margin(name):
    """A condition on the inputs: the oracle's smallest top-1 to top-2 gap in logp over the trees is
    above 2e-4, twice the GPU bar, so a GPU logp inside the bar has the oracle's argmax and the GPU
    tests may assert ``pred`` equal."""
    gap = R.pred_gap(R.edge_case(name).ref.logp)
    print(name, "smallest gap", gap)
    assert gap > R.PRED_GAP


def test_sharp_tiles_crosses_key_tiles_both_ways():
    """The rows at positions >= 64 of head 0 (three key tiles): there are rows whose largest score
    sits in a later key tile, more than 10 above the first tile's largest (the running maximum moves
    and the sum so far shrinks by e^-10 or more), and rows where the first tile's largest is more than
    10 above every later key's.  A missing or misplaced rescale factor is then wrong by e^10.  The
    largest score passes +-88 as well: exp overflows fp32 without the max subtraction."""
    c = R.edge_case("sharp_tiles")
    gap = torch.cat([layers[0][64:] for layers in c.ref.tile_gap])
    later, first = int((gap > R.TILE_GAP).sum()), int((gap < -R.TILE_GAP).sum())
    print("rows", gap.numel(), "later tile leads", later, "first tile leads", first, "top score", c.ref.top_score)
    assert gap.numel() == 6 + 36 and not bool(torch.isnan(gap).any())
    assert later > 0 and first > 0
    assert c.ref.top_score > 88.0
