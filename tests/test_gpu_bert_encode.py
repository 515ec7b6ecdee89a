"""GPU checks of the PHEME feature extraction (bgcn_bert_encode, bigcn_amd.TweetEncoder) against the fp64
oracle of tests/bert_encode_ref.py at bert_gpu_util's bar (1e-4 absolute), and the properties that hold by
construction: sequences are independent (every kernel's rows, and the attention's (sequence, head) pairs,
read their own sequence only; the exact-fp32 GEMM's rows are independent k-ordered chains), no float atomics.
"""
import ctypes
import functools

import pytest
import torch

import bert_encode_ref as E
import bert_ref as R
from bert_gpu_util import BAR, DEV, _err

pytestmark = pytest.mark.gpu

assert BAR == E.BAR


@functools.lru_cache(maxsize=None)
def _model(name):
    return E.model_for(E.case(name), DEV)


@functools.lru_cache(maxsize=None)
def _ids(name):
    return E.case(name).ids.to(DEV)


def _check(name, what, got, want):
    err = _err(got, want)
    print(name, what, f"{err:.3e}")
    assert torch.isfinite(got).all(), (name, what)
    assert err <= BAR, (name, what, err)


# ---------------------------------------------------------------- 4. parity at the tile edges
@pytest.mark.parametrize("name", [n for n in sorted(E.CASES) if n.startswith("t")])
def test_parity_with_the_fp64_oracle(name):
    c, m, ids = E.case(name), _model(name), _ids(name)
    n, T, H = c.cfg["n"], c.cfg["T"], c.cfg["hidden"]
    emb, cls = m.encode(ids)
    emb_f, cls_f, hid = m.encode(ids, return_hidden=True)
    only = m.embed(ids)
    m.check_status()
    assert emb.shape == (n, T, H) and cls.shape == (n, H) and hid.shape == (n, T, H)
    _check(name, "embeddings", emb, c.ref.embeddings)
    _check(name, "cls", cls, c.ref.cls)
    _check(name, "cls (full last layer)", cls_f, c.ref.cls)
    _check(name, "last_hidden_state", hid, c.ref.hidden)
    assert torch.equal(emb_f, emb) and torch.equal(only, emb)


def test_int32_ids_are_converted():
    m, ids = _model("t33_n3"), _ids("t33_n3")
    a, b = m.encode(ids), m.encode(ids.to(torch.int32))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---------------------------------------------------------------- 5. the moving maximum
def test_running_maximum_moves_across_key_tiles():
    c, m, ids = E.case("sharp"), _model("sharp"), _ids("sharp")
    gap = c.ref.tile_gap[0]
    assert int((gap > E.TILE_GAP).sum()) >= 8 and int((gap < -E.TILE_GAP).sum()) >= 8
    emb, cls, hid = m.encode(ids, return_hidden=True)
    _check("sharp", "last_hidden_state", hid, c.ref.hidden)
    _check("sharp", "cls (full last layer)", cls, c.ref.cls)
    _check("sharp", "cls", m.encode(ids)[1], c.ref.cls)
    m.check_status()


# ---------------------------------------------------------------- 6. CLS-only against full
@pytest.mark.parametrize("name", ["t70_n3", "t129_n5", "t192_n1"])
def test_cls_only_last_layer_agrees_with_the_full_one(name):
    c, m, ids = E.case(name), _model(name), _ids(name)
    cls = m.encode(ids)[1]
    cls_f = m.encode(ids, return_hidden=True)[1]
    _check(name, "cls", cls, c.ref.cls)
    _check(name, "cls (full last layer)", cls_f, c.ref.cls)
    _check(name, "cls against cls (full last layer)", cls, cls_f.double().cpu())


def _raw_call(m, ids, **fields):
    """bgcn_bert_encode on the module's own argument struct with ``fields`` overwritten -> (rc, message)."""
    from bigcn_amd import _lib
    m.encode(ids)
    torch.cuda.synchronize()
    st = m.__dict__["_state"]
    a = _lib.BertEncodeArgs()
    ctypes.memmove(ctypes.addressof(a), ctypes.addressof(st["args"]), ctypes.sizeof(a))
    n, T = ids.shape
    keep = [torch.empty(n * T, m.hidden, device=DEV) for _ in range(2)] + [torch.empty(n, m.hidden, device=DEV)]
    a.embeddings, a.hidden_out, a.cls = keep[0].data_ptr(), 0, keep[2].data_ptr()
    a.last_layer_full = a.embed_only = 0
    for k, v in fields.items():
        setattr(a, k, keep[1].data_ptr() if v == "buffer" else v)
    ws = st["ws"]["encode"]
    ws_bytes = fields.get("ws_bytes", ws.numel())
    rc = _lib.lib().bgcn_bert_encode(ctypes.addressof(a), ws.data_ptr(), ws_bytes, _lib.stream_handle())
    torch.cuda.synchronize()
    return rc, _lib.lib().bgcn_last_error()


def test_hidden_out_with_the_cls_only_layer_is_refused():
    m, ids = _model("t33_n3"), _ids("t33_n3")
    rc, msg = _raw_call(m, ids, hidden_out="buffer")
    assert rc == -1 and b"hidden_out needs last_layer_full" in msg
    rc, msg = _raw_call(m, ids, hidden_out="buffer", last_layer_full=1)
    assert rc == 0


# ---------------------------------------------------------------- 7. both GEMM paths
def test_both_gemm_paths_and_their_agreement():
    at, under = E.case("rows_at_switch"), E.case("rows_under_switch")
    m = _model("rows_at_switch")
    ids = _ids("rows_at_switch")
    assert ids.numel() == 8192
    emb_a, cls_a, hid_a = m.encode(ids, return_hidden=True)
    emb_u, cls_u, hid_u = m.encode(ids[:63], return_hidden=True)
    cls_a0, cls_u0 = m.encode(ids)[1], m.encode(ids[:63])[1]
    m.check_status()
    for what, got, c in (("at", (emb_a, cls_a, hid_a, cls_a0), at), ("under", (emb_u, cls_u, hid_u, cls_u0), under)):
        _check(what, "embeddings", got[0], c.ref.embeddings)
        _check(what, "cls (full last layer)", got[1], c.ref.cls)
        _check(what, "last_hidden_state", got[2], c.ref.hidden)
        _check(what, "cls", got[3], c.ref.cls)
    _check("at against under", "last_hidden_state", hid_a[:63], hid_u.double().cpu())
    _check("at against under", "cls (full last layer)", cls_a[:63], cls_u.double().cpu())
    _check("at against under", "cls", cls_a0[:63], cls_u0.double().cpu())
    assert torch.equal(emb_a[:63], emb_u)   # the embeddings run no GEMM


# ---------------------------------------------------------------- 8. invariance
@pytest.mark.parametrize("name", ["t70_n5", "t129_n5"])
def test_permuting_the_sequences_permutes_the_results_bit_for_bit(name):
    m, ids = _model(name), _ids(name)
    perm = torch.tensor([3, 0, 4, 1, 2], device=DEV)
    emb, cls, hid = m.encode(ids, return_hidden=True)
    emb_p, cls_p, hid_p = m.encode(ids[perm], return_hidden=True)
    assert torch.equal(emb_p, emb[perm]) and torch.equal(cls_p, cls[perm]) and torch.equal(hid_p, hid[perm])
    cls0, cls0_p = m.encode(ids)[1], m.encode(ids[perm])[1]
    assert torch.equal(cls0_p, cls0[perm])


def test_two_identical_calls_are_bit_identical():
    m, ids = _model("t129_n5"), _ids("t129_n5")
    a = m.encode(ids, return_hidden=True)
    m.encode(ids[:2])   # another shape in between
    b = m.encode(ids, return_hidden=True)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert torch.equal(m.encode(ids)[1], m.encode(ids)[1])


def test_features_in_chunks_and_the_reference_shapes():
    c, m, ids = E.case("t33_n5"), _model("t33_n5"), _ids("t33_n5")
    n, T, H = 5, 33, c.cfg["hidden"]
    one, two = m.features(ids, max_seqs=64), m.features(ids, max_seqs=2)
    m.check_status()
    for f in (one, two):
        assert f["x"].shape == (n, T * H) and f["cls"].shape == (n, H) and f["root"].shape == (1, T * H)
        assert torch.equal(f["root"], f["x"][0:1])
        _check("features", "x", f["x"].view(n, T, H), c.ref.embeddings)
        _check("features", "cls", f["cls"], c.ref.cls)
    _check("features in chunks", "x", two["x"], one["x"].double().cpu())
    _check("features in chunks", "cls", two["cls"], one["cls"].double().cpu())
    assert torch.equal(m.features(ids, root_index=3)["root"], one["x"][3:4])


# ---------------------------------------------------------------- 9. validity
@pytest.mark.parametrize("bad", ["vocab", -1])
def test_a_token_id_outside_the_vocabulary_is_flagged_and_clamped(bad):
    """Input validation on in-bounds reads: the kernel clamps the id before it reads a row."""
    from bigcn_amd import _lib
    c, m = E.case("t70_n3"), _model("t70_n3")
    ids = _ids("t70_n3").clone()
    good_emb, good_cls, good_hid = m.encode(ids, return_hidden=True)
    m.check_status()
    ids[1, 5] = c.cfg["vocab"] if bad == "vocab" else -1
    emb, cls, hid = m.encode(ids, return_hidden=True)
    assert int(m.__dict__["_state"]["status"].item()) == _lib.BGCN_STATUS_TOKEN
    cls0 = m.encode(ids)[1]
    only = m.embed(ids)
    for t in (emb, cls, hid, cls0, only):
        assert torch.isfinite(t).all()
    for b in (0, 2):   # no other sequence's result changes
        assert torch.equal(emb[b], good_emb[b]) and torch.equal(cls[b], good_cls[b]) and torch.equal(hid[b], good_hid[b])
        assert torch.equal(only[b], good_emb[b])
    with pytest.raises(IndexError, match="token id"):
        m.check_status()
    m.check_status()   # reported once
    m.encode(_ids("t70_n3"))
    assert int(m.__dict__["_state"]["status"].item()) == 0
    m.check_status()


def test_argument_checks_return_einval_before_any_launch():
    m, ids = _model("t33_n3"), _ids("t33_n3")
    before = m.encode(ids)[1].clone()
    for fields, text in (({"seq_len": 193}, b"seq_len must be in [1, max_pos]"), ({"seq_len": 0}, b"unsupported shape"),
                         ({"max_pos": 513}, b"unsupported shape"), ({"vocab": 0}, b"vocab"),
                         ({"heads": 3}, b"unsupported shape"), ({"num_seqs": 0}, b"unsupported shape"),
                         ({"word_emb": 0}, b"null or unaligned BERT weight"), ({"cls": 0}, b"null output"),
                         ({"pooler_b": m.pooler.dense.bias.data_ptr() + 4}, b"null or unaligned BERT weight"),
                         ({"ld_embeddings": 130}, b"16-byte aligned"), ({"ws_bytes": 1024}, b"workspace too small")):
        rc, msg = _raw_call(m, ids, **fields)
        assert rc == -1 and text in msg, (fields, msg)
    assert torch.equal(m.encode(ids)[1], before)


# ---------------------------------------------------------------- 10. strict loading, parameters read in place
def test_stripped_treebert_weights_and_a_rebinding_move():
    from bigcn_amd import TreeBERT, TweetEncoder
    sd = R.make_state_dict(128, 128, 2, 64, 4, seed=3, weight_factor=6.0)
    own = {k[len("BERT."):]: v for k, v in sd.items() if k.startswith("BERT.")}
    m = TweetEncoder(hidden=128, heads=2, intermediate=128, num_layers=2, max_pos=64, vocab=R.VOCAB)
    m.load_state_dict(own, strict=True)
    ids = E.make_ids(3, 40, R.VOCAB, torch.Generator().manual_seed(9))
    ref = E.run(own, ids, 2, 2)
    m = m.to(DEV)
    emb, cls = m.encode(ids.to(DEV))
    _check("stripped", "embeddings", emb, ref.embeddings)
    _check("stripped", "cls", cls, ref.cls)
    # a rebinding .to(): new tensors behind the same names, picked up by the next call
    m = m.to(torch.float64)
    with torch.no_grad():
        m.pooler.dense.bias.add_(0.25)
    m = m.to(torch.float32)
    own2 = dict(own, **{"pooler.dense.bias": own["pooler.dense.bias"] + 0.25})
    _check("stripped, moved", "cls", m.encode(ids.to(DEV))[1], E.run(own2, ids, 2, 2).cls)
    # an in-place write is read in place
    with torch.no_grad():
        m.pooler.dense.bias.sub_(0.25)
    _check("stripped, written", "cls", m.encode(ids.to(DEV))[1], ref.cls)
    # the encoder of a TreeBERT reads that module's tensors
    t = TreeBERT(hidden=128, heads=2, intermediate=128, num_layers=2, max_pos=64, vocab=R.VOCAB)
    t.load_state_dict(sd, strict=True)
    t = t.to(DEV)
    e = TweetEncoder.from_treebert(t)
    _check("from_treebert", "cls", e.encode(ids.to(DEV))[1], ref.cls)
    m.check_status()
    e.check_status()
