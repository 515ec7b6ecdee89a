"""CPU checks of TreeBERT's bf16 weight-image mode: the conditions the GPU tests' inputs must meet
(tests/test_gpu_bert_w16.py), the size queries and argument checks of the new entry points (no GPU, no
HIP call: fake 16-byte-aligned pointers that are never dereferenced, as tests/test_capi.py), and that
the mode leaves ``state_dict()`` alone."""
import ctypes

import pytest
import torch

import bert_ref as R
import bert_w16_ref as W16

FAKE = 0x10000


# ---- (a) the oracle's conditions on the cases
@pytest.mark.parametrize("name", W16.CASES)
def test_oracle_conditions(name):
    c = W16.case(name)
    o = W16.oracle(name)
    # every tree's class is decided by more than twice the bar
    assert R.pred_gap(o.logp) > R.PRED_GAP, R.pred_gap(o.logp)
    # the rounding of the weights shows: the fp32 path cannot pass the parity test of the mode
    moved = float((o.logp - W16.root_run(c, c.sd).logp).abs().max())
    if name != "classes_1":          # one class: logp is 0 whatever the weights
        assert moved > 2 * W16.BAR, moved
    else:
        assert moved == 0.0


def test_only_the_chain_weights_are_rounded():
    c = W16.case("single")
    sd = W16.rounded_state_dict(c.sd, c.cfg["layers"])
    changed = sorted(k for k in sd if not torch.equal(sd[k], c.sd[k]))
    assert changed == sorted([f"BERT.encoder.layer.{i}.{n}" for i in range(c.cfg["layers"]) for n in W16.ROUNDED]
                             + ["BERT.pooler.dense.weight"])


# ---- (b) size queries
def test_size_queries_without_gpu():
    from bigcn_amd import _lib
    lib = _lib.load_library()
    for Nc, K in ((64, 64), (768, 768), (3072, 768), (768, 3072), (320, 4096), (4096, 4096)):
        assert lib.bgcn_w16_image_size(Nc, K) >= 2 * Nc * K
        assert lib.bgcn_gemm_xwt_w16_workspace_size(24, Nc, K) >= 4 * 24 * Nc
    assert lib.bgcn_w16_image_size(96, 64) == 0
    assert lib.bgcn_w16_image_size(64, 4160) == 0
    assert lib.bgcn_w16_image_size(0, 64) == 0
    assert lib.bgcn_gemm_xwt_w16_workspace_size(24, 96, 64) == 0
    assert lib.bgcn_gemm_xwt_w16_workspace_size(0, 64, 64) == 0
    base = lib.bgcn_bert_w16_workspace_size(24, 768, 3072, 12)
    assert base > lib.bgcn_bert_workspace_size(24, 24, 768, 3072, 12, 0) > 0
    assert lib.bgcn_bert_w16_workspace_size(300, 768, 3072, 12) > base
    assert lib.bgcn_bert_w16_workspace_size(24, 100, 3072, 12) == 0
    assert lib.bgcn_bert_w16_workspace_size(24, 768, 3072, 25) == 0
    # the workspace of M rows is M times one row's (the split does not depend on M)
    one = lib.bgcn_gemm_xwt_w16_workspace_size(1, 768, 768)
    assert lib.bgcn_gemm_xwt_w16_workspace_size(64, 768, 768) == 64 * one


# ---- (c) argument checks before any HIP call
def _rejected(lib, rc, text):
    assert rc == -1
    assert text in lib.bgcn_last_error(), lib.bgcn_last_error()


def test_kernel_entry_points_reject_malformed_calls():
    from bigcn_amd import _lib
    lib = _lib.load_library()
    X, IMG, Y, WS = FAKE, FAKE + 0x10000, FAKE + 0x20000, FAKE + 0x30000
    M, Nc, K = 24, 128, 64
    need = lib.bgcn_gemm_xwt_w16_workspace_size(M, Nc, K)

    def gemm(x=X, ldx=K, img=IMG, bias=None, y=Y, ldy=Nc, m=M, nc=Nc, k=K, ws=WS, nbytes=need):
        return lib.bgcn_gemm_xwt_w16(x, ldx, img, bias, y, ldy, m, nc, k, ws, nbytes, None)

    _rejected(lib, gemm(nc=96), b"unsupported shape")
    _rejected(lib, gemm(k=4160), b"unsupported shape")
    _rejected(lib, gemm(m=0), b"unsupported shape")
    _rejected(lib, gemm(x=None), b"null pointer")
    _rejected(lib, gemm(y=None), b"null pointer")
    _rejected(lib, gemm(ldx=K - 4), b"16-byte aligned")
    _rejected(lib, gemm(ldx=K + 1), b"16-byte aligned")
    _rejected(lib, gemm(ldy=Nc + 2), b"16-byte aligned")
    _rejected(lib, gemm(x=X + 4), b"16-byte aligned")
    _rejected(lib, gemm(bias=FAKE + 8), b"16-byte aligned")
    _rejected(lib, gemm(img=None), b"null or unaligned weight image")
    _rejected(lib, gemm(img=IMG + 8), b"null or unaligned weight image")
    _rejected(lib, gemm(ws=None), b"workspace too small")
    _rejected(lib, gemm(nbytes=need - 1), b"workspace too small")

    _rejected(lib, lib.bgcn_w16_pack(X, K, 96, K, IMG, None), b"unsupported shape")
    _rejected(lib, lib.bgcn_w16_pack(None, K, Nc, K, IMG, None), b"null W")
    _rejected(lib, lib.bgcn_w16_pack(X, K - 1, Nc, K, IMG, None), b"ldw < K")
    _rejected(lib, lib.bgcn_w16_pack(X, K, Nc, K, None, None), b"null or unaligned weight image")
    _rejected(lib, lib.bgcn_w16_pack(X, K, Nc, K, IMG + 2, None), b"null or unaligned weight image")


def _plausible(lib, B=3, H=128, inter=256, L=2):
    from bigcn_amd import _lib
    wa = _lib.BertW16Args()
    a = wa.base
    a.x, a.ldx, a.num_nodes, a.seq_start, a.num_seqs = FAKE, H, 10, FAKE + 0x100, B
    a.hidden, a.heads, a.intermediate, a.num_layers, a.max_pos, a.out_feats, a.ln_eps = H, H // 64, inter, L, 512, 4, 1e-12
    nxt = iter(range(FAKE + 0x1000, FAKE + 0x100000, 0x100))
    for f in ("pos_emb", "type_emb", "emb_ln_w", "emb_ln_b", "pooler_w", "pooler_b", "fc_w", "fc_b", "logp", "status"):
        setattr(a, f, next(nxt))
    for i in range(L):
        for f, _ in _lib.BertLayer._fields_:
            setattr(a.layer[i], f, next(nxt))
        for f in ("v_w16", "ao_w16", "i_w16", "o_w16"):
            getattr(wa, f)[i] = next(nxt)
    wa.pooler_w16 = next(nxt)
    return wa


def test_bert_eval_w16_rejects_malformed_calls():
    from bigcn_amd import _lib
    lib = _lib.load_library()
    WS = FAKE + 0x200000
    need = lib.bgcn_bert_w16_workspace_size(3, 128, 256, 2)
    assert need > 0

    def call(wa, ws=WS, nbytes=need):
        return lib.bgcn_bert_eval_w16(ctypes.addressof(wa) if wa is not None else None, ws, nbytes, None)

    _rejected(lib, call(None), b"null args")
    # the fp32 call's conditions, through `base`
    wa = _plausible(lib)
    wa.base.hidden = 100
    _rejected(lib, call(wa), b"unsupported shape")
    wa = _plausible(lib)
    wa.base.logp = None
    _rejected(lib, call(wa), b"null pointer")
    wa = _plausible(lib)
    wa.base.layer[1].o_ln_b = None
    _rejected(lib, call(wa), b"null or unaligned BERT weight")
    wa = _plausible(lib)
    wa.base.ldx = 130
    _rejected(lib, call(wa), b"x rows must be 16-byte aligned")
    # a full-form output
    for f in ("hidden_out", "hidden_sum", "attn_sum"):
        wa = _plausible(lib)
        setattr(wa.base, f, FAKE + 0x300000)
        _rejected(lib, call(wa), b"root-only form")
    # the images
    for f in ("v_w16", "ao_w16", "i_w16", "o_w16"):
        wa = _plausible(lib)
        getattr(wa, f)[1] = None
        _rejected(lib, call(wa), b"null or unaligned weight image")
        wa = _plausible(lib)
        getattr(wa, f)[0] = FAKE + 0x400008
        _rejected(lib, call(wa), b"null or unaligned weight image")
    wa = _plausible(lib)
    wa.pooler_w16 = None
    _rejected(lib, call(wa), b"null or unaligned weight image")
    # an image slot past num_layers is not looked at; then the workspace
    wa = _plausible(lib)
    wa.v_w16[2] = None
    _rejected(lib, call(wa, ws=None, nbytes=0), b"workspace too small")
    _rejected(lib, call(_plausible(lib), nbytes=need - 1), b"workspace too small")
    # the fp32 root-only workspace is too small for this call
    _rejected(lib, call(_plausible(lib), nbytes=lib.bgcn_bert_workspace_size(10, 3, 128, 256, 2, 0)),
              b"workspace too small")


# ---- (d) the mode is no part of the state
def test_mode_leaves_the_state_dict_alone():
    from bigcn_amd import TreeBERT
    c = W16.case("single")
    plain = R.model_for(c)
    m = R.model_for(c)
    assert m.weight_images is None
    assert m.use_weight_images("bf16") is m and m.weight_images == "bf16"
    assert list(m.state_dict()) == list(plain.state_dict())
    assert [n for n, _ in m.named_buffers()] == [n for n, _ in plain.named_buffers()]
    assert all(torch.equal(v, plain.state_dict()[k]) for k, v in m.state_dict().items())
    res = m.load_state_dict(c.sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    fresh = TreeBERT(hidden=128, heads=2, intermediate=256, num_layers=2, vocab=R.VOCAB)
    fresh.load_state_dict(m.state_dict(), strict=True)
    m.use_weight_images(None)
    assert m.weight_images is None
    with pytest.raises(ValueError):
        m.use_weight_images("fp8")
    assert m.weight_images is None
