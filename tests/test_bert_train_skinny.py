"""CPU checks of the skinny fp32 GEMMs' and bgcn_bert_train_grad_skinny's boundary: the size functions,
and the argument checks that come before any HIP call (the pointers are fake 16-byte-aligned addresses
that are never dereferenced, as in tests/test_capi.py)."""
import ctypes

FAKE = 0x100000
BASE = dict(N=600, B=24, hidden=768, intermediate=3072, layers=12)   # BERT-base, the workload's batch


def _lib():
    from bigcn_amd import _lib
    return _lib, _lib.load_library()


def _rejected(lib, rc, text):
    assert rc == -1
    assert text in lib.bgcn_last_error(), lib.bgcn_last_error()


def test_the_gemm_size_function():
    _, lib = _lib()
    size = lib.bgcn_gemm_skinny_workspace_size
    for M, Nc, K in ((24, 96, 768), (24, 768, 32), (24, 768, 4160), (24, 4160, 768), (24, 32, 768), (0, 768, 768),
                     (-1, 768, 768)):
        assert size(M, Nc, K) == 0, (M, Nc, K)
    for Nc, K in ((768, 768), (3072, 768), (768, 3072), (64, 64), (4096, 4096)):
        sizes = [size(M, Nc, K) for M in (1, 2, 24, 25, 129, 300)]
        assert all(s > 0 and s % 256 == 0 for s in sizes), (Nc, K, sizes)
        assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
        # at least one partial of the wider of the two split products
        assert size(24, Nc, K) >= 4 * 24 * max(Nc, K)


def test_the_training_size_function():
    _, lib = _lib()
    size = lib.bgcn_bert_train_skinny_workspace_size
    b = BASE
    assert size(10, 2, 100, 256, 2) == 0    # hidden % 64
    assert size(10, 2, 128, 200, 2) == 0    # intermediate % 64
    assert size(10, 2, 128, 256, 25) == 0   # layers
    assert size(10, 0, 128, 256, 2) == 0    # no tree
    assert size(10, 2, 1088, 256, 2) == 0   # hidden over 1024
    need = size(b["N"], b["B"], b["hidden"], b["intermediate"], b["layers"])
    assert need > 0 and need % 256 == 0
    sizes = [size(8 * B, B, b["hidden"], b["intermediate"], b["layers"]) for B in (1, 2, 23, 24, 25, 128, 129, 300)]
    assert all(s > 0 and s % 256 == 0 for s in sizes)
    assert all(u < v for u, v in zip(sizes, sizes[1:]))
    # it holds the partials of the widest product
    assert need >= lib.bgcn_gemm_skinny_workspace_size(b["B"], b["hidden"], b["intermediate"])


def test_the_gemms_refuse_before_any_hip_call():
    _, lib = _lib()
    M, Nc, K = 24, 768, 3072
    need = lib.bgcn_gemm_skinny_workspace_size(M, Nc, K)
    X, W, Y, G, WS = FAKE, FAKE + 0x1000, FAKE + 0x2000, FAKE + 0x3000, FAKE + 0x4000

    def xwt(x=X, ldx=K, w=W, ldw=K, bias=0, y=Y, ldy=Nc, m=M, nc=Nc, k=K, ws=WS, nb=need):
        return lib.bgcn_gemm_xwt_skinny(x, ldx, w, ldw, bias, y, ldy, m, nc, k, ws, nb, None)

    def xw(g=G, ldg=Nc, w=W, ldw=K, y=Y, ldy=K, m=M, nc=Nc, k=K, ws=WS, nb=need):
        return lib.bgcn_gemm_xw_skinny(g, ldg, w, ldw, y, ldy, m, nc, k, ws, nb, None)

    def tn(g=G, ldg=Nc, x=X, ldx=K, w=W, ldw=K, m=M, nc=Nc, k=K):   # w: dW, the output
        return lib.bgcn_gemm_tn_skinny(g, ldg, x, ldx, w, ldw, m, nc, k, None)

    for call in (xwt, xw, tn):
        for bad in (dict(nc=96), dict(k=32), dict(k=4160), dict(m=0)):
            _rejected(lib, call(**bad), b"unsupported shape")
        _rejected(lib, call(ldw=K - 4), b"at least the row width")
        _rejected(lib, call(ldw=K + 2), b"at least the row width")
        _rejected(lib, call(w=W + 4), b"16-byte aligned")
        _rejected(lib, call(w=0), b"non-null")
    _rejected(lib, xwt(ldx=K - 4), b"at least the row width")
    _rejected(lib, xwt(ldy=Nc - 4), b"at least the row width")
    _rejected(lib, xwt(bias=FAKE + 8), b"16-byte aligned")
    _rejected(lib, xw(ldg=Nc - 4), b"at least the row width")
    _rejected(lib, xw(ldy=K - 4), b"at least the row width")
    _rejected(lib, tn(ldg=Nc - 4), b"at least the row width")
    _rejected(lib, tn(ldx=K - 4), b"at least the row width")
    for call in (xwt, xw):
        _rejected(lib, call(nb=need - 256), b"workspace too small")
        _rejected(lib, call(ws=0), b"workspace too small")
        _rejected(lib, call(ws=WS + 4), b"workspace too small")


def _plausible(L, hidden=128, intermediate=256, layers=2, N=20, B=5):
    """bgcn_bert_train_args whose every pointer is a distinct fake aligned address."""
    t = L.BertTrainArgs()
    nxt = iter(range(FAKE, FAKE + (1 << 24), 0x100))
    a = t.fwd
    a.x, a.ldx, a.num_nodes, a.seq_start, a.num_seqs = next(nxt), hidden, N, next(nxt), B
    a.hidden, a.heads, a.intermediate, a.num_layers = hidden, hidden // 64, intermediate, layers
    a.max_pos, a.out_feats, a.ln_eps = 512, 4, 1e-12
    for field in ("pos_emb", "type_emb", "emb_ln_w", "emb_ln_b", "pooler_w", "pooler_b", "fc_w", "fc_b"):
        setattr(a, field, next(nxt))
        setattr(t, "d_" + field, next(nxt))
    for i in range(layers):
        for field, _ in L.BertLayer._fields_:
            setattr(a.layer[i], field, next(nxt))
            setattr(t.d_layer[i], field, next(nxt))
    a.y, a.logp, a.status, a.loss, a.correct = (next(nxt) for _ in range(5))
    t.skip_flag, t.hidden_dropout, t.attn_dropout = next(nxt), 0.1, 0.1
    return t


def test_the_training_call_refuses_before_any_hip_call():
    L, lib = _lib()
    grad = lib.bgcn_bert_train_grad_skinny
    ws = FAKE + (1 << 25)
    _rejected(lib, grad(None, ws, 1 << 30, None), b"null args")
    t = _plausible(L)
    need = lib.bgcn_bert_train_skinny_workspace_size(20, 5, 128, 256, 2)
    assert need > 0
    _rejected(lib, grad(ctypes.addressof(t), ws, need - 256, None), b"workspace too small")
    _rejected(lib, grad(ctypes.addressof(t), None, 0, None), b"workspace too small")
    # bgcn_bert_train_grad's own conditions, before the workspace's
    t = _plausible(L)
    t.hidden_dropout = 1.0
    _rejected(lib, grad(ctypes.addressof(t), ws, need, None), b"dropout rate")
    t = _plausible(L)
    t.skip_flag = None
    _rejected(lib, grad(ctypes.addressof(t), ws, need, None), b"null pointer")
    t = _plausible(L)
    t.d_layer[1].o_w = None
    _rejected(lib, grad(ctypes.addressof(t), ws, need, None), b"null or unaligned BERT weight gradient")
    t = _plausible(L)
    t.fwd.hidden_out = FAKE
    _rejected(lib, grad(ctypes.addressof(t), ws, need, None), b"root-only")
    t = _plausible(L)
    t.fwd.hidden = 100
    _rejected(lib, grad(ctypes.addressof(t), ws, need, None), b"unsupported shape")
