"""GPU tests of the bf16 weight images: the pack kernel and the skinny-M split-K GEMM on their own
(bgcn_w16_pack, bgcn_gemm_xwt_w16), and TreeBERT's root-only calls on them (bgcn_bert_eval_w16,
``TreeBERT.use_weight_images("bf16")``) against the rounded-weight fp64 oracle of tests/bert_w16_ref.py.

Exact operands (tests of the kernel alone).  W holds small integers, at most 16 nonzeros of magnitude <= 4 per
row; X holds a + b 2^-8 + c 2^-16 with integers |a|, |b|, |c| <= 3, so that all three bf16 planes of the
split carry bits.  Every plane is a multiple of 2^-16 and sum_k |x w| <= 16 * 4 * 3.02 * 1.01 < 2^8 per
output, so every partial sum in any order is an fp32 number: the fp64 product cast to fp32 is THE result,
whatever the split of K.

Random operands.  Per element |got - fp64(X . W16^T)| <= (K + 4) 2^-24 sum_k |x_k w_k|: K fp32 roundings
of the running sum (each at most 2^-24 of a partial sum bounded by sum |x w|), and 4 more for what the
three-plane split of x leaves out and the order of the planes.  A derived worst case, not a measurement."""
import ctypes
import json
import os

import pytest
import torch

import bert_ref as R
import bert_w16_ref as W16
from bert_gpu_util import BAR, DEV, _data, _inputs, _model

pytestmark = pytest.mark.gpu

SHAPES = ((64, 64), (128, 64), (64, 128), (768, 768), (3072, 768), (768, 3072), (320, 4096), (1024, 1024))
GUARD, GUARD_BYTE = 256, 0xA5


def _lib():
    from bigcn_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _guarded(nbytes, fill=0):
    """A uint8 buffer of ``nbytes`` (16-byte aligned, filled with ``fill``) and GUARD guard bytes behind it."""
    t = torch.empty(nbytes + GUARD, dtype=torch.uint8, device=DEV)
    t[:nbytes] = fill
    t[nbytes:] = GUARD_BYTE
    return t


def _guards_ok(t, nbytes):
    return bool((t[nbytes:] == GUARD_BYTE).all())


def pack(W, ldw=None):
    """The image of W [Nc, K] (a guarded buffer and its size); ``ldw``: W is copied into rows of that stride."""
    L = _lib()
    Nc, K = W.shape
    if ldw is not None:
        wide = torch.full((Nc, ldw), float("nan"), device=DEV)
        wide[:, :K] = W
        W = wide[:, :K]
    else:
        W = W.contiguous()
    n = L.lib().bgcn_w16_image_size(Nc, K)
    assert n >= 2 * Nc * K
    img = _guarded(n)
    L.check(L.lib().bgcn_w16_pack(W.data_ptr(), W.stride(0), Nc, K, img.data_ptr(), _stream()))
    assert _guards_ok(img, n)
    return img, n


def gemm(X, img, Nc, K, bias=None, ldy=None, ws=None, Y=None):
    """Y [M, Nc] of bgcn_gemm_xwt_w16 on X [M, K] (any row stride that is a multiple of 4)."""
    L = _lib()
    M = X.size(0)
    need = L.lib().bgcn_gemm_xwt_w16_workspace_size(M, Nc, K)
    assert need > 0
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    if Y is None:
        Y = torch.full((M, ldy or Nc), float("nan"), device=DEV)[:, :Nc]
    L.check(L.lib().bgcn_gemm_xwt_w16(X.data_ptr(), X.stride(0), img.data_ptr(), 0 if bias is None else bias.data_ptr(),
                                      Y.data_ptr(), Y.stride(0), M, Nc, K, ws.data_ptr(), ws.numel(), _stream()))
    return Y


def exact_operands(M, Nc, K, seed):
    g = torch.Generator().manual_seed(seed)
    a, b, c = (torch.randint(-3, 4, (M, K), generator=g).double() for _ in range(3))
    X = (a + b * 2.0 ** -8 + c * 2.0 ** -16).float()
    W = torch.zeros(Nc, K)
    cols = torch.stack([torch.randperm(K, generator=g)[:16] for _ in range(Nc)])
    vals = torch.randint(-4, 5, (Nc, 16), generator=g).float()
    W.scatter_(1, cols, vals)
    want = X.double() @ W.double().t()
    assert torch.equal(want.float().double(), want)
    return X, W, want.float()


# ------------------------------------------------------------------ the pack kernel
def _planted(Nc, K, seed):
    """randn with ties, values one ulp (fp32) either side of a tie, +-0 and the largest bf16 planted."""
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(Nc, K, generator=g)
    bits = W.view(torch.int32).clone()
    flat = bits.view(-1)
    idx = torch.randperm(flat.numel(), generator=g)[:6 * 64].view(6, 64)
    flat[idx[0]] = (flat[idx[0]] & ~0xFFFF) | 0x8000            # tie: to even, down or up by the kept lsb
    flat[idx[1]] = (flat[idx[1]] & ~0xFFFF) | 0x7FFF            # one ulp below a tie
    flat[idx[2]] = (flat[idx[2]] & ~0xFFFF) | 0x8001            # one ulp above a tie
    flat[idx[3]] = torch.where(torch.arange(64) % 2 == 0, 0, -2 ** 31).int()   # +0, -0
    flat[idx[4]] = torch.where(torch.arange(64) % 2 == 0, 0x7F7F0000, 0x7F7F0000 - 2 ** 32).int()   # +-bf16 max
    flat[idx[5]] = 0x7F7F7FFF                                   # the largest fp32 that does not round to inf
    return bits.view(torch.float32)


@pytest.mark.parametrize("Nc,K", SHAPES)
def test_pack_is_torchs_rounding(Nc, K):
    W = _planted(Nc, K, Nc + K)
    want = W.bfloat16().float()                     # [Nc, K]; row k of Y is column k of the image
    assert bool(torch.isfinite(want).all())
    img, _ = pack(W.to(DEV), ldw=K + 12 if (Nc, K) == (768, 768) else None)
    eye = torch.eye(K, device=DEV)
    for r0 in range(0, K, 1024):                    # one-hot rows: Y[m, :] = the image's column r0 + m
        Y = gemm(eye[r0:r0 + 1024], img, Nc, K)
        assert torch.equal(Y.cpu(), want[:, r0:r0 + 1024].t()), (Nc, K, r0)


def test_pack_rounds_to_infinity_as_torch():
    W = torch.randn(64, 64, generator=torch.Generator().manual_seed(3))
    W[5, 7], W[9, 3] = float("inf"), float("-inf")
    W[11, 2] = torch.finfo(torch.float32).max       # above the last tie: rounds to inf
    W[13, 4] = torch.tensor(0x7F7F8000, dtype=torch.int32).view(torch.float32)   # the tie: to even, inf
    want = W.bfloat16().float()
    assert want[11, 2] == float("inf") and want[13, 4] == float("inf")
    img, n = pack(W.to(DEV))
    # an infinite weight cannot be read back through the product (the zero planes of x times inf are NaN
    # in its whole column), so the image itself is looked at, as a multiset: it is 2 Nc K bytes, a
    # permutation of torch's bf16 words
    assert n == 2 * 64 * 64
    words = img[:n].view(torch.int16).cpu().sort().values
    assert torch.equal(words, want.bfloat16().view(torch.int16).flatten().sort().values)
    Y = gemm(torch.eye(64, device=DEV), img, 64, 64).cpu()
    clean = [c for c in range(64) if c not in (5, 9, 11, 13)]
    assert torch.equal(Y[:, clean], want[clean].t())
    assert bool(torch.isnan(Y[:, [5, 9, 11, 13]]).any())


# ------------------------------------------------------------------ exact arithmetic
@pytest.mark.parametrize("M", [1, 24, 31, 32, 33, 64, 65, 130, 300])
def test_exact_product_every_row_count(M):
    X, W, want = exact_operands(M, 768, 768, M)
    img, _ = pack(W.to(DEV))
    assert torch.equal(gemm(X.to(DEV), img, 768, 768).cpu(), want)


@pytest.mark.parametrize("Nc,K", SHAPES)
def test_exact_product_every_shape(Nc, K):
    X, W, want = exact_operands(24, Nc, K, Nc * 7 + K)
    img, _ = pack(W.to(DEV))
    assert torch.equal(gemm(X.to(DEV), img, Nc, K).cpu(), want)


def test_exact_product_padded_rows_and_bias():
    M, Nc, K = 33, 128, 192
    X, W, want = exact_operands(M, Nc, K, 11)
    img, _ = pack(W.to(DEV))
    wide = torch.full((M, K + 8), float("nan"), device=DEV)
    wide[:, :K] = X.to(DEV)
    Ywide = torch.full((M, Nc + 4), 7.0, device=DEV)
    Y = gemm(wide[:, :K], img, Nc, K, Y=Ywide[:, :Nc])
    assert torch.equal(Y.cpu(), want)
    assert bool((Ywide[:, Nc:] == 7.0).all())       # the padding of Y's rows is not written
    bias = torch.randint(-8, 9, (Nc,), generator=torch.Generator().manual_seed(1)).float()
    Yb = gemm(X.to(DEV), img, Nc, K, bias=bias.to(DEV))
    assert torch.equal(Yb.cpu(), want + bias)


# ------------------------------------------------------------------ random data
@pytest.mark.parametrize("Nc,K", [(768, 768), (3072, 768), (768, 3072), (320, 4096)])
def test_random_product_within_the_derived_bound(Nc, K):
    g = torch.Generator().manual_seed(Nc + 3 * K)
    M = 33
    X, W = torch.randn(M, K, generator=g), torch.randn(Nc, K, generator=g) * 0.02
    bias = torch.randn(Nc, generator=g)
    img, _ = pack(W.to(DEV))
    got = gemm(X.to(DEV), img, Nc, K).cpu().double()
    w16 = W.bfloat16().double()
    want = X.double() @ w16.t()
    bound = (K + 4) * 2.0 ** -24 * (X.double().abs() @ w16.abs().t())
    worst = float(((got - want).abs() / bound).max())
    print(f"w16 gemm ({Nc}, {K}): worst error / bound = {worst:.4f}")
    assert bool(((got - want).abs() <= bound).all())
    # the bias is added last, in fp32
    gb = gemm(X.to(DEV), img, Nc, K, bias=bias.to(DEV)).cpu()
    assert torch.equal(gb, got.float() + bias)


# ------------------------------------------------------------------ row independence, determinism, buffers
def test_a_rows_bits_do_not_depend_on_the_other_rows():
    g = torch.Generator().manual_seed(5)
    Nc, K = 768, 768
    X, W = torch.randn(130, K, generator=g).to(DEV), (torch.randn(Nc, K, generator=g) * 0.02).to(DEV)
    img, _ = pack(W)
    Y = gemm(X, img, Nc, K)
    for m in (0, 31, 32, 127, 128, 129):
        assert torch.equal(gemm(X[m:m + 1], img, Nc, K), Y[m:m + 1]), m
    assert torch.equal(gemm(X[:64], img, Nc, K), Y[:64])


def test_deterministic_and_inside_its_buffers():
    L = _lib()
    g = torch.Generator().manual_seed(6)
    Nc, K = 768, 3072
    X, W = torch.randn(300, K, generator=g).to(DEV), (torch.randn(Nc, K, generator=g) * 0.02).to(DEV)
    img, nimg = pack(W)
    image_before = img.clone()
    need = L.lib().bgcn_gemm_xwt_w16_workspace_size(300, Nc, K)
    ws = _guarded(need, fill=0xFF)                   # NaN bits
    ybytes = 300 * Nc * 4
    ybuf = _guarded(ybytes, fill=0xFF)
    Y = ybuf[:ybytes].view(torch.float32).view(300, Nc)
    first = gemm(X, img, Nc, K, ws=ws[:need], Y=Y).clone()
    assert bool(torch.isfinite(first).all())
    ws[:need] = 0xFF
    again = gemm(X, img, Nc, K, ws=ws[:need], Y=Y)
    assert torch.equal(first, again)
    assert _guards_ok(ws, need) and _guards_ok(ybuf, ybytes) and torch.equal(img, image_before)
    # M = 1 straight after M = 300 on the same workspace
    one = gemm(X[7:8], img, Nc, K, ws=ws[:need])
    assert torch.equal(one, first[7:8]) and _guards_ok(ws, need)
    # a non-default stream
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        on_side = gemm(X, img, Nc, K)
    side.synchronize()
    assert torch.equal(on_side, first)


# ------------------------------------------------------------------ the model
_models = {}


def _m16(name):
    """A model of the case with the mode on (its own: bert_gpu_util._model(name) never has it on)."""
    if name not in _models:
        _models[name] = R.model_for(W16.case(name), DEV).use_weight_images("bf16")
    return _models[name]


_worst = {}


@pytest.mark.parametrize("name", W16.CASES)
def test_parity_with_the_rounded_weight_oracle(name):
    """logp and loss within BAR = 1e-4 of the fp64 oracle on the rounded weights; pred and correct equal."""
    c, o, m = W16.case(name), W16.oracle(name), _m16(name)
    x, root, y = _inputs(name)
    r = m._run(x, root, y=y, want_pred=True)
    m.check_status()
    e_logp = float((r["logp"].double().cpu() - o.logp).abs().max())
    e_loss = abs(float(r["loss"]) - o.loss)
    _worst[name] = {"logp": e_logp, "loss": e_loss}
    print(f"w16 parity {name}: logp {e_logp:.3e} loss {e_loss:.3e}")
    out = os.environ.get("BERT_W16_PARITY_OUT")        # profiles/bert_w16_parity.json is written this way
    if out and len(_worst) == len(W16.CASES):
        with open(out, "w") as f:
            json.dump({"bar": BAR, "oracle": "bert_ref.run in fp64 on the chain's GEMM weights rounded to bf16",
                       "worst_abs_error": _worst}, f, indent=1)
    assert e_logp <= BAR and e_loss <= BAR
    assert torch.equal(r["pred"].cpu(), o.pred) and int(r["correct"]) == o.correct
    # evaluate() on a PyG-like batch is the same call
    loss, correct, pred = m.evaluate(_data(name), pred=True)
    assert torch.equal(loss, r["loss"].view(())) and torch.equal(pred, r["pred"]) and int(correct) == o.correct


@pytest.mark.parametrize("name", ["boundaries", "offset_strided", "many_trees", "full_width", "rows_over_switch"])
def test_exact_invariances(name):
    c, m = W16.case(name), _m16(name)
    x, root, y = _inputs(name)
    logp = m.forward_batch(x, root)
    assert m._state["sizes"].get("w16") is not None      # the call went through bgcn_bert_eval_w16
    # evaluate twice
    d = _data(name)
    a, b = m.evaluate(d, pred=True), m.evaluate(d, pred=True)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    # a tree alone; forward(data) per tree, both versions
    starts = c.rootindex.tolist() + [c.N]
    picks = sorted({0, c.B // 2, c.B - 1})
    for b in picks:
        rows = x[starts[b]:starts[b + 1]]
        alone = m.forward_batch(rows.contiguous(), torch.zeros(1, dtype=torch.int64, device=DEV))
        assert torch.equal(alone, logp[b:b + 1]), b
        m.version = 0
        assert torch.equal(m.forward(rows.unsqueeze(1).contiguous()), logp[b:b + 1]), b
        m.version = 2
        try:       # n sequences of one token: each row is its own root
            got = m.forward(rows[:1].unsqueeze(1).contiguous())
        finally:
            m.version = 0
        assert torch.equal(got, logp[b:b + 1]), b
    # any permutation of the trees
    perm = torch.randperm(c.B, generator=torch.Generator().manual_seed(2))
    roots_x = x[root]                                  # [B, hidden]: one-row trees
    assert torch.equal(m.forward_batch(roots_x.contiguous(), torch.arange(c.B, device=DEV)), logp)
    px = roots_x[perm.to(DEV)].contiguous()
    assert torch.equal(m.forward_batch(px, torch.arange(c.B, device=DEV)), logp[perm.to(DEV)])
    m.check_status()


def test_the_modes_do_not_leak():
    name = "boundaries"
    m, plain = _m16(name), _model(name)
    assert plain.weight_images is None
    x, root, y = _inputs(name)
    d = _data(name)
    m.evaluate(d)                                      # images built
    e1, e2 = m.explain_batch(d), plain.explain_batch(d)
    for f in ("prediction", "log_probs", "hidden_sum", "attn_sum", "hidden_order", "attn_order"):
        assert torch.equal(getattr(e1, f), getattr(e2, f)), f
    h1, h2 = m.forward_batch(x, root, return_hidden=True), plain.forward_batch(x, root, return_hidden=True)
    assert torch.equal(h1[0], h2[0]) and torch.equal(h1[1], h2[1])
    g1, g2 = m.grad_batch(x, root, y, drop_seed=3), plain.grad_batch(x, root, y, drop_seed=3)
    assert torch.equal(g1[0], g2[0]) and all(torch.equal(g1[2][k], g2[2][k]) for k in g2[2])
    on = m.forward_batch(x, root)
    want = plain.forward_batch(x, root)
    assert not torch.equal(on, want)
    m.use_weight_images(None)
    try:
        assert m.weight_images is None and torch.equal(m.forward_batch(x, root), want)
        assert all(torch.equal(p, q) for p, q in zip(m.evaluate(d, pred=True), plain.evaluate(d, pred=True)))
    finally:
        m.use_weight_images("bf16")
    assert torch.equal(m.forward_batch(x, root), on)
    m.check_status()
    plain.check_status()


@pytest.mark.parametrize("how", ["in_place", "load_state_dict", "native_adam"])
def test_the_images_follow_the_parameters(how):
    name = "boundaries"
    c = W16.case(name)
    m = R.model_for(c, DEV).use_weight_images("bf16")
    d = _data(name)
    first = m.evaluate(d, pred=True)
    key = "BERT.encoder.layer.1.output.dense.weight"
    if how == "native_adam":
        from bigcn_amd import TreeBERTTrainStep
        step = TreeBERTTrainStep(m, lr=5e-3, drop_seed=1)
        step.step(d)
        step.check_status()
        sd = {k: v.clone() for k, v in m.state_dict().items()}
    else:
        sd = {k: v.clone() for k, v in c.sd.items()}
        sd[key] = sd[key] * 1.5
        if how == "in_place":
            with torch.no_grad():
                dict(m.named_parameters())[key].mul_(1.5)
        else:
            m.load_state_dict(sd, strict=True)
    second = m.evaluate(d, pred=True)
    fresh = R.model_for(c, DEV)
    fresh.load_state_dict(sd, strict=True)
    fresh.use_weight_images("bf16")
    want = fresh.evaluate(d, pred=True)
    assert all(torch.equal(p, q) for p, q in zip(second, want))
    assert not torch.equal(second[0], first[0])
    m.check_status()


@pytest.mark.parametrize("kind", ["roots_not_increasing", "label_out_of_range"])
def test_invalid_batches_are_flagged_and_stay_in_bounds(kind):
    L = _lib()
    name = "many_trees"
    c, m = W16.case(name), _m16(name)
    x, root, y = _inputs(name)
    good = m._run(x, root, y=y, want_pred=True)
    m.check_status()
    broot, by = root.clone(), y.clone()
    if kind == "roots_not_increasing":
        broot[5] = broot[4]
    else:
        by[7] = c.cfg["out"]
    m._state["ws"]["w16"].fill_(0xFF)                  # NaN bits
    r = m._run(x, broot, y=by, want_pred=True)
    with pytest.raises(IndexError):
        m.check_status()
    m.check_status()                                   # cleared
    assert bool(torch.isfinite(r["logp"]).all())
    if kind == "label_out_of_range":
        assert torch.equal(r["logp"], good["logp"]) and torch.equal(r["pred"], good["pred"])
    # the same call on a workspace and a logp of exactly the asked size, guard bytes behind both
    wa = m._w16["args"]
    need = L.lib().bgcn_bert_w16_workspace_size(c.B, c.cfg["hidden"], c.cfg["intermediate"], c.cfg["layers"])
    ws = _guarded(need, fill=0xFF)
    nlogp = c.B * c.cfg["out"] * 4
    logp = _guarded(nlogp, fill=0xFF)
    wa.base.logp = logp.data_ptr()
    L.check(L.lib().bgcn_bert_eval_w16(ctypes.addressof(wa), ws.data_ptr(), need, _stream()))
    torch.cuda.synchronize()
    assert _guards_ok(ws, need) and _guards_ok(logp, nlogp)
    assert torch.equal(logp[:nlogp].view(torch.float32).view(c.B, -1), r["logp"])
    # the next valid call has the first one's bits
    again = m._run(x, root, y=y, want_pred=True)
    m.check_status()
    assert all(torch.equal(again[k], good[k]) for k in ("logp", "loss", "correct", "pred"))
