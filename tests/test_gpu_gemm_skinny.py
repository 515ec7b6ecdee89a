"""GPU checks of the skinny fp32 GEMMs alone (bgcn_gemm_skinny.hip through bigcn_amd.ops):
``xwt`` Y = X W^T (+ bias), ``xw`` Y = G W and ``tn`` dW = G^T X for a weight W [Nc, K] and M rows.

* exact: integer operands (tests/gemm_ref.py, class "int") - every partial sum is an fp32 number in any
  order, so all three products equal ``gemm_ref.expected`` bit for bit;
* dense: ``gemm_ref.dense_matrix`` operands against fp64 within the bound of an fp32 dot product of length
  R summed in S + 1 stages, ``(R + S) 2^-24 (|A| . |B|)`` element-wise (S = 1 for ``tn``, which has no split);
* a row's bits do not depend on the rows beside it; nothing depends on what the workspace and the output
  held; refused calls write nothing.

With BGCN_GEMM_SKINNY_OUT set the dense test's worst ratios to the bound go to that path
(profiles/bert_train_skinny.json holds such a record)."""
import functools
import json
import os

import pytest
import torch

import gemm_ref as G

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
# (M, Nc, K): one tile with S = 1; the workload's three; a second row block of one row; Nc % 128 != 0 with
# the longest reduction and a row tile of one row past 32; three row blocks
SHAPES = [(1, 64, 64), (24, 768, 768), (24, 3072, 768), (24, 768, 3072), (129, 64, 128), (33, 320, 4096), (300, 128, 64)]
PAD = 8
_ratios = {}


def splits(red, width):
    """The split rule: the largest of 8, 4, 2 64-blocks per wave that divides the reduction and still leaves
    (width / 32) S >= 256 workgroups, else 1; S = red / 64 / that."""
    for kw in (8, 4, 2):
        if (red // 64) % kw == 0 and (width // 32) * (red // 64 // kw) >= 256:
            return red // 64 // kw
    return red // 64


def test_the_split_is_the_documented_one():
    from bigcn_amd import _lib
    assert [splits(K, Nc) for Nc, K in ((768, 768), (3072, 768), (768, 3072))] == [12, 3, 12]      # xwt
    assert [splits(Nc, K) for Nc, K in ((768, 768), (3072, 768), (768, 3072))] == [12, 12, 3]      # xw
    for M, Nc, K in SHAPES:
        want = 4 * M * max(splits(K, Nc) * Nc, splits(Nc, K) * K)
        assert _lib.lib().bgcn_gemm_skinny_workspace_size(M, Nc, K) == (want + 255) // 256 * 256


def _strided(t, pad):
    """``t`` on the device with a row stride of width + pad."""
    if not pad:
        return t.to(DEV)
    wide = torch.full((t.size(0), t.size(1) + pad), float("nan"), device=DEV)
    wide[:, :t.size(1)] = t.to(DEV)
    return wide[:, :t.size(1)]


@functools.lru_cache(maxsize=None)
def _operands(kind, M, Nc, K):
    """X [M, K], W [Nc, K], G [M, Nc] and the fp64 products (as fp32 for "int": exact)."""
    seed = 7000 + M + Nc + K
    if kind == "int":
        X, W = G.operands("int", False, M, Nc, K, seed)
        Gm = G.int_matrix(M, Nc, seed + 2)
    else:
        X, W, Gm = G.dense_matrix(M, K, seed), G.dense_matrix(Nc, K, seed + 1), G.dense_matrix(M, Nc, seed + 2)
    pairs = {"xwt": (X, W), "xw": (Gm, W.t().contiguous()), "tn": (Gm.t().contiguous(), X.t().contiguous())}
    if kind == "int":
        ref = {}
        for k, (A, B) in pairs.items():
            ref[k], keep = G.expected(A, B)
            assert bool(keep.all())
    else:
        ref = {k: (A.double() @ B.double().t(), A.double().abs() @ B.double().abs().t()) for k, (A, B) in pairs.items()}
    return X, W, Gm, ref


def _run(X, W, Gm, pad):
    from bigcn_amd import ops
    M, K, Nc = X.size(0), X.size(1), W.size(0)
    x, w, g = _strided(X, pad), _strided(W, pad), _strided(Gm, pad)
    outs = {k: _strided(torch.zeros(*shape), pad) for k, shape in (("xwt", (M, Nc)), ("xw", (M, K)), ("tn", (Nc, K)))}
    assert ops.gemm_xwt_skinny(x, w, out=outs["xwt"]) is outs["xwt"]
    ops.gemm_xw_skinny(g, w, out=outs["xw"])
    ops.gemm_tn_skinny(g, x, out=outs["tn"])
    if pad:
        for o in outs.values():
            assert o.stride(0) == o.size(1) + pad and bool(torch.isnan(o._base[:, o.size(1):]).all())   # padding untouched
    return {k: v.cpu() for k, v in outs.items()}


@pytest.mark.parametrize("pad", [0, PAD])
@pytest.mark.parametrize("M,Nc,K", SHAPES)
def test_integer_operands_give_exact_products(M, Nc, K, pad):
    X, W, Gm, ref = _operands("int", M, Nc, K)
    got = _run(X, W, Gm, pad)
    for k in ("xwt", "xw", "tn"):
        assert torch.equal(got[k], ref[k]), k


@pytest.mark.parametrize("pad", [0, PAD])
@pytest.mark.parametrize("M,Nc,K", SHAPES)
def test_dense_operands_are_within_the_fp32_dot_product_bound(M, Nc, K, pad):
    X, W, Gm, ref = _operands("dense", M, Nc, K)
    got = _run(X, W, Gm, pad)
    stages = {"xwt": (K, splits(K, Nc)), "xw": (Nc, splits(Nc, K)), "tn": (M, 1)}
    worst = {}
    for k, (R, S) in stages.items():
        y64, mag = ref[k]
        bound = (R + S) * 2.0 ** -24 * mag
        worst[k] = float(((got[k].double() - y64).abs() / bound).max())
    print(M, Nc, K, pad, worst)
    _ratios[f"{M}x{Nc}x{K}/ld+{pad}"] = worst
    out = os.environ.get("BGCN_GEMM_SKINNY_OUT")
    if out:
        with open(out, "w") as f:
            json.dump({"bound": "(R + S) 2^-24 (|A| . |B|)", "worst_ratio_to_bound": _ratios}, f, indent=1, sort_keys=True)
    for k, v in worst.items():
        assert v <= 1.0, (k, v)


def test_the_bias_is_added_after_the_partials():
    from bigcn_amd import ops
    M, Nc, K = 24, 768, 3072
    X, W, _, ref = _operands("int", M, Nc, K)
    bias = G.int_matrix(1, Nc, 99).view(-1)
    got = ops.gemm_xwt_skinny(X.to(DEV), W.to(DEV), bias.to(DEV))
    assert torch.equal(got.cpu(), ref["xwt"] + bias)


@pytest.mark.parametrize("M,Nc,K,rows", [(24, 768, 3072, (0, 11, 23)), (24, 3072, 768, (0, 23)),
                                         (300, 320, 4096, (0, 31, 32, 127, 128, 299))])
def test_a_row_has_the_bits_of_the_same_row_computed_alone(M, Nc, K, rows):
    from bigcn_amd import ops
    x = G.dense_matrix(M, K, 41).to(DEV)
    g = G.dense_matrix(M, Nc, 42).to(DEV)
    w = G.dense_matrix(Nc, K, 43).to(DEV)
    y, d = ops.gemm_xwt_skinny(x, w), ops.gemm_xw_skinny(g, w)
    for r in rows:
        assert torch.equal(ops.gemm_xwt_skinny(x[r:r + 1], w)[0], y[r]), r
        assert torch.equal(ops.gemm_xw_skinny(g[r:r + 1], w)[0], d[r]), r


def _capi(x, w, g, fill, M, Nc, K, ws_short=0, ld=None):
    """The three entries on a workspace and outputs pre-filled with ``fill``; (codes, outputs)."""
    from bigcn_amd import _lib
    L = _lib.lib()
    need = L.bgcn_gemm_skinny_workspace_size(M, Nc, K)
    ws = torch.full((max(need, 16) // 4,), fill, device=DEV)
    ld = {**dict(x=x.stride(0), w=w.stride(0), g=g.stride(0), y=Nc, d=K, dw=K), **(ld or {})}
    y, d, dw = (torch.full(s, fill, device=DEV) for s in ((M, Nc), (M, K), (Nc, K)))
    s = _lib.stream_handle()
    rc = (L.bgcn_gemm_xwt_skinny(x.data_ptr(), ld["x"], w.data_ptr(), ld["w"], 0, y.data_ptr(), ld["y"], M, Nc, K,
                                 ws.data_ptr(), need - ws_short, s),
          L.bgcn_gemm_xw_skinny(g.data_ptr(), ld["g"], w.data_ptr(), ld["w"], d.data_ptr(), ld["d"], M, Nc, K,
                                ws.data_ptr(), need - ws_short, s),
          L.bgcn_gemm_tn_skinny(g.data_ptr(), ld["g"], x.data_ptr(), ld["x"], dw.data_ptr(), ld["dw"], M, Nc, K, s))
    torch.cuda.synchronize()
    return rc, (y.cpu(), d.cpu(), dw.cpu())


@pytest.mark.parametrize("M,Nc,K", [(24, 768, 3072), (129, 64, 128)])
def test_results_do_not_depend_on_what_the_workspace_and_the_output_held(M, Nc, K):
    X, W, Gm, _ = _operands("dense", M, Nc, K)
    x, w, g = X.to(DEV), W.to(DEV), Gm.to(DEV)
    rc0, zero = _capi(x, w, g, 0.0, M, Nc, K)
    rc1, nan = _capi(x, w, g, float("nan"), M, Nc, K)
    rc2, again = _capi(x, w, g, float("nan"), M, Nc, K)
    assert rc0 == rc1 == rc2 == (0, 0, 0)
    for a, b, c in zip(zero, nan, again):
        assert bool(torch.isfinite(b).all())
        assert torch.equal(a, b) and torch.equal(b, c)


@pytest.mark.parametrize("what,M,Nc,K,kw", [
    ("Nc = 96", 8, 96, 128, {}), ("K = 32", 8, 128, 32, {}), ("K = 4160", 8, 64, 4160, {}),
    ("a short workspace", 8, 128, 128, dict(ws_short=256)),
    ("ld below the width", 8, 128, 128, dict(ld=dict(x=124, w=124, g=124))),
])
def test_a_refused_call_leaves_the_output_untouched(what, M, Nc, K, kw):
    from bigcn_amd import _lib, ops
    x, w, g = (torch.ones(s, device=DEV) for s in ((M, K), (Nc, K), (M, Nc)))
    rc, outs = _capi(x, w, g, 5.0, M, Nc, K, **kw)
    # the product that takes no workspace is not refused for a short one
    assert rc == ((-1, -1, 0) if "ws_short" in kw else (-1, -1, -1)), what
    for o, code in zip(outs, rc):
        if code:
            assert bool((o == 5.0).all()), what
    if not kw:
        with pytest.raises(_lib.BGCNError, match="unsupported shape"):
            ops.gemm_xwt_skinny(x, w)
        with pytest.raises(_lib.BGCNError, match="unsupported shape"):
            ops.gemm_tn_skinny(g, x)
