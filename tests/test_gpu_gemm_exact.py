"""Bit-exact tests of the dense-path kernels (bgcn_gemm.hip, bgcn_scatter.hip) through the C ABI.

The operands come from tests/gemm_ref.py: every product and every partial sum has an fp32 value,
so the kernels must return the fp64 result cast to fp32 bit for bit (torch.equal), whatever the
summation order, the split of K or the order of the float atomics.  tests/test_gemm_ref.py shows
on the CPU that a six-product kernel which leaves out any one product fails this comparison.

Every operand lives inside a larger allocation: the columns from its width to its leading
dimension and a guard region after its last row hold NaN (a load that reaches the result shows),
the padding of every output holds a sentinel that must survive.

Kernel each case enters (gemm_xwt_t / gemm_xw_impl / gemm_tn_t, fp32 X, default knobs):
* test_xwt_six_product*, test_xwt_k5000: k_gemm_xwt_x6p (M >= 8192, K, ldx, ldw % 4 == 0, 16-byte
  bases, Nc % 128 == 0, split % 64 == 0);
* test_xwt_off_the_six_product_path: X base + 4 bytes or ldx = K + 1 -> k_gemm_xwt<VEC=false>;
  Nc = 192 or split = 32 -> k_gemm_xwt<VEC=true>;
* test_xwt_f32_mfma: K in {32, 36}, ld tight or a multiple of 4, aligned -> k_gemm_xwt<true,
  BKM=false>; everything else (K % 4 != 0, odd ld, X or W0 base + 4 bytes) -> <false, false>;
* test_xw: (64, 128, 32) and (130, 20, 36) with ld tight or a multiple of 4 and aligned bases
  -> k_gemm_xwt<true, BKM=true>; everything else (Nc % 4 != 0, K % 4 != 0, odd ld, X or W base
  + 4 bytes) -> <false, true>;
* test_tn: Mc, Nc, ldg, ldx % 4 == 0 and aligned -> k_gemm_tn_w (shapes (128, 64), (64, 132),
  (132, 260), (4, 4) with ld tight or a multiple of 4); (20, 30), odd ld and G base + 4 bytes ->
  k_gemm_tn<VEC=false>; k_reduce_splits always, over 1 (K <= 32), 4 (K = 100) or up to 16
  (K = 512) node splits;
* test_colsum: k_colsum_part + k_colsum_final, rows = 0: the memset;
* test_scatter_mean: sorted index -> k_seg_bounds + k_seg_mean, unsorted -> k_atomic_zero /
  _sum / _div; k_check and k_mean_bwd always.
"""
import numpy as np
import pytest
import torch

import gemm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
SENT = -777.25          # no integer and (almost surely) no product of the classes
GUARD = 1024            # floats after the last row: the x6p ring prefetches 3 k-tiles (192 floats)

CASES = [("int", True), ("onehot_a", True), ("onehot_a", False), ("onehot_c", True), ("onehot_c", False)]
CASE_IDS = ["int", "onehot_a-x", "onehot_a-w", "onehot_c-x", "onehot_c-w"]
# the classes of the f32 MFMA kernels: INT, and ONEHOT-A (one exact product per output)
CASES_F32 = CASES[:3]


def _api():
    from bigcn_amd import _lib
    return _lib.lib(), _lib.check, _lib.stream_handle()


def _ws(nbytes):
    """A workspace of all-ones bytes (fp32 NaN): nothing may be read before it is written."""
    return torch.full((max(int(nbytes), 16),), 255, dtype=torch.uint8, device=DEV)


class Dev:
    """A [rows, width] fp32 matrix with row stride `ld` inside one device allocation of
    lead + rows * ld + guard + 4 floats; everything outside the matrix holds `fill`."""

    def __init__(self, rows, width, ld=None, lead=0, guard=0, fill=NAN, data=None):
        self.rows, self.width, self.ld, self.lead = rows, width, ld or width, lead
        assert self.ld >= width
        self.fill = fill
        self.buf = torch.full((lead + rows * self.ld + guard + 4,), fill, device=DEV)
        if data is not None and rows:
            assert tuple(data.shape) == (rows, width)
            self.view(self.buf).copy_(data)

    def view(self, buf):
        return buf[self.lead:self.lead + self.rows * self.ld].view(self.rows, self.ld)[:, :self.width]

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * self.lead

    def check(self, want, keep=None, what=""):
        """The matrix equals `want` bit for bit (on `keep`) and the rest of the allocation is
        untouched."""
        got = self.buf.cpu()
        exp = torch.full_like(got, self.fill)
        if self.rows:
            g, e = self.view(got), self.view(exp)
            if keep is not None:
                g.copy_(R.masked(g, keep))
                want = R.masked(want, keep)
            e.copy_(want)
            bad = int((g != e).sum())
        else:
            bad = 0
        assert torch.equal(got, exp), (f"{what}: {bad} of {self.rows * self.width} elements differ, "
                                       f"{int((got != exp).sum()) - bad} outside the matrix")


def ld_of(width, mode):
    if mode == "tight":
        return width
    if mode == "pad4":
        return (width + 3) // 4 * 4 + 4
    return width + 1 + width % 2          # "odd"


# ---------------------------------------------------------------------------- bgcn_gemm_xwt
def run_xwt(x, B, split, M=None, ldw=None, ldy=None, w_lead=0, guard=0):
    """Y [M, Nc] = X . B^T with B's rows [0, split) in one allocation and the rest in another."""
    L, check, stream = _api()
    Nc, K = B.shape
    M = x.rows if M is None else M
    w0 = Dev(split, K, ldw, w_lead, guard, data=B[:split])
    w1 = Dev(Nc - split, K, ldw, 0, guard, data=B[split:]) if split < Nc else None
    y = Dev(M if M else 3, Nc, ldy, fill=SENT)      # (no rows: room for a stray write to show)
    check(L.bgcn_gemm_xwt(x.ptr, x.ld, w0.ptr, w1.ptr if w1 else 0, w0.ld, split, y.ptr, y.ld, M, Nc, K, stream))
    return y


X6_M = 8229             # 64 full 128-row tiles and a partial one
X6_LAYOUTS = ((128, 64), (128, 128), (256, 64), (256, 128), (256, 192))     # (Nc, split)


@pytest.mark.parametrize("cls,left", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("K", [4, 60, 64, 68, 192, 200, 320])     # 1, 1, 1, 2, 3, 4, 5 k-tiles of 64
def test_xwt_six_product(K, cls, left):
    A, B = R.operands(cls, left, X6_M, 256, K, seed=K)
    Y, keep = R.expected(A, B)
    assert float(keep.float().mean()) >= 0.99
    x = Dev(X6_M, K, guard=GUARD, data=A)
    for Nc, split in X6_LAYOUTS:
        y = run_xwt(x, B[:Nc], split, guard=GUARD)
        y.check(Y[:, :Nc], keep[:, :Nc], f"Nc {Nc} split {split}")


@pytest.mark.parametrize("cls,left", CASES, ids=CASE_IDS)
def test_xwt_six_product_padded_ld(cls, left):
    K, Nc, split = 200, 256, 64
    A, B = R.operands(cls, left, X6_M, Nc, K, seed=1)
    Y, keep = R.expected(A, B)
    x = Dev(X6_M, K, ld=K + 4, guard=GUARD, data=A)
    run_xwt(x, B, split, ldw=K + 8, ldy=Nc + 4, guard=GUARD).check(Y, keep)


def test_xwt_k5000():
    """The conv1 shape of test_gpu_kernels.test_gemm_xwt: 79 k-tiles."""
    M, Nc, K = 8300, 128, R.K_MAX
    A, B = R.operands("int", True, M, Nc, K, seed=2)
    Y, keep = R.expected(A, B, chunk=1024)
    assert bool(keep.all())
    run_xwt(Dev(M, K, guard=GUARD, data=A), B, 64, guard=GUARD).check(Y)


@pytest.mark.parametrize("how", ["x_offset", "ldx_odd", "nc192", "split32"])
def test_xwt_off_the_six_product_path(how):
    K = 200
    Nc = 192 if how == "nc192" else 128
    A, B = R.operands("int", True, X6_M, Nc, K, seed=3)
    Y, _ = R.expected(A, B)
    x = Dev(X6_M, K, ld=K + 1 if how == "ldx_odd" else K, lead=1 if how == "x_offset" else 0, data=A)
    run_xwt(x, B, 32 if how == "split32" else 64).check(Y)


SMALL = [(1, 1, 1), (63, 127, 31), (64, 128, 32), (65, 129, 33), (130, 20, 36)]     # (M, Nc, K)


@pytest.mark.parametrize("M,Nc,K", SMALL)
def test_xwt_f32_mfma(M, Nc, K):
    for cls, left in CASES_F32:
        A, B = R.operands(cls, left, M, Nc, K, seed=M)
        Y, _ = R.expected(A, B)
        for mode in ("tight", "pad4", "odd"):
            for x_lead, w_lead in ((0, 0), (1, 0), (0, 1)):
                x = Dev(M, K, ld_of(K, mode), x_lead, data=A)
                for split in sorted({0, Nc // 2, Nc}):
                    y = run_xwt(x, B, split, ldw=ld_of(K, mode), ldy=ld_of(Nc, mode), w_lead=w_lead)
                    y.check(Y, None, f"{cls} {mode} leads {x_lead} {w_lead} split {split}")


def test_xwt_no_rows_writes_nothing():
    A, B = R.operands("int", True, 0, 128, 64)
    y = run_xwt(Dev(0, 64, data=A), B, 64, M=0)
    assert bool((y.buf == SENT).all())


# ----------------------------------------------------------------------------- bgcn_gemm_xw
@pytest.mark.parametrize("M,Nc,K", SMALL)
def test_xw(M, Nc, K):
    L, check, stream = _api()
    for cls, left in CASES_F32:
        A, B = R.operands(cls, left, M, Nc, K, seed=K)
        Y, _ = R.expected(A, B)
        W = B.t().contiguous()                                    # [K, Nc]
        for mode, x_lead, w_lead in (("tight", 0, 0), ("pad4", 0, 0), ("odd", 0, 0), ("tight", 1, 0),
                                     ("tight", 0, 1), ("pad4", 0, 1)):
            x = Dev(M, K, ld_of(K, mode), x_lead, data=A)
            w = Dev(K, Nc, ld_of(Nc, mode), w_lead, data=W)
            y = Dev(M, Nc, ld_of(Nc, mode), fill=SENT)
            check(L.bgcn_gemm_xw(x.ptr, x.ld, w.ptr, w.ld, y.ptr, y.ld, M, Nc, K, stream))
            y.check(Y, None, f"{cls} {mode} leads {x_lead} {w_lead}")


# ----------------------------------------------------------------------------- bgcn_gemm_tn
def run_tn(A, B, split, mode="tight", g_lead=0, what=""):
    """C [Mc, Nc] = G^T X for G = A^T [K, Mc], X = B^T [K, Nc]; rows [0, split) -> C0, rest -> C1."""
    L, check, stream = _api()
    (Mc, K), Nc = A.shape, B.size(0)
    Y, keep = R.expected(A, B)
    assert bool(keep.all())
    g = Dev(K, Mc, ld_of(Mc, mode), g_lead, data=A.t())
    x = Dev(K, Nc, ld_of(Nc, mode), data=B.t())
    c0 = Dev(split, Nc, ld_of(Nc, mode), fill=SENT)
    c1 = Dev(Mc - split, Nc, ld_of(Nc, mode), fill=SENT) if split < Mc else None
    ws = _ws(L.bgcn_gemm_tn_workspace_size(Mc, Nc, K))
    check(L.bgcn_gemm_tn(g.ptr, g.ld, x.ptr, x.ld, c0.ptr, c1.ptr if c1 else 0, c0.ld, split, Mc, Nc, K,
                         ws.data_ptr(), ws.numel(), stream))
    c0.check(Y[:split], None, what + " C0")
    if c1:
        c1.check(Y[split:], None, what + " C1")


TN_SHAPES = [(128, 64), (64, 132), (132, 260), (20, 30), (4, 4)]      # (Mc, Nc)


@pytest.mark.parametrize("K", [0, 1, 15, 16, 17, 31, 32, 33, 100, 512])
def test_tn(K):
    for Mc, Nc in TN_SHAPES:
        A, B = R.operands("int", True, Mc, Nc, K, seed=K + Mc)
        for split in sorted({Mc, Mc // 2, 4}):
            for mode in ("tight", "pad4", "odd"):
                run_tn(A, B, split, mode, what=f"int {Mc}x{Nc} split {split} {mode}")     # K == 0: zeros
        if K:
            for left in (True, False):
                A, B = R.operands("onehot_a", left, Mc, Nc, K, seed=K + Mc)
                run_tn(A, B, Mc // 2, what=f"onehot_a {left} {Mc}x{Nc}")


def test_tn_g_offset():
    A, B = R.operands("int", True, 128, 64, 100, seed=4)
    run_tn(A, B, 64, g_lead=1)


# ------------------------------------------------------------------------------ bgcn_colsum
@pytest.mark.parametrize("C", [1, 70, 256, 257, 300])
def test_colsum(C):
    L, check, stream = _api()
    for rows in (0, 1, 255, 256, 257, 513):
        A = R.int_matrix(rows, C, seed=rows + C)
        want = A.double().sum(0).float()[None]
        for lda in (C, C + 3):
            a = Dev(rows, C, lda, data=A)
            out = Dev(1, C, fill=SENT)
            ws = _ws(L.bgcn_colsum_workspace_size(rows, C))
            check(L.bgcn_colsum(a.ptr, lda, rows, C, out.ptr, ws.data_ptr(), ws.numel(), stream))
            out.check(want, None, f"rows {rows} lda {lda}")


# ------------------------------------------------------------------------- bgcn_scatter_mean
def scatter_index(n, B, sorted_index, oob, seed):
    """n segment ids with the first, middle and last segment empty (B >= 3); `oob` puts ids
    below 0 and >= B among them."""
    rng = np.random.default_rng(seed)
    live = [b for b in range(B) if B < 3 or b not in (0, B // 2, B - 1)]
    idx = rng.choice(live, n).astype(np.int64)
    if oob and n:
        idx[rng.choice(n, 8, replace=False)] = [-3, -1, B, B + 2, -1, B, -(2 ** 40), 2 ** 40]
    idx = np.sort(idx) if sorted_index else rng.permutation(idx)
    return idx


def scatter_expected(src, idx, B):
    """torch_scatter's mean: fp32(sum) / fp32(max(count, 1)), ids outside [0, B) left out."""
    ok = (idx >= 0) & (idx < B)
    sums = np.zeros((B, src.shape[1]), np.float64)
    np.add.at(sums, idx[ok], src[ok].astype(np.float64))
    count = np.maximum(np.bincount(idx[ok], minlength=B), 1).astype(np.float32)
    return sums.astype(np.float32) / count[:, None], count, ok


@pytest.mark.parametrize("B", [1, 5, 40])
@pytest.mark.parametrize("C", [1, 63, 64, 65, 130])
def test_scatter_mean(C, B):
    L, check, stream = _api()
    for n in (0, 301):
        src = R.int_matrix(n, C, seed=C + B)
        dout = R.dense_matrix(B, C, seed=C)
        for sorted_index in (True, False):
            for oob in (False, True):
                idx = scatter_index(n, B, sorted_index, oob, seed=B)
                is_sorted = bool((np.diff(idx) >= 0).all())
                if n and is_sorted != sorted_index:
                    assert B == 1 and not oob          # one segment: no unsorted order exists
                    continue
                want, count, ok = scatter_expected(src.numpy(), idx, B)
                if n == 0:
                    assert not want.any() and (count == 1).all()
                what = f"n {n} sorted {sorted_index} oob {oob}"
                for pad in (3, 0):
                    s = Dev(n, C, C + pad, data=src)
                    index = torch.from_numpy(idx).to(DEV)
                    out = Dev(B, C, C + pad, fill=SENT)
                    cnt = Dev(1, B, fill=SENT)
                    status = torch.zeros(1, dtype=torch.int32, device=DEV)
                    ws = _ws(L.bgcn_scatter_mean_workspace_size(B))
                    check(L.bgcn_scatter_mean_fwd(s.ptr if n else 0, s.ld, index.data_ptr() if n else 0, n, C, B,
                                                  out.ptr, out.ld, cnt.ptr, status.data_ptr(), ws.data_ptr(),
                                                  ws.numel(), stream))
                    out.check(torch.from_numpy(want), None, what + " fwd")
                    cnt.check(torch.from_numpy(count)[None], None, what + " count")
                    assert int(status) & 1 == int(oob and n > 0), what
                    # backward: dsrc[i] = dout[index[i]] / count[index[i]], zero rows outside [0, B)
                    d = Dev(B, C, C + pad, data=dout)
                    dsrc = Dev(n, C, C + pad, fill=SENT)
                    check(L.bgcn_scatter_mean_bwd(d.ptr, d.ld, index.data_ptr() if n else 0, cnt.ptr, n, C, B,
                                                  dsrc.ptr, dsrc.ld, stream))
                    safe = np.where(ok, idx, 0)
                    wd = np.where(ok[:, None], dout.numpy()[safe] / count[safe][:, None], np.float32(0))
                    dsrc.check(torch.from_numpy(wd.astype(np.float32)), None, what + " bwd")
