"""Exactly representable operands for the dense GEMM kernels (bgcn_gemm.hip) and a CPU
restatement of their six-product bf16 arithmetic (split3_bf16 / mfma_x6 of bgcn_common.h).
TEST INFRASTRUCTURE: tests/test_gemm_ref.py checks the classes and the restatement on the CPU,
tests/test_gpu_gemm_exact.py compares the kernels with them bit for bit.

Every class builds fp32 operands A [M, K] and B [N, K] whose product Y = A B^T has an fp32
value in every element, so the fp64 result cast to fp32 is THE result: any summation order, any
split of K and any order of float atomics must give the same bits.

* INT       both operands integers in [-8, 8]: every product and partial sum is an integer of
            magnitude <= 64 K < 2^24.
* ONEHOT-A  every row of one operand has a single nonzero +-2^e (e in [-6, 6]) at a column that
            walks down from the last one with the row; the other operand is full-mantissa randn.
            Each output is one product by a power of two.  The dense operand has nonzero hi, mid
            and lo bf16 planes, the one-hot operand only hi: with the one-hot operand on the left
            the result needs ah.bl, ah.bm, ah.bh, on the right al.bh, am.bh, ah.bh.
* ONEHOT-C  the one-hot value is (1 +- 2^-9) 2^e (hi and mid planes nonzero, lo zero) and the
            dense operand is rounded to 15 significant bits (hi and mid nonzero, lo zero), so
            am.bm carries the product's last bits.  A 10-bit by 15-bit product has 24 or 25
            bits; the elements whose fp64 product is not an fp32 number (a carry into the 25th
            bit, about 0.1 %) are left out of the comparison (`keep`).
"""
import torch

INT_MAX_ABS = 8
# the largest K any GPU case uses (the carry-over conv1 shape of tests/test_gpu_kernels.py)
K_MAX = 5000
# mfma_x6's products in the order bgcn_common.h issues them: (plane of a, plane of b),
# planes 0 = hi, 1 = mid, 2 = lo
X6_ORDER = ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0))
X6_NAMES = ("al.bh", "am.bm", "ah.bl", "am.bh", "ah.bm", "ah.bh")
CLASSES = ("int", "onehot_a", "onehot_c")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def int_matrix(rows, cols, seed):
    return torch.randint(-INT_MAX_ABS, INT_MAX_ABS + 1, (rows, cols), generator=_gen(seed)).float()


def onehot_matrix(rows, cols, seed, mid_plane=False):
    """One nonzero per row at column (cols - 1 - row) mod cols: +-2^e, times (1 +- 2^-9) for
    `mid_plane`."""
    g = _gen(seed)
    e = torch.randint(-6, 7, (rows,), generator=g)
    v = torch.ldexp(torch.ones(rows, dtype=torch.float64), e)
    v = v * (torch.randint(0, 2, (rows,), generator=g) * 2 - 1)
    if mid_plane:
        v = v * (1.0 + (torch.randint(0, 2, (rows,), generator=g) * 2 - 1) * 2.0 ** -9)
    out = torch.zeros(rows, cols, dtype=torch.float32)
    if rows:
        r = torch.arange(rows)
        out[r, (cols - 1 - r) % cols] = v.float()
    return out


def dense_matrix(rows, cols, seed, bits=24):
    """randn in fp32, rounded (half away from zero) to `bits` significant bits."""
    x = torch.randn(rows, cols, generator=_gen(seed), dtype=torch.float32)
    if bits < 24:
        drop = 24 - bits
        i = x.view(torch.int32)
        i = (i + (1 << (drop - 1))) & ~((1 << drop) - 1)
        x = i.view(torch.float32)
    return x


def operands(cls, onehot_left, M, N, K, seed=0):
    """A [M, K], B [N, K] of class `cls`; the one-hot operand is A for `onehot_left`, else B
    (ignored for "int")."""
    if cls == "int":
        return int_matrix(M, K, seed), int_matrix(N, K, seed + 1)
    mid = cls == "onehot_c"
    bits = 15 if mid else 24
    if onehot_left:
        return onehot_matrix(M, K, seed, mid), dense_matrix(N, K, seed + 1, bits)
    return dense_matrix(M, K, seed, bits), onehot_matrix(N, K, seed + 1, mid)


def expected(A, B, chunk=2048):
    """(Y, keep): Y = fp32(A B^T in fp64) and the mask of the elements where that cast is exact
    (all of them for INT and ONEHOT-A)."""
    Bd = B.double().t().contiguous()
    Y = torch.empty(A.size(0), B.size(0), dtype=torch.float32)
    keep = torch.empty(A.size(0), B.size(0), dtype=torch.bool)
    for r in range(0, A.size(0), chunk):
        y64 = A[r:r + chunk].double() @ Bd
        Y[r:r + chunk] = y64.float()
        keep[r:r + chunk] = Y[r:r + chunk].double() == y64
    return Y, keep


def masked(Y, keep):
    """Y with the left-out elements replaced by 0 (apply to both sides of a comparison)."""
    return torch.where(keep, Y, torch.zeros((), dtype=Y.dtype, device=Y.device))


# ------------------------------------------------------------------ the six-product restatement
def split3_bf16(x):
    """bgcn_common.h split3_bf16: hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid),
    round to nearest even, as fp32 tensors."""
    hi = x.bfloat16().float()
    r = x - hi
    mid = r.bfloat16().float()
    lo = (r - mid).bfloat16().float()
    return hi, mid, lo


def mfma_x6(A, B, drop=None):
    """A B^T as mfma_x6 accumulates it: the six plane products added to an fp32 accumulator in
    X6_ORDER (product `drop` left out).  Each plane product is formed in fp64 - exact for these
    classes, where it has one nonzero term (one-hot) or integer terms (INT)."""
    a, b = split3_bf16(A), split3_bf16(B)
    acc = torch.zeros(A.size(0), B.size(0), dtype=torch.float32)
    for i, (pa, pb) in enumerate(X6_ORDER):
        if i == drop:
            continue
        acc = (acc.double() + a[pa].double() @ b[pb].double().t()).float()
    return acc
