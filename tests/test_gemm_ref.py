"""CPU self-check of tests/gemm_ref.py: the operand classes of tests/test_gpu_gemm_exact.py are
exactly representable, the restatement of split3_bf16 / mfma_x6 reproduces them bit for bit, and
leaving out any single one of the six products is visible in most elements of some class - so the
GPU comparison (torch.equal) fails for a kernel that drops or misplaces a product."""
import pytest
import torch

import gemm_ref as R

M, N, K = 517, 128, 200     # A [M, K], B [N, K]: more rows than columns, so every column is hit
CASES = [("int", True), ("onehot_a", True), ("onehot_a", False), ("onehot_c", True), ("onehot_c", False)]


@pytest.fixture(scope="module")
def built():
    out = {}
    for cls, left in CASES:
        A, B = R.operands(cls, left, M, N, K, seed=11)
        out[cls, left] = (A, B) + R.expected(A, B)
    return out


def test_split3_is_exact_and_planes_are_as_described():
    x = R.dense_matrix(64, 64, 3)
    hi, mid, lo = R.split3_bf16(x)
    assert torch.equal(hi.double() + mid.double() + lo.double(), x.double())
    assert float((lo != 0).float().mean()) > 0.9
    for p in R.split3_bf16(R.int_matrix(64, 64, 3))[1:]:
        assert not bool(p.any())                       # integers up to 8: the hi plane alone
    for p in R.split3_bf16(R.onehot_matrix(64, 64, 3))[1:]:
        assert not bool(p.any())                       # a power of two: the hi plane alone
    hi, mid, lo = R.split3_bf16(R.onehot_matrix(64, 64, 3, mid_plane=True))
    assert int((hi != 0).sum()) == 64 and int((mid != 0).sum()) == 64 and not bool(lo.any())
    hi, mid, lo = R.split3_bf16(R.dense_matrix(64, 64, 3, bits=15))
    assert float((mid != 0).float().mean()) > 0.9 and not bool(lo.any())


def test_onehot_reaches_the_last_column():
    for rows, cols in ((1, 1), (5, 3), (3, 5), (64, 64)):
        oh = R.onehot_matrix(rows, cols, 1)
        assert int((oh != 0).sum()) == rows and bool((oh != 0).sum(1).eq(1).all())
        assert float(oh[0, cols - 1]) != 0.0
        if rows > 1 and cols > 1:
            assert float(oh[1, cols - 2]) != 0.0


@pytest.mark.parametrize("cls,left", CASES)
def test_expected_is_fp32_exact(built, cls, left):
    A, B, Y, keep = built[cls, left]
    share = float(keep.float().mean())
    if cls == "onehot_c":
        assert share >= 0.99, share
    else:
        assert share == 1.0, share
    assert bool(Y.any())


@pytest.mark.parametrize("cls,left", CASES)
def test_all_six_products_reproduce_expected(built, cls, left):
    A, B, Y, keep = built[cls, left]
    assert torch.equal(R.masked(R.mfma_x6(A, B), keep), R.masked(Y, keep))


@pytest.mark.parametrize("drop", range(6), ids=R.X6_NAMES)
def test_each_dropped_product_is_seen(built, drop):
    shares = {}
    for (cls, left), (A, B, Y, keep) in built.items():
        got = R.mfma_x6(A, B, drop=drop)
        shares[cls, left] = float((R.masked(got, keep) != R.masked(Y, keep)).float().mean())
    assert max(shares.values()) > 0.9, shares


def test_int_sums_stay_below_2_24():
    assert R.INT_MAX_ABS ** 2 * R.K_MAX < 2 ** 24
    # the worst operands the class can draw at the largest K: every product +64
    A = torch.full((3, R.K_MAX), float(R.INT_MAX_ABS))
    Y, keep = R.expected(A, -A)
    assert float(Y.abs().max()) == R.INT_MAX_ABS ** 2 * R.K_MAX < 2 ** 24 and bool(keep.all())
    A, B = R.operands("int", True, 64, 64, R.K_MAX, seed=5)
    assert float(A.abs().max()) == R.INT_MAX_ABS and float(B.abs().max()) == R.INT_MAX_ABS
    Y, keep = R.expected(A, B)
    assert float(Y.abs().max()) < 2 ** 24 and bool(keep.all())
    assert torch.equal(R.mfma_x6(A, B), Y)
