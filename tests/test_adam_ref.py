"""CPU checks of tests/adam_ref.py (TEST INFRASTRUCTURE): fma32 is the correctly rounded fused
multiply-add, the restatement of adam_elem is Adam (within the error its fp32 operations allow, and
not without weight decay, grad_scale or either bias correction), and images() is the layout
bgcn_sparse.h documents."""
import struct
from fractions import Fraction

import numpy as np
import pytest
import torch

import adam_ref as R

U = 2.0 ** -24          # the relative error bound of one correctly rounded fp32 operation


# ---------------------------------------------------------------------------------------- fma32
def _round_f32(x):
    """A Fraction rounded once to fp32 (nearest, ties to even; subnormals included), as a float."""
    if x == 0:
        return 0.0
    sign, x = (-1.0, -x) if x < 0 else (1.0, x)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    assert Fraction(2) ** e <= x < Fraction(2) ** (e + 1)
    q = max(e, -126) - 23                      # the exponent of the last significand bit
    y = x / Fraction(2) ** q
    n = y.numerator // y.denominator
    rem = y - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    assert n <= 2 ** 24 and q + 24 <= 128
    return sign * float(np.ldexp(float(n), q))


def _full(rng, n, emin=-20, emax=20):
    """Full-mantissa fp32 numbers with the last bit set: a product of two needs all 48 bits."""
    x = (rng.standard_normal(n) * np.exp2(rng.integers(emin, emax + 1, n))).astype(np.float32)
    return (x.view(np.uint32) | 1).view(np.float32)


def _fma_triples():
    rng = np.random.default_rng(0)
    n = 2000
    out = {}
    a, b = _full(rng, n), _full(rng, n)
    out["random"] = (a, b, _full(rng, n))
    # c of the product's magnitude (within a factor 2^-3 .. 2^3): the sum's last bits come from both
    ab = (a.astype(np.float64) * b).astype(np.float32)
    out["same_scale"] = (a, b, (_full(rng, n, 0, 0) * ab * np.exp2(rng.integers(-3, 4, n))).astype(np.float32))
    # c far above / far below the product: the smaller term only decides the rounding direction
    out["sticky"] = (a, b, (ab * np.exp2(rng.choice([-60, -30, -25, -24, 24, 25, 30, 60], n))).astype(np.float32))
    out["c_zero"] = (a, b, np.zeros(n, np.float32))
    # cancellation: c = -fl32(ab), the result is the product's rounding error (an fp32 number);
    # and c one ulp beside it
    out["cancel"] = (a, b, -ab)
    out["cancel_near"] = (a, b, -np.nextafter(ab, np.float32(np.inf)))
    # exact midpoints: c an even integer well inside [2^24, 2^25) (ulp 2), ab an odd integer below
    # 2^12 -> the sum is an odd integer of that range: a tie
    odd = lambda: (2 * rng.integers(0, 32, n) + 1).astype(np.float32)
    c = (2 * rng.integers(2 ** 23 + 2 ** 12, 2 ** 24 - 2 ** 12, n)).astype(np.float32) * rng.choice([-1.0, 1.0], n).astype(np.float32)
    out["midpoint"] = (odd() * rng.choice([-1.0, 1.0], n).astype(np.float32), odd(), c)
    # half an ulp of c times (1 - 2^-46): the fp64 sum rounds ONTO the midpoint, so a plain
    # double rounding (without the round-to-odd step) goes wrong for odd c
    c = _full(rng, n)
    half = np.exp2(np.floor(np.log2(np.abs(c.astype(np.float64)))) - 24)
    s = rng.choice([-1.0, 1.0], n)
    out["near_midpoint"] = ((np.float32(1 + 2.0 ** -23) * half * s).astype(np.float32),
                            np.full(n, 1 - 2.0 ** -23, np.float32), c)
    return out


def test_fma32_is_the_correctly_rounded_fma():
    total = 0
    for name, (a, b, c) in _fma_triples().items():
        got = R.fma32(a, b, c)
        assert got.dtype == np.float32
        for x, y, z, r in zip(a.tolist(), b.tolist(), c.tolist(), got.tolist()):
            want = _round_f32(Fraction(x) * Fraction(y) + Fraction(z))
            assert struct.pack("<f", r) == struct.pack("<f", want), (name, x, y, z, r, want)
        total += len(a)
    assert total >= 10 ** 4


def test_fma32_classes_are_what_they_claim():
    """The midpoint classes do defeat a product-then-sum in fp64 rounded twice."""
    t = _fma_triples()
    a, b, c = t["near_midpoint"]
    naive = (a.astype(np.float64) * b + c).astype(np.float32)
    assert (naive != R.fma32(a, b, c)).mean() > 0.2
    a, b, c = t["midpoint"]
    s = a.astype(np.float64) * b + c
    assert (s % 2 == 1).all() and (np.abs(s) > 2 ** 24).all()
    a, b, c = t["cancel"]
    assert (R.fma32(a, b, c) != 0).mean() > 0.9


# ------------------------------------------------------------------------------ the restatement
HP = dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4, grad_scale=1.0 / 3)
LR = 5e-4


def _state(seed, n=4096):
    rng = np.random.default_rng(seed)
    p = (0.1 * rng.standard_normal(n)).astype(np.float32)
    g = (3e-3 * rng.standard_normal(n)).astype(np.float32)
    m = (1e-4 * rng.standard_normal(n)).astype(np.float32)
    v = (1e-7 * rng.random(n) + 1e-9).astype(np.float32)
    return p, g, m, v


def _bounds(p, g, m, v, t):
    """First-order error bounds (Ep, Em, Ev) of adam_elem against adam_fp64, per element.

    Each fp32 operation and each constant rounded from a Python double contributes a relative
    error of at most U = 2^-24.  With the exact quantities in capitals:
      constants  beta, eps, wd, gs, lr, bc1, bc2s: U each; step = lr / bc1: 3 U (two constants, one
                 division); inv_bc2 = 1 / bc2s: 2 U; 1 - beta is exact in fp32 (Sterbenz), so it
                 inherits beta's absolute error: relative beta / (1 - beta) U (9 U and 999 U);
      G  = wd P + GR gs          Eg = 2 U |GR gs| + U |wd P| + U |G|        (constant + product, constant, fma)
      D  = G - M                 Ed = Eg + U |D|
      M' = M + w1 D              Em = w1 Ed + 9 U |w1 D| + U |M'|
      V' = b2 V + w2 G^2         Ev = 2 U |b2 V| + w2 (2 |G| Eg + U G^2) + 999 U w2 G^2 + U |V'|
      S  = sqrt(V')              Es = Ev / (2 S) + U S
      DEN = S ibc2 + eps         Eden = ibc2 Es + 2 U S ibc2 + U eps + U DEN
      Q  = M' / DEN              Eq = Em / DEN + |Q| Eden / DEN + U |Q|
      P' = P - step Q            Ep = step Eq + 3 U step |Q| + U |P'|
    The products of two errors that this drops are below 1000 U of the terms kept: the bounds are
    multiplied by 1.01."""
    b1, b2 = HP["betas"]
    wd, gs, eps = HP["weight_decay"], HP["grad_scale"], HP["eps"]
    P, GR, M, V = (x.astype(np.float64) for x in (p, g, m, v))
    w1, w2 = 1 - b1, 1 - b2
    e1, e2 = b1 / w1 * U, b2 / w2 * U
    ibc2, step = 1 / np.sqrt(1 - b2 ** t), LR / (1 - b1 ** t)
    G = wd * P + GR * gs
    Eg = 2 * U * np.abs(GR * gs) + U * np.abs(wd * P) + U * np.abs(G)
    D = G - M
    Ed = Eg + U * np.abs(D)
    M1 = M + w1 * D
    Em = w1 * Ed + e1 * np.abs(w1 * D) + U * np.abs(M1)
    V1 = b2 * V + w2 * G * G
    Ev = 2 * U * b2 * V + w2 * (2 * np.abs(G) * Eg + U * G * G) + e2 * w2 * G * G + U * V1
    S = np.sqrt(V1)
    Es = Ev / (2 * S) + U * S
    DEN = S * ibc2 + eps
    Eden = ibc2 * Es + 2 * U * S * ibc2 + U * eps + U * DEN
    Q = M1 / DEN
    Eq = Em / DEN + np.abs(Q) * Eden / DEN + U * np.abs(Q)
    P1 = P - step * Q
    Ep = step * Eq + 3 * U * step * np.abs(Q) + U * np.abs(P1)
    return 1.01 * Ep, 1.01 * Em, 1.01 * Ev


def _within(got, want, bounds):
    return [bool((np.abs(x.astype(np.float64) - y) <= e).all()) for x, y, e in zip(got, want, bounds)]


@pytest.mark.parametrize("t", [1, 2, 1000])
def test_restatement_is_adam(t):
    p, g, m, v = _state(t)
    want = R.adam_fp64(p, g, m, v, LR, t, **HP)
    bounds = _bounds(p, g, m, v, t)
    got = R.adam_elem(p, g, m, v, R.AdamConst(LR, t, **HP))
    assert all(x.dtype == np.float32 for x in got)
    assert _within(got, want, bounds) == [True, True, True]
    # the bound is no blanket: it is a few ulp of each result, and the update is far above it
    assert float(np.median(bounds[0] / np.abs(want[0]))) < 4 * U
    assert float(np.median(np.abs(want[0] - p) / bounds[0])) > 1e3
    # ... and not Adam with a piece left out
    without = {
        "weight_decay": R.AdamConst(LR, t, **dict(HP, weight_decay=0.0)),
        "grad_scale": R.AdamConst(LR, t, **dict(HP, grad_scale=1.0)),
        "bias_correction2": R.AdamConst(LR, t, bias_correction2=False, **HP),
    }
    if t < 1000:        # 1 - 0.9^1000 is 1 in fp64: the first correction has nothing left to remove
        without["bias_correction1"] = R.AdamConst(LR, t, bias_correction1=False, **HP)
    else:
        assert 1.0 - 0.9 ** t == 1.0
    for name, c in without.items():
        ok = _within(R.adam_elem(p, g, m, v, c), want, bounds)
        assert not ok[0], name                                  # the parameter always shows it
        if name in ("weight_decay", "grad_scale"):
            assert ok == [False, False, False], name            # and so do both moments


def test_constants_are_formed_in_fp32():
    """step, inv_bc2 and 1 - beta as the kernel forms them, not as fp64 would."""
    c = R.AdamConst(5e-4 / 5, 2, **HP)
    f = np.float32
    assert c.step == f(5e-4 / 5) / f(1.0 - 0.9 ** 2) and c.step.dtype == np.float32
    assert c.inv_bc2 == f(1) / f(np.sqrt(1.0 - 0.999 ** 2))
    assert c.omb1 == f(1) - f(0.9) and c.omb1 != f(0.1)
    assert c.omb2 == f(1) - f(0.999) and c.omb2 != f(0.001)
    assert c.wd == f(1e-4) and c.gs == f(1.0 / 3) and c.eps == f(1e-8)


def test_zero_gradient_leaves_a_fresh_parameter_alone():
    p = _state(5)[0]
    z = np.zeros_like(p)
    p1, m1, v1 = R.adam_elem(p, z, z, z, R.AdamConst(LR, 1))
    assert p1.tobytes() == p.tobytes() and not m1.any() and not v1.any()


# ------------------------------------------------------------------------------- weight images
def _weights(F, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [0.1 * torch.randn(64, K, generator=g) for K in (F, F, F + 64, F + 64)]


@pytest.mark.parametrize("F", [4, 60, 64, 132, 260])
def test_image_sizes(F):
    layout, total = R.image_layout(F)
    sizes = {"w1t": F * 128 * 4, "w2t": 2 * (F + 64) * 64 * 4, "w2s": 2 * 3 * 64 * 104 * 2, "w2d": 2 * 3 * 64 * 72 * 2}
    off = 0
    for name in ("w1t", "w2t", "w2s", "w2d"):
        off = (off + 255) // 256 * 256
        assert layout[name][0] == off and off % 256 == 0, name
        off += sizes[name]
    assert total == off
    data, mask = R.images(F, *_weights(F))
    assert data.size == mask.size == total
    # defined bytes: both halves of W1^T, both W2^T, 64 of 104 / 72 columns of the split images
    assert int(mask.sum()) == sizes["w1t"] + sizes["w2t"] + 2 * (2 * 3 * 64 * 64 * 2)
    from bigcn_amd import _lib
    assert _lib.load_library().bgcn_weight_images_size(F) == total + 256


def _bf16(data, off, index):
    """The bf16 number at element `index` of the array at byte `off`, as a float."""
    (bits,) = struct.unpack_from("<H", data, off + 2 * index)
    return struct.unpack("<f", struct.pack("<I", bits << 16))[0]


@pytest.mark.parametrize("F", [4, 68, 132])
def test_image_transposes_and_splits(F):
    """Every element, read back from the bytes by the index formulas of bgcn_sparse.h."""
    w = _weights(F, seed=F)
    data, mask = R.images(F, *w)
    layout, _ = R.image_layout(F)
    raw = data.tobytes()
    K2 = F + 64
    for d in (0, 1):
        w1, w2 = w[d].numpy(), w[2 + d].numpy()
        for o in range(64):
            for k in range(F):
                at = layout["w1t"][0] + 4 * (k * 128 + d * 64 + o)
                assert struct.unpack_from("<f", raw, at)[0] == w1[o, k]
                assert mask[at:at + 4].all()
            for k in range(K2):
                at = layout["w2t"][0] + 4 * ((d * K2 + k) * 64 + o)
                assert struct.unpack_from("<f", raw, at)[0] == w2[o, k]
                assert mask[at:at + 4].all()
            for k in range(64):
                s = [_bf16(raw, layout["w2s"][0], ((d * 3 + part) * 64 + o) * 104 + k) for part in range(3)]
                t = [_bf16(raw, layout["w2d"][0], ((d * 3 + part) * 64 + k) * 72 + o) for part in range(3)]
                assert s == t
                assert s[0] + s[1] + s[2] == float(w2[o, k])          # (exact in fp64)
                assert s[0] == float(torch.tensor(w2[o, k]).bfloat16()) and abs(s[2]) <= abs(s[1]) <= abs(s[0])
    # the padding columns are not the optimiser's
    ks = mask[layout["w2s"][0]:layout["w2s"][0] + 2 * 3 * 64 * 104 * 2].reshape(2, 3, 64, 104, 2)
    kd = mask[layout["w2d"][0]:layout["w2d"][0] + 2 * 3 * 64 * 72 * 2].reshape(2, 3, 64, 72, 2)
    assert ks[..., :64, :].all() and not ks[..., 64:, :].any()
    assert kd[..., :64, :].all() and not kd[..., 64:, :].any()
    assert not data[~mask].any()


def test_images_of_a_missing_tensor_are_undefined():
    F = 68
    w = _weights(F)
    full, fmask = R.images(F, *w)
    for drop in range(4):
        part = list(w)
        part[drop] = None
        data, mask = R.images(F, *part)
        assert (fmask & ~mask).sum() == (64 * F * 4 if drop < 2 else 64 * (F + 64) * 4 + 2 * 3 * 64 * 64 * 2)
        assert not (mask & ~fmask).any()
        assert (data[mask] == full[mask]).all()
