"""A CPU restatement of the fused Adam's arithmetic (adam_elem of bgcn_internal.h, the constants of
k_adam / TailAdam::c, the table of bigcn_amd/optim.py) and of the weight images its tile
epilogue writes (carve_images of bgcn_sparse.hip, the layouts of bgcn_sparse.h).
TEST INFRASTRUCTURE: tests/test_adam_ref.py checks it on the CPU, tests/test_gpu_adam.py compares
bgcn_adam_step with it bit for bit.

adam_elem spells out every operation (fmaf, __fmul_rn, __fsub_rn, __fdiv_rn, sqrtf) and the build
has no fast-math, so each of its results is one correctly rounded fp32 operation and the bits of an
update are defined.  numpy's fp32 multiply, subtract, divide and sqrt are correctly rounded too;
the fused multiply-add is `fma32` below.
"""
import math

import numpy as np
import torch

from gemm_ref import split3_bf16

F32 = np.float32
H = 64                  # rows of the conv weights with images
ALIGN = 256             # Carve::take: every image array starts on a 256-byte boundary
W2S_LD = 64 + 32 + 8    # kW2sLd: bf16 row stride of conv2's split image
W2D_LD = 64 + 8         # kW2dLd: bf16 row stride of the middle launch's split image
IMAGE_TD_W1, IMAGE_BU_W1, IMAGE_TD_W2, IMAGE_BU_W2 = 1, 2, 3, 4


def _f32(x):
    return np.ascontiguousarray(x, dtype=F32)


def fma32(a, b, c):
    """The correctly rounded fp32 value of a * b + c (fp32 arrays, finite values).

    The product of two 24-bit significands has 48 bits: exact in fp64.  s = fl64(ab + c) and the
    TwoSum residual e give ab + c = s + e exactly.  Where e != 0, s is replaced by the one of the
    two fp64 neighbours of the exact sum whose last significand bit is odd (round to odd); rounding
    that to fp32 gives the same result as rounding the exact sum, because fp64 carries
    53 >= 2 * 24 + 2 bits (Boldo & Melquiond, "Emulation of FMA and correctly rounded sums")."""
    a, b, c = np.broadcast_arrays(_f32(a), _f32(b), _f32(c))
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    t = s - p
    e = (p - (s - t)) + (c - t)
    bits = s.view(np.int64).copy()
    # the other neighbour lies towards e: one step up in the ordered integer image of |s|
    # when e and s have the same sign, one step down otherwise (s == 0 only when e == 0)
    step = np.where((e > 0) == (s > 0), 1, -1).astype(np.int64)
    fix = (e != 0) & ((bits & 1) == 0)
    bits = np.where(fix, bits + step, bits)
    return bits.view(np.float64).astype(F32)


class AdamConst:
    """The constants of one tensor's update as k_adam forms them from bgcn_adam_args: every field
    of the argument struct is a C float (ctypes rounds the Python doubles, the bias corrections
    1 - b1^t and sqrt(1 - b2^t) among them), and step / inv_bc2 / 1 - b are fp32 operations."""

    def __init__(self, lr, t, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=1.0,
                 bias_correction1=True, bias_correction2=True):
        b1, b2 = betas
        self.b1, self.b2, self.eps, self.wd, self.gs = F32(b1), F32(b2), F32(eps), F32(weight_decay), F32(grad_scale)
        bc1 = F32(1.0 - b1 ** t) if bias_correction1 else F32(1)
        bc2s = F32(math.sqrt(1.0 - b2 ** t)) if bias_correction2 else F32(1)
        self.step = F32(lr) / bc1
        self.inv_bc2 = F32(1) / bc2s
        self.omb1 = F32(1) - self.b1
        self.omb2 = F32(1) - self.b2


def adam_elem(p, g, m, v, c):
    """adam_elem of bgcn_internal.h, line by line, on fp32 arrays; returns the new (p, m, v)."""
    p, gr, m, v = _f32(p), _f32(g), _f32(m), _f32(v)
    g = fma32(c.wd, p, gr * c.gs)
    m = fma32(c.omb1, g - m, m)
    v = fma32(c.omb2, g * g, v * c.b2)
    denom = fma32(np.sqrt(v), c.inv_bc2, c.eps)
    p = fma32(-c.step, m / denom, p)
    return p, m, v


def adam_fp64(p, g, m, v, lr, t, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=1.0):
    """The same formula in fp64 from the Python doubles (torch.optim.Adam: L2 weight decay,
    amsgrad off): what the restatement approximates."""
    b1, b2 = betas
    p, g, m, v = (np.asarray(x, dtype=np.float64) for x in (p, g, m, v))
    g = g * grad_scale + weight_decay * p
    m = m + (1.0 - b1) * (g - m)
    v = b2 * v + (1.0 - b2) * g * g
    denom = np.sqrt(v) / math.sqrt(1.0 - b2 ** t) + eps
    p = p - lr / (1.0 - b1 ** t) * (m / denom)
    return p, m, v


# ------------------------------------------------------------------------------ weight images
def image_layout(F):
    """{name: (byte offset, shape, bytes per element)} of the four image arrays in carve order,
    and the end of the last one (bgcn_weight_images_size(F) - 256)."""
    out, off = {}, 0
    for name, shape, size in (("w1t", (F, 2 * H), 4), ("w2t", (2, F + H, H), 4),
                              ("w2s", (2, 3, H, W2S_LD), 2), ("w2d", (2, 3, H, W2D_LD), 2)):
        off = (off + ALIGN - 1) // ALIGN * ALIGN
        out[name] = (off, shape, size)
        off += int(np.prod(shape)) * size
    return out, off


def _bf16_bits(x):
    """The 16 bits of fp32 values that are bf16 numbers."""
    u = np.ascontiguousarray(x.numpy()).view(np.uint32)
    assert not (u & 0xFFFF).any()
    return (u >> 16).astype(np.uint16)


def images(F, td_w1, bu_w1, td_w2, bu_w2):
    """(bytes, mask): the contents of a weight-image buffer for conv weights W1_d [64, F] and
    W2_d [64, F + 64] (fp32 torch tensors; None = that tensor takes no update, its image region
    is not written), as uint8 arrays of bgcn_weight_images_size(F) - 256 bytes; mask marks the
    bytes the update defines.

    w1t [F][128] fp32:        w1t[k][64 d + o] = W1_d[o][k]
    w2t [2][F+64][64] fp32:   w2t[d][k][o] = W2_d[o][k]
    w2s [2][3][64][104] bf16: w2s[d][part][o][k] = part of W2_d[o][k], k < 64 (columns 64..103 are
                              conv2's root slots, not the optimiser's)
    w2d [2][3][64][72] bf16:  w2d[d][part][c][o] = part of W2_d[o][c], c < 64 (columns 64..71 pad
                              the rows to 16 bytes)
    part 0 / 1 / 2 = hi / mid / lo of split3_bf16; d = 0 top-down, 1 bottom-up."""
    layout, total = image_layout(F)
    data = np.zeros(total, np.uint8)
    mask = np.zeros(total, bool)

    def arrays(name, dtype):
        off, shape, size = layout[name]
        n = int(np.prod(shape)) * size
        return data[off:off + n].view(dtype).reshape(shape), mask[off:off + n].reshape(shape + (size,))

    w1t, k1 = arrays("w1t", np.float32)
    w2t, k2 = arrays("w2t", np.float32)
    w2s, ks = arrays("w2s", np.uint16)
    w2d, kd = arrays("w2d", np.uint16)
    for d, w in enumerate((td_w1, bu_w1)):
        if w is not None:
            assert tuple(w.shape) == (H, F) and w.dtype == torch.float32
            w1t[:, d * H:(d + 1) * H] = w.numpy().T
            k1[:, d * H:(d + 1) * H] = True
    for d, w in enumerate((td_w2, bu_w2)):
        if w is not None:
            assert tuple(w.shape) == (H, F + H) and w.dtype == torch.float32
            w2t[d] = w.numpy().T
            k2[d] = True
            for part, x in enumerate(split3_bf16(w[:, :H].contiguous())):
                b = _bf16_bits(x)
                w2s[d, part, :, :H] = b
                w2d[d, part, :, :H] = b.T
            ks[d, :, :, :H] = True
            kd[d, :, :, :H] = True
    return data, mask
