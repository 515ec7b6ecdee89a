// The per-edge 64 x 64 x 64 product of EBGCN's edge inference (EBGCN.py:95-116) and the epilogue
// of its networks, shared by the eval kernel (bgcn_ebgcn.hip) and the training kernels
// (bgcn_ebgcn_train.hip).  With a = h[(row_e - 1) mod N], b = h[(col_e - 1) mod N]:
//   D[c][l] = |a[c] - b[l]|,   Y[o][l] = sum_c Wc[o][c] D[c][l]
// on the fp32 MFMA (exact fp32 products): Wc is the A operand, held in 64 registers per lane for
// the whole block; D is the B operand, made in registers from the two 256-byte rows (one subtract
// + abs per element) and never stored.  One wave per edge, 256 threads per block.
#pragma once

#include "bgcn_common.h"

namespace bgcn {

constexpr int kH = 64;              // hidden size (the fork's only configuration)
constexpr int kMaxEdgeNum = 8;      // latent relation types (edge_num, default 2)
constexpr int kWLd = kH + 1;        // LDS row stride of the Wc staging tile (conflict-free column reads)
constexpr float kSlope = 0.01f;     // LeakyReLU's default

// The "- 1" is the reference's `x[row - 1]` as written: node ids are used one lower than the edge
// list says, and id 0 reads the LAST node (Python's negative index).  False: an end outside
// [0, N) - never a wild read; the caller decides what to write.
__device__ __forceinline__ bool edge_ends(const int64_t* __restrict__ ei, int64_t E, int64_t N, int64_t e,
                                          int64_t& ia, int64_t& ib) {
  const int64_t row = ei[e], col = ei[E + e];   // wave-uniform
  if (row < 0 || row >= N || col < 0 || col >= N) return false;
  ia = row == 0 ? N - 1 : row - 1;   // x[row - 1]: 0 wraps to the last node
  ib = col == 0 ? N - 1 : col - 1;
  return true;
}

// Wc [64][64] -> LDS (all 256 threads), then the A-operand image of the f32 MFMA:
// lane (r32, hh) holds wa[tt][s] = Wc[32 tt + r32][2 s + hh]
__device__ __forceinline__ void stage_w(const float* __restrict__ Wc, float* sW) {
  for (int i = threadIdx.x; i < kH * kH; i += 256) sW[(i >> 6) * kWLd + (i & 63)] = Wc[i];
}
__device__ __forceinline__ void load_wa(const float* sW, int r32, int hh, float (&wa)[2][32]) {
#pragma unroll
  for (int tt = 0; tt < 2; ++tt)
#pragma unroll
    for (int s = 0; s < 32; ++s) wa[tt][s] = sW[(32 * tt + r32) * kWLd + 2 * s + hh];
}

__device__ __forceinline__ void zero_acc(f32x16 (&acc)[2][2]) {
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
}

// av = a[lane], b0 = b[r32], b1 = b[32 + r32]; the B operand of k-step s is D[c = 2 s + hh][l]:
// acc[tt][u][r] = Y[o = 32 tt + 8 (r >> 2) + 4 hh + (r & 3)][l = 32 u + r32]
__device__ __forceinline__ void y_tile(const float (&wa)[2][32], float av, float b0, float b1, int hh,
                                       f32x16 (&acc)[2][2]) {
  zero_acc(acc);
#pragma unroll
  for (int s = 0; s < 32; ++s) {
    const float a = __shfl(av, 2 * s + hh);
    const float d0 = fabsf(a - b0), d1 = fabsf(a - b1);
    acc[0][0] = mfma32x32x2(wa[0][s], d0, acc[0][0]);
    acc[0][1] = mfma32x32x2(wa[0][s], d1, acc[0][1]);
    acc[1][0] = mfma32x32x2(wa[1][s], d0, acc[1][0]);
    acc[1][1] = mfma32x32x2(wa[1][s], d1, acc[1][1]);
  }
}
// the same product with the operands swapped: the transpose,
// acc[tt][u][r] = Y[o = 32 tt + r32][l = 32 u + 8 (r >> 2) + 4 hh + (r & 3)]
__device__ __forceinline__ void yt_tile(const float (&wa)[2][32], float av, float b0, float b1, int hh,
                                        f32x16 (&acc)[2][2]) {
  zero_acc(acc);
#pragma unroll
  for (int s = 0; s < 32; ++s) {
    const float a = __shfl(av, 2 * s + hh);
    const float d0 = fabsf(a - b0), d1 = fabsf(a - b1);
    acc[0][0] = mfma32x32x2(d0, wa[0][s], acc[0][0]);
    acc[0][1] = mfma32x32x2(d1, wa[0][s], acc[0][1]);
    acc[1][0] = mfma32x32x2(d0, wa[1][s], acc[1][0]);
    acc[1][1] = mfma32x32x2(d1, wa[1][s], acc[1][1]);
  }
}

__device__ __forceinline__ float f4at(const float4& v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }

// A network's epilogue on y_tile's accumulators, with the folded BatchNorm (sG, sT) and the
// output convolution's weights (sO) in LDS, [64] each and 16-byte aligned:
//   (x, y) = sum_o w_out[o] leaky_relu(g[o] Y[o][l] + t[o])   at l = r32, 32 + r32
// A lane sums its half-wave's rows o in accumulator order; the other half-wave holds the other
// rows of the same l, so after the exchange every lane has the whole sums.  b_out is the caller's.
__device__ __forceinline__ float2 edge_out_sums(const f32x16 (&acc)[2][2], const float* sG, const float* sT,
                                                const float* sO, int hh) {
  float s0 = 0.f, s1 = 0.f;
#pragma unroll
  for (int tt = 0; tt < 2; ++tt)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int o0 = 32 * tt + 8 * q + 4 * hh;
      const float4 Gv = *reinterpret_cast<const float4*>(&sG[o0]);
      const float4 Tv = *reinterpret_cast<const float4*>(&sT[o0]);
      const float4 Ov = *reinterpret_cast<const float4*>(&sO[o0]);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float z0 = fmaf(f4at(Gv, j), acc[tt][0][4 * q + j], f4at(Tv, j));
        float z1 = fmaf(f4at(Gv, j), acc[tt][1][4 * q + j], f4at(Tv, j));
        z0 = fmaxf(z0, kSlope * z0);   // LeakyReLU: the slope is below 1
        z1 = fmaxf(z1, kSlope * z1);
        s0 = fmaf(f4at(Ov, j), z0, s0);
        s1 = fmaf(f4at(Ov, j), z1, s1);
      }
    }
  s0 += __shfl_xor(s0, 32);
  s1 += __shfl_xor(s1, 32);
  return make_float2(s0, s1);
}

}  // namespace bgcn
