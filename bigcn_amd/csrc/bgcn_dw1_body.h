// Device bodies of the tail launch's pass over the CSC of X (k_bwd_tail,
// bgcn_sparse_bwd.hip): dW1, the dW2 root columns and the fused optimiser step's extra
// block.
#pragma once

#include "bgcn_bwd.h"
#include "bgcn_internal.h"
#include "bgcn_sparse.h"

namespace bgcn {

// Both bodies walk the CSC of X by column (slot and value side by side: k_csc_place stores
// the value next to the slot); (row, value) of an entry reach the wave by scalar readlane.
// dW1 = [dZ1_td | dZ1_bu]^T X is dw1_sliced_body's; the forms that gave a column one or
// four whole waves (each lane 2 of the 128 outputs, chosen by a knob) lost to it and are
// gone (profiles/r02_split_ab.txt, profiles/r02_dw1_slices_ab.txt).  What is left of them
// is dw2_root_cols_body: the dW2 root columns alone, for the deferred-dW1 step.
// Device bodies, up to 1024 threads, column block bid; smem: kDw1Smem floats (the tail
// launch's LDS, kept at the size it has had: more than either body needs).
constexpr int kDw1Smem = 2 * 2 * H * 17;
// Spilled root entries (a root row of more than kCap words): their dW2 root-column
// partial is summed over the tree's nodes directly (no ELL slot, no item partial):
//   sum_{i in tree b} keep_d(i, 64 + c) * dZ2_d[i][o]
__device__ __forceinline__ void tree_range(const SparseState& S, int b, int64_t& nb, int64_t& ne) {
  const int it0 = S.tree_item0[b], it1 = S.tree_item0[b + 1];
  nb = it1 > it0 ? S.item_beg[it0] : 0;
  ne = it1 > it0 ? S.item_end[it1 - 1] : 0;
}

// The dW2 root columns only, one wave per column, each lane owning 2 of the 128 outputs (no
// dZ1 gathers, dW1 untouched: the deferred-dW1 step's first tail launch).  A root entry
// with an ELL slot adds its terms in dw1_sliced_body's order (root rows in CSC order, a
// tree's item partials in item order, four loads in flight), so the deferred step gives
// the bits of the one-call step; a spilled root's tree is summed in node order.
__device__ inline void dw2_root_cols_body(const SparseState& S, const int64_t* __restrict__ batch,
                                          float* __restrict__ dw2_td, float* __restrict__ dw2_bu, float scale,
                                          int bid, float* smem, const float* __restrict__ dZ2,
                                          const KeepSrc& keep) {
  const int cols = int(blockDim.x >> 6);   // columns per block
  if (!use_sparse(S)) return;
  float (*t2)[17] = reinterpret_cast<float (*)[17]>(smem);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t F = S.F;
  const int64_t c = int64_t(bid) * cols + wave;
  const int rd = lane >> 5, ro = (2 * lane) & (H - 1);   // this lane's (direction, output pair)
  float2 a2 = make_float2(0.f, 0.f);
  if (c < F) {
    const int64_t beg = S.col_start[c], end = S.col_end[c];
    for (int64_t u0 = beg; u0 < end; u0 += 64) {
      const int64_t u = min<int64_t>(u0 + lane, end - 1);   // clamped: duplicates, x masked
      const uint2 ent = S.csc[u];
      const uint32_t slot = ent.x & kCscSlotMask;
      const float xv = __uint_as_float(ent.y);
      const int n = int(min<int64_t>(64, end - u0));
      const float x_l = lane < n ? xv : 0.f;
      const int32_t i_l = int32_t(slot / kCap);
      // dW2 root columns: dW2_d[:, 64 + c] = sum over the root rows holding column c (tree
      // order = CSC row order) of 2 relu(x) * sum_items root_part[d][item][slot] - the
      // root entries (rare) are flagged in the CSC record, so this pass over the column
      // finds them (a separate role re-read every column and gathered node_root per entry)
      uint64_t m = __ballot(lane < n && (ent.x & kCscRootFlag));
      while (m) {   // in row (= tree) order
        const int j = __builtin_ctzll(m);
        m &= m - 1;
        const int32_t i = __builtin_amdgcn_readlane(i_l, j);     // j is wave-uniform
        const int32_t sl = int32_t(__builtin_amdgcn_readlane(int32_t(slot), j) % kCap);
        const float f = scale * fmaxf(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(x_l), j)), 0.f);
        const int b = int(batch[i]);
        float2 sum = make_float2(0.f, 0.f);
        if (__builtin_amdgcn_readlane(int32_t(ent.x), j) & int32_t(kCscSpillFlag)) {
          int64_t nb, ne;
          tree_range(S, b, nb, ne);
          const uint32_t k = uint32_t(H + c);
          for (int64_t n0 = nb; n0 < ne; n0 += 4) {   // four rows in flight, in node order
            float2 z[4];
            uint32_t kw[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const int64_t nd = min(n0 + u, ne - 1);
              z[u] = *reinterpret_cast<const float2*>(dZ2 + nd * (2 * H) + rd * H + ro);
              kw[u] = keep.get(uint32_t(rd), uint32_t(nd), k >> 5);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
              if (n0 + u < ne && ((kw[u] >> (k & 31)) & 1u)) {
                sum.x += z[u].x;
                sum.y += z[u].y;
              }
          }
          a2.x = fmaf(f, sum.x, a2.x);
          a2.y = fmaf(f, sum.y, a2.y);
          continue;
        }
        const int it0 = S.tree_item0[b], it1 = S.tree_item0[b + 1];
        for (int it = it0; it < it1; it += 4) {   // four item partials in flight, in item order
          float2 v[4];
#pragma unroll
          for (int q = 0; q < 4; ++q)
            v[q] = *reinterpret_cast<const float2*>(
                S.root_part + (int64_t(rd) * S.max_items + min(it + q, it1 - 1)) * (kCap * H) + sl * H + ro);
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (it + q < it1) {
              sum.x += v[q].x;
              sum.y += v[q].y;
            }
        }
        a2.x = fmaf(f, sum.x, a2.x);
        a2.y = fmaf(f, sum.y, a2.y);
      }
    }
  }
  t2[2 * lane][wave] = a2.x;
  t2[2 * lane + 1][wave] = a2.y;
  __syncthreads();
  // store through LDS (the block's consecutive columns per output row); every root column
  // is written (zero when no root holds it)
  const int tx = threadIdx.x % cols;
  const int64_t cc = int64_t(bid) * cols + tx;
  const int64_t K2 = F + H;
  for (int ty = threadIdx.x / cols; ty < 2 * H && cc < F; ty += int(blockDim.x) / cols) {
    float* dst2 = ty < H ? dw2_td + int64_t(ty) * K2 : dw2_bu + int64_t(ty - H) * K2;
    dst2[H + cc] = t2[ty][tx];
  }
}

// dW1 by output slices, XCD-aware.  The 128-wide dZ1 row splits into
// kSlices slices of kSliceW outputs; the blocks of XCD x (blocks are dispatched to the
// XCDs round-robin: block b runs on XCD b % 8) take slice x % kSlices of every column of
// their column groups, so an XCD's L2 serves the gathers of ONE slice of dZ1 - N x 128 B
// (3.9 MB at Twitter size) instead of the whole 15.7 MB table, most of which the
// column-per-wave form fetched from the Infinity Cache (PMC: 140 MB per launch, the
// fabric-bound ~7 TB/s).  A wave takes one (column, slice): kSliceGroups entries per
// gather instruction (kSliceLanes lanes x 16 B per entry), kSliceDepth rounds in flight;
// the lane groups' partials are combined by a fixed xor-shuffle tree (deterministic).  The
// dW2 root columns ride along as in dw2_root_cols_body (same per-output order, same values).
#ifndef BGCN_DW1_SLICES
#define BGCN_DW1_SLICES 4
#endif
#ifndef BGCN_DW1_DEPTH
#define BGCN_DW1_DEPTH 4
#endif
constexpr int kSlices = BGCN_DW1_SLICES;
constexpr int kSliceW = 2 * H / kSlices;          // outputs per slice
constexpr int kSliceLanes = kSliceW / 4;          // lanes per entry (one float4 each)
constexpr int kSliceGroups = 64 / kSliceLanes;    // entries per gather instruction
constexpr int kSliceDepth = BGCN_DW1_DEPTH;
static_assert(8 % kSlices == 0 && kSliceW <= H && kSliceLanes >= 1, "slices");
static_assert(kDw1Smem >= 2 * kSliceW * 17 && kDw1Smem >= 2 * H * 17, "both bodies at 16 waves per block");
__device__ __forceinline__ float4 shfl4(float4 v, int src) {
  return make_float4(__shfl(v.x, src, 64), __shfl(v.y, src, 64), __shfl(v.z, src, 64), __shfl(v.w, src, 64));
}
__device__ __forceinline__ float4 shfl_xor4(float4 v, int m) {
  return make_float4(__shfl_xor(v.x, m, 64), __shfl_xor(v.y, m, 64), __shfl_xor(v.z, m, 64),
                     __shfl_xor(v.w, m, 64));
}
// blocks of the sliced form for F columns with W waves (= columns) per block
__host__ __device__ inline int dw1_sliced_blocks(int64_t F, int W) {
  const int64_t groups = (F + W - 1) / W, reps = 8 / kSlices;
  return int(8 * ((groups + reps - 1) / reps));
}
// rows in flight per lane group in the spilled-root sweep (rare): 1 keeps the launch at 64
// VGPRs, 8 dW1 waves per SIMD (4: 80 VGPRs, 6 waves; twitter15 +1 %,
// profiles/r03_tail_depth_ab.txt)
#ifndef BGCN_SPILL_DEPTH
#define BGCN_SPILL_DEPTH 1
#endif
constexpr int kSpillDepth = BGCN_SPILL_DEPTH;
template <int kPart = 0>   // 0: dW1 + the dW2 root columns, 2: dW1 only
__device__ inline void dw1_sliced_body(const SparseState& S, const float* __restrict__ dZ1,
                                       float* __restrict__ dw1_td, float* __restrict__ dw1_bu,
                                       const int64_t* __restrict__ batch, float* __restrict__ dw2_td,
                                       float* __restrict__ dw2_bu, float scale, int bid, float* smem,
                                       const float* __restrict__ dZ2, const KeepSrc& keep,
                                       const TailAdam* ad = nullptr) {
  if (!use_sparse(S)) return;
  const int W = int(blockDim.x >> 6);
  const int64_t F = S.F;
  const int x = bid & 7, sl_ = x % kSlices;
  const int64_t cg = int64_t(bid >> 3) * (8 / kSlices) + x / kSlices;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int g = lane / kSliceLanes, q = lane % kSliceLanes;
  const int so = kSliceW * sl_, d = so / H, oo = so % H + 4 * q;   // slice start, direction, my outputs
  const int64_t c = cg * W + wave;
  // the fused optimiser step (TailAdam, kPart 0): this block's kSliceW outputs x W columns of
  // W1_d and of W2_d's root columns - their parameters and moments requested here, beside
  // the gathers, and updated with the finished gradients at the end
  const bool fa = kPart == 0 && ad && ad->on && int(threadIdx.x) < kSliceW * W && !ad->skip();
  const int ka1 = d == 0 ? 0 : 4, ka2 = d == 0 ? 2 : 6;
  const int a_ol = int(threadIdx.x) / W, a_tx = int(threadIdx.x) % W;
  const int64_t a_cc = min<int64_t>(cg * W + a_tx, F - 1);
  const int64_t ia1 = int64_t(so % H + a_ol) * F + a_cc, ia2 = int64_t(so % H + a_ol) * (F + H) + H + a_cc;
  float ap1 = 0.f, am1 = 0.f, av1 = 0.f, ap2 = 0.f, am2 = 0.f, av2 = 0.f;
  if (fa) {
    ap1 = ad->p[ka1][ia1]; am1 = ad->m[ka1][ia1]; av1 = ad->v[ka1][ia1];
    ap2 = ad->p[ka2][ia2]; am2 = ad->m[ka2][ia2]; av2 = ad->v[ka2][ia2];
  }
  float4 a1 = f4zero(), a2 = f4zero();
  bool spill_root = false;
  if (c < F) {
    const int64_t beg = S.col_start[c], end = S.col_end[c];
    // the next 64 CSC entries are requested before this chunk's gathers (clamped: duplicates, x masked):
    // loads retire in order, so they cost no wait, and the chunk loop then takes one
    // dependent round trip less per 64 entries
    // (32-bit entry indices: the CSC holds fewer than 2^31 entries, kSparseMaxN)
    const int32_t be = int32_t(beg), en = int32_t(end);
    uint2 ent_nx = be < en ? S.csc[min(be + lane, en - 1)] : make_uint2(0u, 0u);
    for (int32_t u0 = be; u0 < en; u0 += 64) {
      const uint2 ent = ent_nx;
      if (u0 + 64 < en) ent_nx = S.csc[min(u0 + 64 + lane, en - 1)];
      const uint32_t slot = ent.x & kCscSlotMask;
      const int n = min(64, en - u0);
      const float x_l = lane < n ? __uint_as_float(ent.y) : 0.f;
      const int32_t i_l = int32_t(slot / kCap);
      for (int j0 = 0; j0 < n; j0 += kSliceGroups * kSliceDepth) {
        float4 gv[kSliceDepth];
        float xx[kSliceDepth];
#pragma unroll
        for (int v = 0; v < kSliceDepth; ++v) {
          const int j = j0 + v * kSliceGroups + g;
          const int jc = j < n ? j : n - 1;
          const int32_t i = __shfl(i_l, jc, 64);
          const float xv = __shfl(x_l, jc, 64);
          xx[v] = j < n ? xv : 0.f;
          gv[v] = ld4(dZ1 + int64_t(i) * (2 * H) + so + 4 * q);
        }
#pragma unroll
        for (int v = 0; v < kSliceDepth; ++v) a1 = f4fma(xx[v], gv[v], a1);
      }
      uint64_t m = kPart == 2 ? 0ull : __ballot(lane < n && (ent.x & kCscRootFlag));
      while (m) {   // root entries, in row (= tree) order; lane group 0 holds the slice
        const int j = __builtin_ctzll(m);
        m &= m - 1;
        const int32_t i = __builtin_amdgcn_readlane(i_l, j);
        const int32_t sl = int32_t(__builtin_amdgcn_readlane(int32_t(slot), j) % kCap);
        const float f = scale * fmaxf(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(x_l), j)), 0.f);
        if (__builtin_amdgcn_readlane(int32_t(ent.x), j) & int32_t(kCscSpillFlag)) {
          spill_root = true;   // summed after the column's main pass (its registers are free then)
          continue;
        }
        if (g != 0) continue;
        const int b = int(batch[i]);
        float4 sum = f4zero();
        const int it0 = S.tree_item0[b], it1 = S.tree_item0[b + 1];
        for (int it = it0; it < it1; it += 4) {   // four item partials in flight, in item order
          float4 v[4];
#pragma unroll
          for (int qq = 0; qq < 4; ++qq)
            v[qq] = ld4(S.root_part + (int64_t(d) * S.max_items + min(it + qq, it1 - 1)) * (kCap * H) + sl * H + oo);
#pragma unroll
          for (int qq = 0; qq < 4; ++qq)
            if (it + qq < it1) sum = f4add(sum, v[qq]);
        }
        a2 = f4fma(f, sum, a2);
      }
    }
    if (spill_root) {
      // the column's spilled root entries (a root row of more than kCap words, rare), in
      // row order: sum_{i in tree} keep_d(i, 64 + c) * dZ2_d[i] - lane group g takes the
      // tree's nodes g, g + 8, ..., the groups' partials combined by the fixed xor tree
      const uint32_t k = uint32_t(H + c);
      for (int64_t u0 = beg; u0 < end; u0 += 64) {
        const int64_t u = min<int64_t>(u0 + lane, end - 1);
        const uint2 ent = S.csc[u];
        const int n = int(min<int64_t>(64, end - u0));
        uint64_t m = __ballot(lane < n && (ent.x & kCscRootFlag) && (ent.x & kCscSpillFlag));
        while (m) {
          const int j = __builtin_ctzll(m);
          m &= m - 1;
          const int32_t i = int32_t((uint32_t(__builtin_amdgcn_readlane(int32_t(ent.x), j)) & kCscSlotMask) / kCap);
          const float f = scale * fmaxf(__int_as_float(__builtin_amdgcn_readlane(int32_t(ent.y), j)), 0.f);
          int64_t nb, ne;
          tree_range(S, int(batch[i]), nb, ne);
          float4 sum = f4zero();
          for (int64_t n0 = nb + g; n0 < ne; n0 += kSpillDepth * kSliceGroups) {   // rows in flight
            float4 z[kSpillDepth];
            uint32_t kw[kSpillDepth];
#pragma unroll
            for (int v = 0; v < kSpillDepth; ++v) {
              const int64_t nd = min(n0 + v * kSliceGroups, ne - 1);
              z[v] = ld4(dZ2 + nd * (2 * H) + d * H + oo);
              kw[v] = keep.get(uint32_t(d), uint32_t(nd), k >> 5);
            }
#pragma unroll
            for (int v = 0; v < kSpillDepth; ++v)
              if (n0 + v * kSliceGroups < ne && ((kw[v] >> (k & 31)) & 1u)) sum = f4add(sum, z[v]);
          }
#pragma unroll
          for (int off = kSliceLanes; off < 64; off <<= 1) sum = f4add(sum, shfl_xor4(sum, off));
          if (g == 0) a2 = f4fma(f, sum, a2);
        }
      }
    }
  }
#pragma unroll
  for (int off = kSliceLanes; off < 64; off <<= 1) a1 = f4add(a1, shfl_xor4(a1, off));
  float* t1 = smem;                                 // [kSliceW][W + 1]
  float* t2 = smem + kSliceW * (W + 1);
  if (g == 0) {
    const float v1[4] = {a1.x, a1.y, a1.z, a1.w}, v2[4] = {a2.x, a2.y, a2.z, a2.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      t1[(4 * q + j) * (W + 1) + wave] = v1[j];
      t2[(4 * q + j) * (W + 1) + wave] = v2[j];
    }
  }
  __syncthreads();
  const int64_t K2 = F + H;
  float* w1 = d == 0 ? dw1_td : dw1_bu;
  float* w2 = d == 0 ? dw2_td : dw2_bu;
  for (int e = threadIdx.x; e < kSliceW * W; e += int(blockDim.x)) {
    const int ol = e / W, tx = e % W;
    const int64_t cc = cg * W + tx;
    if (cc >= F) continue;
    const int o = so % H + ol;
    const float g1 = t1[ol * (W + 1) + tx], g2 = t2[ol * (W + 1) + tx];
    w1[int64_t(o) * F + cc] = g1;
    if (kPart != 2) w2[int64_t(o) * K2 + H + cc] = g2;
    if (fa && e == int(threadIdx.x)) {   // (this thread's prefetched pair: a_ol == ol, a_cc == cc)
      adam_elem(ap1, g1, am1, av1, ad->c(ka1));
      ad->p[ka1][ia1] = ap1; ad->m[ka1][ia1] = am1; ad->v[ka1][ia1] = av1;
      adam_elem(ap2, g2, am2, av2, ad->c(ka2));
      ad->p[ka2][ia2] = ap2; ad->m[ka2][ia2] = am2; ad->v[ka2][ia2] = av2;
      if (ad->w1t) {
        ad->w1t[cc * (2 * H) + d * H + o] = ap1;                 // W1^T[c][d*64 + o]
        ad->w2t[(int64_t(d) * K2 + H + cc) * H + o] = ap2;       // W2^T_d[64 + c][o]
      }
    }
  }
}

// The fused optimiser step's parameters without a tail role of their own (b2: the middle
// launch's db2; the head's fc weight and bias), one extra block of the tail launch; it also
// counts a skipped update as k_adam does.
__device__ inline void tail_adam_block(const TailAdam& ad) {
  if (ad.skip()) {
    if (threadIdx.x == 0 && ad.skip_count) atomicAdd(ad.skip_count, 1);
    return;
  }
  const int ks[4] = {3, 7, 8, 9};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int k = ks[q];
    const AdamConst c = ad.c(k);
    for (int64_t e = threadIdx.x; e < ad.n[k]; e += blockDim.x) {
      float p = ad.p[k][e], m = ad.m[k][e], v = ad.v[k][e];
      adam_elem(p, ad.g[k][e], m, v, c);
      ad.p[k][e] = p;
      ad.m[k][e] = m;
      ad.v[k][e] = v;
    }
  }
}

}  // namespace bgcn
