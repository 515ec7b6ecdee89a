// Device bodies over the batch's trees: the node -> root map and tree pointers, the tree
// work items and the dW2 root-column partials per item.  Shared by the sparse forward
// (k_prologue, k_items: bgcn_sparse.hip), the batch preparation (k_prep_a, k_prep_b:
// bgcn_prep.hip) and the backward's middle launch (k_bwd_mid: bgcn_sparse_bwd.hip).
#pragma once

#include "bgcn_bwd.h"
#include "bgcn_internal.h"
#include "bgcn_sparse.h"

namespace bgcn {

// Batch part of the prologue (block bid of blockDim threads): blocks [0, nR) the node ->
// root map (block 0 also resets the overflow flags), then the tree pointers (binary
// search in the sorted batch vector).
__device__ inline void prologue_batch_body(const SparseState& S, const int64_t* __restrict__ batch,
                                           const int64_t* __restrict__ rootindex,
                                           int32_t* __restrict__ node_root, int32_t* __restrict__ tree_ptr,
                                           int bid, int nR) {
  if (bid == 0 && nR > 0 && S.mode != 1 && threadIdx.x < 8) S.flags[threadIdx.x] = 0;
  if (bid < nR) {
    const int64_t i = int64_t(bid) * blockDim.x + threadIdx.x;
    if (i >= S.N) return;
    const int64_t b = batch[i];
    // a node in no tree would keep stale backward rows (the readout never visits it):
    // flagged as a bad index, which invalidates the step
    if ((b < 0 || b >= S.B) && S.bstatus) atomicOr(S.bstatus, 1);
    const int64_t bc = b < 0 ? 0 : (b >= S.B ? S.B - 1 : b);
    const int64_t r = rootindex[bc];
    node_root[i] = int32_t((b >= 0 && b < S.B && r >= 0 && r < S.N) ? r : 0);
    return;
  }
  const int64_t b = int64_t(bid - nR) * blockDim.x + threadIdx.x;
  if (b > S.B) return;
  int64_t lo = 0, hi = S.N;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (batch[mid] < b) lo = mid + 1; else hi = mid;
  }
  tree_ptr[b] = int32_t(lo);
}

// ---------------------------------------------------------------- dW2 root columns, part 1
// Work item = (tree b, chunk of <= kChunk nodes of b), blockIdx.y = direction:
// part[d][item][s][o] = sum_{i in chunk} keep_i[64 + col_s] * dZ2_d[i][o] for the root's
// non-zeros s (the 2 relu(x) factor is applied in k_dw_cols).
// one block: items per tree = ceil(n_b / kChunk), exclusive scan over trees (1024 at a
// time with a carry), then every tree writes its item descriptors.
__device__ inline void items_body(const SparseState& S, const int32_t* __restrict__ tree_ptr,
                                  const int64_t* __restrict__ rootindex) {
  if (S.mode == 1) return;   // (not the overflow flag: the pass over X may run beside this)
  __shared__ int sh[1024];
  __shared__ int carry;
  const int nth = int(blockDim.x);
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int64_t b0 = 0; b0 < S.B; b0 += nth) {
    const int64_t b = b0 + threadIdx.x;
    const int t0 = b < S.B ? tree_ptr[b] : 0, t1 = b < S.B ? tree_ptr[b + 1] : 0;
    const int chunks = (t1 - t0 + kChunk - 1) / kChunk;
    sh[threadIdx.x] = chunks;
    __syncthreads();
    for (int o = 1; o < nth; o <<= 1) {
      const int v = threadIdx.x >= o ? sh[threadIdx.x - o] : 0;
      __syncthreads();
      sh[threadIdx.x] += v;
      __syncthreads();
    }
    const int first = carry + sh[threadIdx.x] - chunks;
    if (b < S.B) {
      S.tree_item0[b] = first < S.max_items ? first : S.max_items;
      // the item's node range and root stored with it: its readers skip the tree_ptr /
      // rootindex level of their dependent load chains
      const int64_t r = rootindex[b];
      const int32_t root = int32_t(r >= 0 && r < S.N ? r : 0);
      for (int q = 0; q < chunks && first + q < S.max_items; ++q) {
        S.item_tree[first + q] = int32_t(b);
        S.item_beg[first + q] = t0 + q * kChunk;
        S.item_end[first + q] = min(t0 + (q + 1) * kChunk, t1);
        S.item_root[first + q] = root;
      }
    }
    __syncthreads();
    if (threadIdx.x == nth - 1) carry += sh[nth - 1];
    __syncthreads();
  }
  if (threadIdx.x == 0) S.tree_item0[S.B] = carry < S.max_items ? carry : S.max_items;
}

// dW2 root-column partials per work item (<= kChunk nodes of one tree), on the MFMA:
//   part[s][o] = sum_{i in item} kept_d(i, s) * dZ2_d[i][o]      (s < 32 root slots)
// a [32 x nodes] x [nodes x 64] product with the 0/1 keep masks of the forward (S.rbits)
// as A.  Each wave takes 64 of the item's nodes (lane half h owns 32 of them: permuted
// K); the four waves' partials are combined in a fixed order.
// Device body, 256 threads: work item `item` of direction d; smem: kRootPartSmem floats.
constexpr int kRootPartSmem = kChunk + 4 * kCap * H;
__device__ inline void root_part_body(const SparseState& S, const float* __restrict__ dZ2,
                                      const int32_t* __restrict__ tree_ptr, int item, int d,
                                      float* smem) {
  if (!use_sparse(S)) return;
  if (item >= S.tree_item0[S.B]) return;
  uint32_t* bits = reinterpret_cast<uint32_t*>(smem);
  float (*red)[kCap * H] = reinterpret_cast<float (*)[kCap * H]>(smem + kChunk);
  const int64_t beg = S.item_beg[item], end = S.item_end[item];
  for (int t = threadIdx.x; t < kChunk; t += 256) {
    const int64_t i = beg + t;
    bits[t] = i < end ? S.rbits[int64_t(d) * S.N + i] : 0u;
  }
  __syncthreads();
  const int wv = threadIdx.x >> 6, l = threadIdx.x & 63, r32 = l & 31, h = l >> 5;
  f32x16 acc0 = {}, acc1 = {};
  if (beg + wv * 64 < end) {
    // bf16 MFMA: A = the 0/1 keep bits (exact in bf16), B = dZ2 split hi + mid + lo
    // (three products: all 24 bits, the fp32-grade dW2 root columns); k-step s takes
    // nodes n0 + 16s + 8h + j
    const int64_t n0 = beg + wv * 64;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      bf16x8 a, b0h, b0m, b0l, b1h, b1m, b1l;
      float z0[8], z1[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int64_t node = n0 + 16 * s + 8 * h + j;
        const float* zr = dZ2 + (node < end ? node : beg) * (2 * H) + d * H;
        z0[j] = zr[r32];
        z1[j] = zr[32 + r32];
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int64_t node = n0 + 16 * s + 8 * h + j;
        const bool ok = node < end;
        a[j] = __bf16((ok && ((bits[node - beg] >> r32) & 1u)) ? 1.f : 0.f);
        __bf16 x, y, z;
        split3_bf16(ok ? z0[j] : 0.f, x, y, z);
        b0h[j] = x; b0m[j] = y; b0l[j] = z;
        split3_bf16(ok ? z1[j] : 0.f, x, y, z);
        b1h[j] = x; b1m[j] = y; b1l[j] = z;
      }
      acc0 = mfma_bf16(a, b0l, acc0);
      acc0 = mfma_bf16(a, b0m, acc0);
      acc0 = mfma_bf16(a, b0h, acc0);
      acc1 = mfma_bf16(a, b1l, acc1);
      acc1 = mfma_bf16(a, b1m, acc1);
      acc1 = mfma_bf16(a, b1h, acc1);
    }
  }
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int sl = (q & 3) + 8 * (q >> 2) + 4 * h;
    red[wv][sl * H + r32] = acc0[q];
    red[wv][sl * H + 32 + r32] = acc1[q];
  }
  __syncthreads();
  float* out = S.root_part + (int64_t(d) * S.max_items + item) * (kCap * H);
  for (int e = threadIdx.x; e < kCap * H; e += 256)
    out[e] = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
}

}  // namespace bgcn
