// Backward of the sparse-feature path (see bgcn_sparse.hip): the merged middle and tail
// launches, the dense feature mode's dW2 launches, and their host launchers.
#include <cstdlib>
#include <cstring>

#include "bgcn_bwd.h"
#include "bgcn_dw1_body.h"
#include "bgcn_internal.h"
#include "bgcn_items_body.h"
#include "bgcn_sparse.h"
#include "bgcn_trace.h"

namespace bgcn {
namespace {

// ---------------------------------------------------------------- merged backward launches
// middle (256 threads): dH1 (+ the relu(H1) block of dW2), db2 column sums, dW2 partials
// (dense path), dW2 root partials, the head's weight gradients;  tail (512 threads): dW1
// over the CSC, dW2 root columns, the dW2 partial reduction, db1 column sums.  Roles by
// block range, in that order.
// db2 from the readout's per-item positive-H2 counts (BwdMidArgs::db2_dhead): dH2 of a
// row is [H2 > 0] * dhead[b] / |tree b| (BiGCN_Twitter.py:57,65), so column c of db2 =
// sum_i dH2[i][c] = sum over items p of count[p][c] * dhead[tree(p)][hc] / |tree(p)|; one
// block per column, the fixed order of colsum_col_block (items past tree_item0[B]: none).
__device__ inline void db2_from_counts(const BwdMidArgs& a, int c, float* sm) {
  const int nit = a.S.tree_item0[a.S.B];
  const int hc = c < H ? 2 * H + c : c - H;   // head input = cat(BU, TD) (:128)
  const float* cnt = a.db2.part;
  float acc = 0.f;
  for (int p0 = 0; p0 < nit; p0 += 4 * 256) {   // 4 items per thread in flight
    int32_t b[4];
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int p = min(p0 + u * 256 + int(threadIdx.x), nit - 1);
      b[u] = a.S.item_tree[p];
      v[u] = cnt[int64_t(p) * 128 + c];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t bb = min<int64_t>(max<int64_t>(b[u], 0), a.S.B - 1);
      const float n = float(max(a.tree_ptr[bb + 1] - a.tree_ptr[bb], 1));
      const float g = a.db2_dhead[bb * kHeadIn + hc];
      if (p0 + u * 256 + int(threadIdx.x) < nit) acc += v[u] * (g / n);
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float s = ((sm[0] + sm[1]) + sm[2]) + sm[3];
    if (c < H) a.db2.out_td[c] = s; else a.db2.out_bu[c - H] = s;
  }
}

constexpr int cmax(int a, int b) { return a > b ? a : b; }
constexpr int kMidSmem = cmax(cmax(cmax(kDw2Smem, kRootPartSmem), cmax(kDh1Smem, kColsumSmem)), kHeadGradSmem);
template <class TX>
__global__ __launch_bounds__(256, 2) void k_bwd_mid(BwdMidArgs a) {   // LDS: two blocks per CU (dh1_body)
  __shared__ __attribute__((aligned(16))) float smem[kMidSmem];
  BT_BEGIN
  int b = int(blockIdx.x);
  if (b < 2 * a.nblk_h) {   // longest-lived role first
    // the relu(H1) block of dW2 rides along when the sparse path is the one running
    float* part = (a.S.mode != 1 && !dense_active(a.gate)) ? a.dw2_sparse.part : nullptr;
    dh1_body(a.dZ2, a.H1, a.W2td, a.W2bu, a.S.F + H, a.S.N, a.keep, a.dH1, a.colpart, a.rows_h, part,
             a.nblk_h, b % a.nblk_h, b / a.nblk_h, smem, a.S.mode != 1 ? a.S.w2d : nullptr);
    BT_END(72);
    return;
  }
  b -= 2 * a.nblk_h;
  if (b < kColsumColBlocks) {   // db2 before the short roles: not the launch's last blocks
    if (a.db2_dhead) db2_from_counts(a, b, smem);
    else colsum_col_block(a.db2, b, smem);
    BT_END(73);
    return;
  }
  b -= kColsumColBlocks;
  if (b < a.n_dw2) {
    dw2_body<TX>(static_cast<const TX*>(a.X), a.ldx, a.S.F, a.H1, a.dZ2, a.node_root, a.S.N, a.keep,
                 a.gate, a.dw2_dense, a.dw2_sparse, a.n_dw2_dense, b, smem);
    BT_END(70);
    return;
  }
  b -= a.n_dw2;
  if (b < a.n_root) {
    root_part_body(a.S, a.dZ2, a.tree_ptr, b % a.S.max_items, b / a.S.max_items, smem);
    BT_END(71);
    return;
  }
  head_grad_block(a.hg, b - a.n_root, smem);
}

constexpr int kTailSmem = cmax(cmax(kDw1Smem, kRedSmem), kColsumSmem);
#ifndef BGCN_TAIL_THREADS
#define BGCN_TAIL_THREADS 512   // 1024-thread blocks ran one per CU: dW1 in two rounds
#endif
constexpr int kTailThreads = BGCN_TAIL_THREADS;   // threads per block of the tail launch
// kPart (the deferred-dW1 step, bgcn_step_args.defer_dw1): 0 = every role; 1 = all but dW1
// (the dW2 root columns by one wave per column, dw2_root_cols_body); 2 = dW1 only
template <int kPart>
__global__ __launch_bounds__(kTailThreads) void k_bwd_tail(BwdTailArgs a) {
  __shared__ __attribute__((aligned(16))) float smem[kTailSmem];
  BT_BEGIN
  int b = int(blockIdx.x);
  if (b < a.n_dw1) {
    if constexpr (kPart == 1)
      dw2_root_cols_body(a.S, a.batch, a.dw2_td, a.dw2_bu, a.keep_scale, b, smem, a.dZ2, a.keep);
    else
      dw1_sliced_body<kPart>(a.S, a.dZ1, a.dw1_td, a.dw1_bu, a.batch, a.dw2_td, a.dw2_bu, a.keep_scale, b,
                             smem, a.dZ2, a.keep, &a.adam);
    BT_END(80);
    return;
  }
  if (kPart == 2) return;
  b -= a.n_dw1;
  if (b < a.red_dense.blocks + a.red_sparse.blocks) {
    reduce_dw2_body(a.dw2_part, a.S.F + H, a.dw2_td, a.dw2_bu, a.gate, a.red_dense, a.red_sparse, b, smem,
                    &a.adam);
    BT_END(82);
    return;
  }
  b -= a.red_dense.blocks + a.red_sparse.blocks;
  if (b < colsum_job_blocks(kTailThreads)) {
    colsum_job_block(a.db1, b, smem, &a.adam);
    BT_END(83);
    return;
  }
  if (a.adam.on) tail_adam_block(a.adam);   // the launch's last block
}

}  // namespace

// The dense feature mode's dW2 root columns for bf16 X (dw2_bf16_body) as a launch of its
// own: ~45 KB of LDS, three blocks per CU (inside the middle launch they ran at its two
// per CU).
// The H1 columns' blocks (dw2_body's column tile 0: f32 MFMA, a split's k-tiles in
// sequence, the launch's longest-lived blocks) go first, so they run beside the root
// columns instead of lengthening the middle launch.
constexpr int kDw2RootSmem = cmax(kDw2bSmem, kDw2Smem);
__global__ __launch_bounds__(256) void k_dw2_bf16(BwdMidArgs a) {
  __shared__ __attribute__((aligned(16))) float smem[kDw2RootSmem];
  int b = int(blockIdx.x);
  if (b < a.n_dw2h) {
    dw2_body<bf16_t>(static_cast<const bf16_t*>(a.X), a.ldx, a.S.F, a.H1, a.dZ2, a.node_root, a.S.N, a.keep,
                     a.gate, a.dw2_dense, a.dw2_sparse, a.n_dw2_dense, b, smem);
    return;
  }
  b -= a.n_dw2h;
  dw2_bf16_body(static_cast<const bf16_t*>(a.X), a.ldx, a.S.F, a.dZ2, a.node_root, a.S.N, a.keep, a.gate,
                a.dw2_dense, a.gxb, b, smem);
}

// ... and for fp32 X (dw2_root_body: k-tiles of one root's nodes, the root factor
// applied per tile in fp32), same LDS and block ids; TX = bf16_t: the same form for bf16 X
// (the default; BGCN_DW2_ROOT=0 keeps k_dw2_bf16).
#ifndef BGCN_DW2R_WPE
#define BGCN_DW2R_WPE 3   // three waves per SIMD (dw2_root_body: 162 VGPRs)
#endif
template <class TX>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(BGCN_DW2R_WPE))) void k_dw2_root(BwdMidArgs a) {
  __shared__ __attribute__((aligned(16))) float smem[kDw2RootSmem];
  int b = int(blockIdx.x);
  if (b < a.n_dw2h) {
    dw2_body<TX>(static_cast<const TX*>(a.X), a.ldx, a.S.F, a.H1, a.dZ2, a.node_root, a.S.N, a.keep,
                 a.gate, a.dw2_dense, a.dw2_sparse, a.n_dw2_dense, b, smem);
    return;
  }
  b -= a.n_dw2h;
  dw2_root_body<TX>(static_cast<const TX*>(a.X), a.ldx, a.S.F, a.dZ2, a.node_root, a.S.N, a.keep, a.gate,
                    a.dw2_dense, a.gxb, b, smem);
}

int dw2_bf16_launch(BwdMidArgs& a, hipStream_t s) {
  if (a.n_dw2b <= 0) return BGCN_OK;
  const unsigned n = unsigned(a.n_dw2b + a.n_dw2h);
  if (a.dw2b_f32 == 1)
    hipLaunchKernelGGL(k_dw2_root<float>, dim3(n), dim3(256), 0, s, a);
  else if (a.dw2b_f32 == 2)
    hipLaunchKernelGGL(k_dw2_root<bf16_t>, dim3(n), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(k_dw2_bf16, dim3(n), dim3(256), 0, s, a);
  BGCN_CHECK_LAUNCH();
  return BGCN_OK;
}

// The dense feature mode's dW2 (fp32 X; dw2_body, f32 MFMA) as a launch of its own: inside
// the middle launch it ran at that launch's register budget (210 VGPRs since the fused
// dH1 + relu(H1)-dW2 role of round 3: two waves per SIMD) - 76.5 -> 64 TF/s.
__global__ __launch_bounds__(256) void k_dw2_f32(BwdMidArgs a) {
  __shared__ __attribute__((aligned(16))) float smem[kDw2Smem];
  dw2_body<float>(static_cast<const float*>(a.X), a.ldx, a.S.F, a.H1, a.dZ2, a.node_root, a.S.N, a.keep,
                  a.gate, a.dw2_dense, a.dw2_sparse, a.n_dw2_dense, int(blockIdx.x), smem);
}

int dw2_f32_launch(BwdMidArgs& a, hipStream_t s) {
  if (a.n_dw2f <= 0) return BGCN_OK;
  hipLaunchKernelGGL(k_dw2_f32, dim3(unsigned(a.n_dw2f)), dim3(256), 0, s, a);
  BGCN_CHECK_LAUNCH();
  return BGCN_OK;
}

int bwd_mid_launch(BwdMidArgs& a, int x_dtype, hipStream_t s) {
  a.n_root = (a.S.mode != 1) ? 2 * a.S.max_items : 0;
  const int n = a.n_dw2 + a.n_root + 2 * a.nblk_h + kColsumColBlocks + a.n_hg;
  if (x_dtype == BGCN_DTYPE_BF16)
    hipLaunchKernelGGL(k_bwd_mid<bf16_t>, dim3(unsigned(n)), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(k_bwd_mid<float>, dim3(unsigned(n)), dim3(256), 0, s, a);
  BGCN_CHECK_LAUNCH();
  return BGCN_OK;
}

int bwd_tail_launch(BwdTailArgs& a, hipStream_t s, int part) {
  // dW1 by the XCD-aware output slices (dw1_sliced_body); the forms of one and of four
  // whole waves per column that it replaced: profiles/r02_split_ab.txt
  const bool sparse = a.S.mode != 1;
  constexpr int wpb = kTailThreads / 64;   // waves per block
  a.n_dw1 = !sparse ? 0 : dw1_sliced_blocks(a.S.F, wpb);
  if (part == 1) a.n_dw1 = !sparse ? 0 : int((a.S.F + wpb - 1) / wpb);   // root columns: a wave per column
  // the reduction configurations are sized in 1024-thread blocks (4 groups of 256)
  a.red_dense.blocks *= 1024 / kTailThreads;
  a.red_sparse.blocks *= 1024 / kTailThreads;
  if (part != 0) a.adam.on = 0;   // (bigcn_backward_impl only fuses into part 0)
  const int n = part == 2 ? a.n_dw1
                          : a.n_dw1 + a.red_dense.blocks + a.red_sparse.blocks + colsum_job_blocks(kTailThreads) +
                                (a.adam.on ? 1 : 0);
  if (n == 0) return BGCN_OK;
  if (part == 1)
    hipLaunchKernelGGL(k_bwd_tail<1>, dim3(unsigned(n)), dim3(kTailThreads), 0, s, a);
  else if (part == 2)
    hipLaunchKernelGGL(k_bwd_tail<2>, dim3(unsigned(n)), dim3(kTailThreads), 0, s, a);
  else
    hipLaunchKernelGGL(k_bwd_tail<0>, dim3(unsigned(n)), dim3(kTailThreads), 0, s, a);
  BGCN_CHECK_LAUNCH();
  return BGCN_OK;
}

}  // namespace bgcn

BT_READER(sparse_bwd)
