// Sparse-feature path of the fused BiGCN encoder.
//
// The reference's node features are bag-of-words counts (Process/getTwittergraph.py:
// 67-72: x[n, 5000] holds the "idx:count" pairs of one post, ~10-20 non-zeros) stored
// dense.  Every product with X or with the root-extended X[root] is exact when the
// zero entries are skipped (x * w == 0 for x == 0), so this path reads the dense X from
// HBM exactly once per step, compacts every row to an ELL list (col, val) of at most
// kCap entries, and evaluates
//   conv1        Z1[i]         = sum_s val_s * W1^T[col_s]                      (K2)
//   conv2        Z2_d[i]       = sum_{k<64} a_ik W2_d^T[k] + sum_{s in root(i)} a_is W2_d^T[64+col_s]
//   dW2 (root)   dW2_d[:,64+c] = sum_{b: c in root_b} 2 relu(x_rb,c) sum_{i in b} keep_i[64+c] dZ2_d[i]
//   dW1          dW1[:, c]     = sum_{i: x_ic != 0} x_ic dZ1[i]                 (K10)
// (a_ik = keep * 2 * relu(.)), every sum in a fixed order (deterministic).  dW1 and the
// dW2 root columns come out of one pass over the column-sorted (CSC) non-zeros of X.
// A row with more than kCap non-zeros sets a device flag that switches the whole batch
// to the dense MFMA path (identical results); every kernel of both paths checks the flag
// on the device, so the choice costs no host sync.
#include <cstdlib>
#include <cstring>

#include "bgcn_compact_body.h"
#include "bgcn_csc_body.h"
#include "bgcn_internal.h"
#include "bgcn_items_body.h"
#include "bgcn_sparse.h"
#include "bgcn_trace.h"

namespace bgcn {
namespace {

// the prologue's clears when its launch is skipped (weight images current): the step's
// status word and the readout tickets, by conv1's block 0 (both are first used by the
// readout, two launches later)
__device__ __forceinline__ void conv1_clears(const SparseState& S) {
  if (!S.conv1_clears || blockIdx.x != 0) return;
  if (threadIdx.x == 0 && S.zero_word) *S.zero_word = 0;
  if (S.rtick)
    for (int64_t b = threadIdx.x; b < S.B; b += blockDim.x) S.rtick[b] = 0;
}

// ---------------------------------------------------------------- weight transposes
// W1T[c][d*64 + o] = W1_d[o][c] (c < F) and W2T_d[k][o] = W2_d[o][k] (k < 64+F):
// 32 x 32 tiles through LDS; blockIdx.z: 0/1 = W1 td/bu, 2/3 = W2 td/bu.
__device__ __forceinline__ void transpose_tile(const SparseState& S, int bx, int by, int z,
                                               const float* __restrict__ w1td,
                                               const float* __restrict__ w1bu,
                                               const float* __restrict__ w2td,
                                               const float* __restrict__ w2bu) {
  __shared__ float tile[32][33];
  const int64_t K = z < 2 ? S.F : S.F + H;
  const float* src = z == 0 ? w1td : z == 1 ? w1bu : z == 2 ? w2td : w2bu;
  const int64_t k0 = int64_t(bx) * 32;
  const int o0 = by * 32;
  if (k0 >= K) return;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int r = ty; r < 32; r += 8) {
    const int64_t k = k0 + tx;
    tile[r][tx] = k < K ? src[int64_t(o0 + r) * K + k] : 0.f;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int64_t k = k0 + r;
    if (k >= K) continue;
    if (z < 2) S.w1t[k * (2 * H) + z * H + o0 + tx] = tile[tx][r];
    else S.w2t[(int64_t(z - 2) * K + k) * H + o0 + tx] = tile[tx][r];
  }
}

// W2_d[:, :64] split for the bf16 MFMA (kSplitBlocks 256-thread blocks per direction, one
// element per thread): conv2's image [3][o][k] and the middle launch's [3][c][o] (hi / mid /
// lo: both feed fp32-grade six-product MFMAs).
constexpr int kSplitBlocks = H * H / 256;
__device__ inline void split_w2_block(const SparseState& S, int sb, const float* __restrict__ w2td,
                                      const float* __restrict__ w2bu) {
  const int d = sb / kSplitBlocks;
  const float* W2 = d == 0 ? w2td : w2bu;
  const int64_t ld = S.F + H;
  __bf16* cs = S.w2s + int64_t(d) * 3 * H * kW2sLd;
  __bf16* ds = S.w2d + int64_t(d) * 3 * H * kW2dLd;
  {
    const int e = (sb % kSplitBlocks) * 256 + threadIdx.x;
    const int o = e >> 6, k = e & 63;
    __bf16 x, y, z;
    const float v = W2[int64_t(o) * ld + k];
    split3_bf16(v, x, y, z);
    cs[o * kW2sLd + k] = x;
    cs[H * kW2sLd + o * kW2sLd + k] = y;
    cs[2 * H * kW2sLd + o * kW2sLd + k] = z;
    split3_bf16(v, x, y, z);
    ds[k * kW2dLd + o] = x;
    ds[H * kW2dLd + k * kW2dLd + o] = y;
    ds[2 * H * kW2dLd + k * kW2dLd + o] = z;
  }
}

// Forward prologue, one launch: the weight transposes (sparse path), node -> root map,
// tree pointers (binary search in the sorted batch vector) and the overflow-flag reset.
// Block ranges: [0, nT) transposes, [nT, nT + nR) node_root, then tree_ptr.
__global__ __launch_bounds__(256) void k_prologue(SparseState S, const float* __restrict__ w1td,
                                                  const float* __restrict__ w1bu,
                                                  const float* __restrict__ w2td,
                                                  const float* __restrict__ w2bu,
                                                  const int64_t* __restrict__ batch,
                                                  const int64_t* __restrict__ rootindex,
                                                  int32_t* __restrict__ node_root,
                                                  int32_t* __restrict__ tree_ptr, int nTx, int nT,
                                                  int nR) {
  const int blk = blockIdx.x;
  if (blk == 0 && threadIdx.x == 0 && S.zero_word) *S.zero_word = 0;
  if (blk == 0 && S.rtick)
    for (int64_t b = threadIdx.x; b < S.B; b += blockDim.x) S.rtick[b] = 0;
  if (blk < nT) {
    if (S.mode == 1) return;
    transpose_tile(S, blk % nTx, (blk / nTx) % 2, blk / (2 * nTx), w1td, w1bu, w2td, w2bu);
    return;
  }
  const int nS = nT > 0 ? 2 * kSplitBlocks : 0;   // the split W2 images ride with the transposes
  if (blk < nT + nS) {
    split_w2_block(S, blk - nT, w2td, w2bu);
    return;
  }
  prologue_batch_body(S, batch, rootindex, node_root, tree_ptr, blk - nT - nS, nR);
}

// ---------------------------------------------------------------- X compaction + conv1
// (the pass over X: bgcn_compact_body.h)

// bgcn_csr_to_dense: one wave per row, the row assembled in LDS (zeros, then the row's
// entries) and written with 16-byte stores - every output element written once, in order.
template <class TX>
__global__ __launch_bounds__(128) void k_csr_dense(const int32_t* __restrict__ rp, const int32_t* __restrict__ rc,
                                                   const float* __restrict__ rv, int64_t N, int64_t F,
                                                   TX* __restrict__ X, int64_t ldx, int32_t* status) {
  extern __shared__ __attribute__((aligned(16))) float rowbuf[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t Fp = (F + 3) / 4 * 4;
  float* row = rowbuf + wave * Fp;
  const int nw = int(blockDim.x) >> 6;
  for (int64_t i = int64_t(blockIdx.x) * nw + wave; i < N; i += int64_t(gridDim.x) * nw) {
    for (int64_t c = lane; c < Fp; c += 64) row[c] = 0.f;
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    const int32_t b = rp[i], e = rp[i + 1];
    for (int32_t k = b + lane; k < e; k += 64) {
      const int32_t c = rc[k];
      if (c >= 0 && c < F) row[c] = rv[k];
      else if (status) atomicOr(status, 1);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    TX* out = X + i * ldx;
    if constexpr (sizeof(TX) == 4) {
      for (int64_t c = int64_t(lane) * 4; c < F; c += 256)
        *reinterpret_cast<float4*>(out + c) = *reinterpret_cast<const float4*>(row + c);
    } else {   // round to nearest even (the host-fed values of a bf16 batch are bf16-exact)
      for (int64_t c = lane; c < F; c += 64) {
        const uint32_t u = __float_as_uint(row[c]);
        out[c] = TX((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

// the per-op encoder's forward: compaction + conv1 in one pass over X
template <class TX>
__global__ __launch_bounds__(256) void k_compact_conv1(SparseState S, const TX* __restrict__ X,
                                                       int64_t ldx, float* __restrict__ Z1) {
  compact_body<true, TX>(S, X, ldx, Z1, int(blockIdx.x), int(gridDim.x));
}

// conv1 lin from a prepared ELL of X (bgcn_prepare_batch), the 128 outputs of both
// directions per row.  The kernel is latency-bound (ELL load -> W1^T row gathers from L2 ->
// store per row), so a wave keeps several rows' gathers in flight instead of one (measured
// at Weibo size: 62 us for one row per wave, beside nothing).  Two rows per wave: half-wave
// h (32 lanes) owns row 2w + h, lane l of a half the outputs [4l, 4l + 4) - one 16-byte load
// per lane per entry, a wave instruction still moves 1 KiB (two 512-byte W1^T rows).  Entry
// s of a row reaches its half by shuffle; past a row's count the value is 0 and the
// (clamped) column still loads, so every load is unconditional.  The loop runs to the
// longer of the two rows in steps of kStep entries (a wave-uniform bound; 4 is the one
// instantiation).  Tried four rows per wave (one per 16-lane quarter, steps of 8) and two
// rows in steps of 8: more padded gathers and more registers (fewer waves per SIMD).
// Long rows (more than kCap non-zeros: the ELL list + the spill pool) get a block each
// instead of a half-wave: a long row walked by one half-wave is a serial chain of gathers
// (270 entries: ~70 us at 4 in flight), so the block's four waves take a quarter of the
// entries each, 8 gathers in flight per wave, combined in wave order (deterministic).
// Blocks stride over the compaction's list of long rows; with none they exit at once.
constexpr int kLongRowBlocks = 256;
__device__ inline void conv1_long_rows(const SparseState& S, float* __restrict__ Z1, int bid, int nblk) {
  __shared__ float part[4][2 * H];
  const int n_long = S.flags[2];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int q = bid; q < n_long; q += nblk) {
    const int64_t i = S.long_rows[q];
    const int nall = S.nnz[i];
    const int64_t off = S.ovf_off[i];
    const int seg = (nall + 3) / 4;
    const int e0 = wv * seg, e1 = min(nall, e0 + seg);
    float2 acc = make_float2(0.f, 0.f);
    for (int k0 = e0; k0 < e1; k0 += 64) {
      const int n = min(64, e1 - k0);
      const int e = k0 + min(lane, n - 1);
      // ELL entry (e < kCap) or pool entry: both loaded from clamped indices, selected after
      const int32_t ce = S.cols[i * kCap + min(e, kCap - 1)];
      const float ve = S.vals[i * kCap + min(e, kCap - 1)];
      const uint2 pe = S.ovf[off + max(e - kCap, 0)];
      const float2 p = conv1_row(S, n, e < kCap ? ce : int32_t(pe.x), e < kCap ? ve : __uint_as_float(pe.y));
      acc.x += p.x;
      acc.y += p.y;
    }
    part[wv][2 * lane] = acc.x;
    part[wv][2 * lane + 1] = acc.y;
    __syncthreads();
    if (threadIdx.x < 2 * H)
      Z1[i * (2 * H) + threadIdx.x] = (part[0][threadIdx.x] + part[1][threadIdx.x]) +
                                     (part[2][threadIdx.x] + part[3][threadIdx.x]);
    __syncthreads();
  }
}

// Entries of two rows per wave (half h: row 2w + h) held by the half's lanes (cl, vl of
// lane hl: entry hl), cnt of this half, cmax the wave-uniform bound: acc += val * W1^T[col].
template <int kStep>
__device__ __forceinline__ float4 conv1_half_entries(const SparseState& S, int32_t cl, float vl, int cnt,
                                                     int cmax, float4 acc) {
  const int lane = threadIdx.x & 63, hl = lane & 31, hb = lane & 32;
  for (int s0 = 0; s0 < cmax; s0 += kStep) {
    float4 w[kStep];
    float x[kStep];
#pragma unroll
    for (int u = 0; u < kStep; ++u) {
      const int sl = s0 + u;                          // uniform, < kCap
      const int32_t c = __shfl(cl, hb + (sl & 31), 64);
      const float v = __shfl(vl, hb + (sl & 31), 64);
      x[u] = sl < cnt ? v : 0.f;
      const int32_t cc = min(max(c, 0), int32_t(S.F - 1));
      w[u] = ld4(S.w1t + int64_t(cc) * (2 * H) + 4 * hl);
    }
#pragma unroll
    for (int u = 0; u < kStep; ++u) acc = f4fma(x[u], w[u], acc);
  }
  return acc;
}
// Blocks [0, kLongRowBlocks): the long rows (conv1_long_rows); then two rows per wave.
template <int kStep>
__global__ __launch_bounds__(256) void k_conv1_rows2(SparseState S, float* __restrict__ Z1) {
  BT_BEGIN
  conv1_clears(S);
  if (!use_sparse(S)) return;
  const int bx = int(blockIdx.x);
  if (bx < kLongRowBlocks) {
    conv1_long_rows(S, Z1, bx, kLongRowBlocks);
    return;
  }
  const int lane = threadIdx.x & 63, hl = lane & 31;
  const int64_t i = (int64_t(bx - kLongRowBlocks) * 4 + (threadIdx.x >> 6)) * 2 + (lane >> 5);
  const bool live = i < S.N;
  const int64_t ic = live ? i : S.N - 1;
  const int nall = live ? S.nnz[ic] : 0;
  const int cnt = min(nall, kCap);
  const int32_t cl = S.cols[ic * kCap + hl];
  const float vl = S.vals[ic * kCap + hl];
  int cmax = max(cnt, __shfl_xor(cnt, 32, 64));
  cmax = __builtin_amdgcn_readfirstlane(cmax);
  const float4 acc = conv1_half_entries<kStep>(S, cl, vl, cnt, cmax, f4zero());
  if (live && nall <= kCap) st4_chain(Z1, i * (2 * H) + 4 * hl, acc);   // long rows: their block's
  BT_END(1);
}

// ---------------------------------------------------------------- conv2 forward
// conv2 lin on the sparse path, per work item (<= kChunk nodes of one tree):
//   Z2_d[i] = [keep * 2 relu(H1_d[i]) | kept_d(i, s)] . [W2_d^T[0:64] ; Wr_b]
//   Wr_b[s] = 2 relu(x_root,col_s) W2_d^T[64 + col_s]      (s < nnz(root), else 0)
// i.e. one [nodes x (64 + nnz(root))] x [. x 64] product per item, with the dropout-masked
// relu(H1) and the per-node root keep bits (0/1) generated in registers and the block's B
// operand staged once in LDS.  The root keep masks are stored in S.rbits for the dW2 root
// columns of the backward.
//
// The product runs on the bf16 MFMA in the fp32-grade split form (mfma_x6, bgcn_common.h):
// the f32-input MFMA issues at the FP32 vector rate and bounds this kernel at Weibo /
// 1024-node sizes; the three-product form (~1e-5 relative) flips relu'(H2) for entries
// near zero, hence six.  B is staged transposed and pre-split (hi / mid / lo bf16 [o][k]):
// k < 64 the H1 columns (W2^T rows), k in [64, 96) the root slots (slot 2j + h at
// 64 + 16h + j, value 2 relu(x_root) W2^T[64 + col]).  K order: lane half h owns H1
// columns [32h, 32h + 32) (k-step s: columns 32h + 8s + j) and root slots 2j + h (k-step
// t: slots 2(8t + j) + h), so each lane hashes only its own keep words and the steps past
// the root's non-zeros are skipped; the keep bits are exact in bf16 (three products).
//
// Every wave works on ONE 32-node tile and a block is one (work item, direction): 512
// threads, wave w takes tile w of the item's <= 8 (kChunk = 256 nodes), so no wave runs two
// tiles in series and the B operand - the 24.6 KB split W2 image, the root's 32 slots and
// their W2^T rows, a dependent chain item -> root -> cols -> W2^T - is filled once per item
// and direction, by all 512 threads.  (The half-item form before it, 256-thread blocks of
// four tiles, filled twice for every item over 128 nodes; beside the next batch's pass over
// X those loads are what queues.)  A wave whose tile lies past the item's end computes
// nothing and stays for the spill rounds' barriers.  Each lane loads its H1 A-fragment (row
// r32, columns [32h, 32h + 32) of direction d: eight 16-byte loads, a 128-byte run) straight
// into registers - no LDS staging of H1 (the block's LDS is the B operand only) - and
// requests it after the fill's loads (all twelve 16-byte loads are in flight before the
// fill's barrier).  With 32-bit node indices the wave takes 96 registers, no scratch
// (__launch_bounds__(512, 5)).  What that does NOT buy: a block is two waves per SIMD, 192
// registers, so beside the next batch's pass over X (201 registers a wave) it fits on a CU
// that holds one block of the pass (304 free: one block, as two of the 120-register
// half-item blocks did) and not on one that holds two (96 free).  In the step its blocks
// still start over ~65 us in three rounds of ~20 us (profiles/r07_conv2_blocks.txt); the
// launch is 80 us there either way, 20.5 -> 17.7 us alone.  Fitting beside two blocks of
// the pass needs one wave per SIMD at <= 96 registers (a four-wave block) or 48 a wave.
// Tried a block per whole item with two tiles per wave in series (H1 staged through LDS):
// the kernel was the fill plus two tiles' products on the items of 256 nodes.
// Tried per-tree root images built by extra blocks of conv1's launch (one dependent level
// less in this fill): conv1 alone 15.6 -> 19.5 us for its 2B extra blocks, conv2 unchanged
// (20.6 -> 20.2), the step not faster (profiles/r05_pass_regs_ab.txt and the round-5
// root-image timelines beside it).
constexpr int kC2K = H + kCap;           // B rows: 64 H1 columns + 32 root slot positions
constexpr int kC2Ld16 = kC2K + 8;        // bf16 row stride of the split B (16-byte aligned)
static_assert(kC2Ld16 == kW2sLd, "conv2's B rows are the prologue image's rows");
constexpr int kC2Threads = 512;          // 8 waves: one per 32-node tile of an item
static_assert(kChunk == 32 * (kC2Threads / 64), "a wave per tile of a work item");
__global__ __launch_bounds__(kC2Threads, 5) void k_conv2_item(SparseState S, const float* __restrict__ H1,
                                                              float* __restrict__ Z2, KeepSrc keep) {
  BT_BEGIN
  if (!use_sparse(S)) return;
  const int item = int(blockIdx.x);
  if (item >= S.tree_item0[S.B]) return;
  __shared__ __attribute__((aligned(16))) __bf16 Bs[3][H * kC2Ld16];   // hi, mid, lo
  __shared__ uint32_t rk[kCap];
  const int d = blockIdx.y;
  const int32_t beg = S.item_beg[item], end = S.item_end[item];   // node indices: 32-bit, as stored
  const int wv = threadIdx.x >> 6, l = threadIdx.x & 63, r32 = l & 31, h = l >> 5;
  const int32_t i0 = beg + 32 * wv;
  const int32_t i = i0 + r32;
  const bool ok = i < end;
  const bool live = i0 < end;                        // wave-uniform: the wave has a tile
  const int64_t r = S.item_root[item];
  const float sc = keep.scale();
  const int64_t K2 = S.F + H;
  const float* w2t = S.w2t + int64_t(d) * K2 * H;
  // the fill, once per block: every thread takes three 16-byte pieces of the split W2 image
  // and four outputs of one root slot (unconditional loads from a clamped slot / column,
  // selects after; zero past rn).  All of its loads are requested before the H1 fragment.
  static_assert(3 * H * 8 == 3 * kC2Threads && kCap * (H / 4) == kC2Threads, "one fill round per thread");
  const __bf16* src = S.w2s + int64_t(d) * 3 * H * kW2sLd;
  uint4 im[3];
#pragma unroll
  for (int u = 0; u < 3; ++u) {
    const int e = int(threadIdx.x) + u * kC2Threads;
    const int part = e / (H * 8), o = (e / 8) % H, q = (e % 8) * 8;
    im[u] = *reinterpret_cast<const uint4*>(src + (int64_t(part) * H + o) * kW2sLd + q);
  }
  const int rn_all = S.nnz[r];
  const int rn = min(rn_all, kCap);   // root slots in the ELL (the rest spilled)
  const int fs = int(threadIdx.x) >> 4, fq = (int(threadIdx.x) & 15) * 4;
  const int64_t slot = r * kCap + fs;
  const int32_t fcol_raw = S.cols[slot];
  const float fval = S.vals[slot];
  const float4 fw = ld4(w2t + int64_t(H + min(max(fcol_raw, 0), int32_t(S.F - 1))) * H + fq);
  // this lane's A-fragment rows (clamped: a row past the item reads the item's last row and
  // is masked by `ok`)
  float4 hv[8];
  const float* hsrc = H1 + int64_t(min(i, end - 1)) * (2 * H) + d * H + 32 * h;
#pragma unroll
  for (int u = 0; u < 8; ++u) hv[u] = ld4(hsrc + 4 * u);
#pragma unroll
  for (int u = 0; u < 3; ++u) {
    const int e = int(threadIdx.x) + u * kC2Threads;
    const int part = e / (H * 8), o = (e / 8) % H, q = (e % 8) * 8;
    *reinterpret_cast<uint4*>(&Bs[part][o * kC2Ld16 + q]) = im[u];
  }
  if ((threadIdx.x & 15) == 0) rk[fs] = fs < rn ? uint32_t(H + fcol_raw) : 0u;
  {
    const float av = fs < rn ? sc * fmaxf(fval, 0.f) : 0.f;
    const float vv[4] = {av * fw.x, av * fw.y, av * fw.z, av * fw.w};
    const int k = H + (fs & 1) * (kCap / 2) + (fs >> 1);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int o = (fq + u) * kC2Ld16 + k;
      split3_bf16(vv[u], Bs[0][o], Bs[1][o], Bs[2][o]);
    }
  }
  __syncthreads();
  BT_MARK(2, 0);
  // a wave without a tile (past a short item's end) computes nothing but stays for the
  // spill rounds' barriers
  const uint32_t ni = uint32_t(ok ? i : beg);
  const uint32_t kb = keep.base(ni);
  f32x16 acc0 = {}, acc1 = {};
  if (live) {
    const uint32_t wd = keep.get_b(uint32_t(d), ni, kb, uint32_t(h));
    const float hf[32] = {hv[0].x, hv[0].y, hv[0].z, hv[0].w, hv[1].x, hv[1].y, hv[1].z, hv[1].w,
                          hv[2].x, hv[2].y, hv[2].z, hv[2].w, hv[3].x, hv[3].y, hv[3].z, hv[3].w,
                          hv[4].x, hv[4].y, hv[4].z, hv[4].w, hv[5].x, hv[5].y, hv[5].z, hv[5].w,
                          hv[6].x, hv[6].y, hv[6].z, hv[6].w, hv[7].x, hv[7].y, hv[7].z, hv[7].w};
#pragma unroll
    for (int s = 0; s < 4; ++s) {   // H1 columns 32h + 8s + j
      bf16x8 ah, am, al;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int kk = 8 * s + j;
        const float a = ((wd >> kk) & 1u) ? sc * fmaxf(hf[kk], 0.f) : 0.f;
        __bf16 x, y, z;
        split3_bf16(a, x, y, z);
        ah[j] = x; am[j] = y; al[j] = z;
      }
      const int k = 32 * h + 8 * s;
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        const int o = (32 * hh + r32) * kC2Ld16 + k;
        const bf16x8 bh = *reinterpret_cast<const bf16x8*>(&Bs[0][o]);
        const bf16x8 bm = *reinterpret_cast<const bf16x8*>(&Bs[1][o]);
        const bf16x8 bl = *reinterpret_cast<const bf16x8*>(&Bs[2][o]);
        if (hh == 0) acc0 = mfma_x6(ah, am, al, bh, bm, bl, acc0);
        else acc1 = mfma_x6(ah, am, al, bh, bm, bl, acc1);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  if (wv == 0) BT_MARK(2, 2);
  // the root slots (exact 0/1 keep bits times the staged root rows, three products); a root
  // row over the ELL cap continues from the spill pool in rounds of kCap entries
  const int64_t off = rn_all > kCap ? S.ovf_off[r] : 0;
  const int nsp = rn_all > kCap ? rn_all - kCap : 0;
  for (int c0 = -kCap; c0 < nsp; c0 += kCap) {
    const int cn = c0 < 0 ? rn : min(kCap, nsp - c0);
    if (c0 >= 0) {   // a spill round: the next kCap pool entries into the root slots
      __syncthreads();   // every wave is done with the previous round's slots (all waves loop alike)
      const int tk = min(int(threadIdx.x), kCap - 1);
      const uint2 ek = S.ovf[off + min(c0 + tk, nsp - 1)];
      if (threadIdx.x < kCap) rk[threadIdx.x] = uint32_t(H + min(max(int32_t(ek.x), 0), int32_t(S.F - 1)));
      for (int e = threadIdx.x; e < kCap * (H / 4); e += kC2Threads) {
        const int s = e >> 4, q = (e & 15) * 4;
        const uint2 ent = S.ovf[off + min(c0 + s, nsp - 1)];
        const float4 w = ld4(w2t + int64_t(H + min(max(int32_t(ent.x), 0), int32_t(S.F - 1))) * H + q);
        const float av = s < cn ? sc * fmaxf(__uint_as_float(ent.y), 0.f) : 0.f;
        const float vv[4] = {av * w.x, av * w.y, av * w.z, av * w.w};
        const int k = H + (s & 1) * (kCap / 2) + (s >> 1);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int o = (q + u) * kC2Ld16 + k;
          split3_bf16(vv[u], Bs[0][o], Bs[1][o], Bs[2][o]);
        }
      }
      __syncthreads();
    }
    const int mc = (cn + 1) / 2;
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < kCap / 2; ++j) {
      const int sl = 2 * j + h;
      if (j < mc && sl < cn) {
        const uint32_t k = rk[sl];
        m |= ((keep.get_b(uint32_t(d), ni, kb, k >> 5) >> (k & 31)) & 1u) << sl;
      }
    }
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
      if (live && 8 * tt < mc) {
        bf16x8 ar;
#pragma unroll
        for (int j = 0; j < 8; ++j) ar[j] = __bf16(((m >> (2 * (8 * tt + j) + h)) & 1u) ? 1.f : 0.f);
        const int k = H + (kCap / 2) * h + 8 * tt;
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
          const int o = (32 * hh + r32) * kC2Ld16 + k;
          f32x16 c = hh == 0 ? acc0 : acc1;
          c = mfma_bf16(ar, *reinterpret_cast<const bf16x8*>(&Bs[2][o]), c);
          c = mfma_bf16(ar, *reinterpret_cast<const bf16x8*>(&Bs[1][o]), c);
          c = mfma_bf16(ar, *reinterpret_cast<const bf16x8*>(&Bs[0][o]), c);
          if (hh == 0) acc0 = c; else acc1 = c;
        }
      }
    }
    if (c0 < 0) {   // the ELL slots' keep mask, for the dW2 root columns of the backward
      m |= __shfl_xor(m, 32);
      if (h == 0 && ok) S.rbits[int64_t(d) * S.N + i] = m;
    }
  }
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int32_t ii = i0 + (q & 3) + 8 * (q >> 2) + 4 * h;
    if (ii < end) {
      Z2[int64_t(ii) * (2 * H) + d * H + r32] = acc0[q];
      Z2[int64_t(ii) * (2 * H) + d * H + 32 + r32] = acc1[q];
    }
  }
  BT_END(2);
}

// ---------------------------------------------------------------- tree items
// (items_body: bgcn_items_body.h)
__global__ __launch_bounds__(1024) void k_items(SparseState S, const int32_t* __restrict__ tree_ptr,
                                                const int64_t* __restrict__ rootindex) {
  items_body(S, tree_ptr, rootindex);
}

// ---------------------------------------------------------------- CSC of X
// (the four steps: bgcn_csc_body.h)
__global__ __launch_bounds__(kRowBlock) void k_csc_hist(SparseState S) {
  extern __shared__ __attribute__((aligned(16))) int32_t hsm[];
  csc_hist_body(S, int(blockIdx.x), hsm);
}
__global__ __launch_bounds__(256) void k_csc_prefix(SparseState S, int R) {
  csc_prefix_body(S, R, int(blockIdx.x));
}
__global__ __launch_bounds__(1024) void k_csc_colscan(SparseState S) { csc_colscan_body(S); }
__global__ __launch_bounds__(256) void k_csc_place(SparseState S) {
  extern __shared__ __attribute__((aligned(16))) int32_t psm[];
  csc_place_body(S, int(blockIdx.x), psm);
}

}  // namespace

// ---------------------------------------------------------------- host side
size_t carve_images(Carve& c, int64_t F, WeightImages* im) {
  WeightImages t;
  t.w1t = c.take<float>(size_t(F) * 2 * H);
  t.w2t = c.take<float>(size_t(2) * (F + H) * H);
  t.w2s = c.take<__bf16>(size_t(2) * 3 * H * kW2sLd);
  t.w2d = c.take<__bf16>(size_t(2) * 3 * H * kW2dLd);
  if (im) *im = t;
  return c.off;
}

size_t carve_sparse(Carve& c, int64_t N, int64_t B, int64_t F, SparseState* S) {
  SparseState t{};
  t.N = N;
  t.F = F;
  t.B = B;
  t.max_items = int(N / kChunk + B + 1);
  WeightImages im;
  carve_images(c, F, &im);
  t.w1t = im.w1t; t.w2t = im.w2t; t.w2s = im.w2s; t.w2d = im.w2d;
  t.item_tree = c.take<int32_t>(size_t(t.max_items));
  t.item_beg = c.take<int32_t>(size_t(t.max_items));
  t.item_end = c.take<int32_t>(size_t(t.max_items));
  t.item_root = c.take<int32_t>(size_t(t.max_items));
  t.tree_item0 = c.take<int32_t>(size_t(B + 1));
  t.root_part = c.take<float>(size_t(2) * t.max_items * kCap * H);
  const size_t slots = size_t(N) * kCap;
  const size_t R = size_t((N + kRowBlock - 1) / kRowBlock);
  t.hist = c.take<int32_t>(R * size_t(F));
  t.col_total = c.take<int32_t>(size_t(F));
  t.col_start = c.take<int32_t>(size_t(F));
  t.col_end = c.take<int32_t>(size_t(F));
  t.csc = c.take<uint2>(slots + size_t(N) * kSpillPerRow);
  t.rbits = c.take<uint32_t>(size_t(2) * N);
  t.ovf_off = c.take<int32_t>(size_t(N));   // the per-op encoder's spill pool (a prepared
  t.ovf_cap = N * kSpillPerRow;             // batch brings its own)
  t.ovf = c.take<uint2>(size_t(t.ovf_cap));
  t.long_rows = c.take<int32_t>(size_t(N));
  if (S) {
    t.mode = S->mode;
    t.flags = S->flags;
    t.nnz = S->nnz;
    t.cols = S->cols;
    t.vals = S->vals;
    *S = t;
  }
  return c.off;
}

int sparse_prologue(SparseState& S, const bgcn_bigcn_args* a, int32_t* node_root, hipStream_t s,
                    bool batch_part) {
  const int nTx = int((S.F + H + 31) / 32);
  const int nT = S.mode == 1 ? 0 : nTx * 2 * 4;
  const int nS = nT > 0 ? 2 * kSplitBlocks : 0;
  const int nR = batch_part ? int((S.N + 255) / 256) : 0;
  const int nP = batch_part ? int((S.B + 1 + 255) / 256) : 0;
  const int nZ = (nT + nR + nP == 0 && (S.zero_word || S.rtick)) ? 1 : 0;
  if (nT + nR + nP + nZ == 0) return BGCN_OK;
  hipLaunchKernelGGL(k_prologue, dim3(unsigned(nT + nS + nR + nP + nZ)), dim3(256), 0, s, S, a->td_w1, a->bu_w1,
                     a->td_w2, a->bu_w2, a->batch, a->rootindex, node_root, a->tree_ptr, nTx, nT, nR);
  BGCN_CHECK_LAUNCH();
  return BGCN_OK;
}

int sparse_compact_conv1(SparseState& S, const void* X, int xdt, int64_t ldx, float* Z1,
                         hipStream_t s) {
  if (xdt == BGCN_DTYPE_BF16)
    hipLaunchKernelGGL(k_compact_conv1<bf16_t>, dim3(grid_for(S.N, 4)), dim3(256), 0, s, S,
                       static_cast<const bf16_t*>(X), ldx, Z1);
  else
    hipLaunchKernelGGL(k_compact_conv1<float>, dim3(grid_for(S.N, 4)), dim3(256), 0, s, S,
                       static_cast<const float*>(X), ldx, Z1);
  BGCN_CHECK_LAUNCH();
  return BGCN_OK;
}

int sparse_items(SparseState& S, const int32_t* tree_ptr, const int64_t* rootindex, hipStream_t s) {
  hipLaunchKernelGGL(k_items, dim3(1), dim3(1024), 0, s, S, tree_ptr, rootindex);
  BGCN_CHECK_LAUNCH();
  return BGCN_OK;
}

int sparse_conv2(SparseState& S, const float* H1, float* Z2, KeepSrc keep, hipStream_t s) {
  hipLaunchKernelGGL(k_conv2_item, dim3(unsigned(S.max_items), 2), dim3(kC2Threads), 0, s, S, H1, Z2, keep);
  BGCN_CHECK_LAUNCH();
  return BGCN_OK;
}

int sparse_csc(SparseState& S, hipStream_t s) {
  const int R = int((S.N + kRowBlock - 1) / kRowBlock);
  hipLaunchKernelGGL(k_csc_hist, dim3(unsigned(R)), dim3(kRowBlock), size_t(S.F) * sizeof(int32_t), s, S);
  BGCN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_csc_prefix, dim3(grid_for(S.F, kPrefixCols)), dim3(256), 0, s, S, R);
  BGCN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_csc_colscan, dim3(1), dim3(1024), 0, s, S);
  BGCN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_csc_place, dim3(unsigned(R)), dim3(256), size_t(2 * S.F) * sizeof(int32_t), s, S);
  BGCN_CHECK_LAUNCH();
  return BGCN_OK;
}

int sparse_conv1_gather(SparseState& S, float* Z1, hipStream_t s) {
  hipLaunchKernelGGL(k_conv1_rows2<4>, dim3(kLongRowBlocks + grid_for(S.N, 8)), dim3(256), 0, s, S, Z1);
  BGCN_CHECK_LAUNCH();
  return BGCN_OK;
}

}  // namespace bgcn

extern "C" size_t bgcn_weight_images_size(int64_t in_feats) {
  if (in_feats <= 0) return 0;
  bgcn::Carve c(nullptr, 0);
  return bgcn::carve_images(c, in_feats, nullptr) + 256;
}

BT_READER(sparse)

extern "C" int bgcn_csr_to_dense(const int32_t* x_row_ptr, const int32_t* x_col, const float* x_val,
                                 int64_t num_nodes, int64_t in_feats, void* x, int64_t ldx, int32_t x_dtype,
                                 int32_t* status, bgcn_stream_t stream) {
  using namespace bgcn;
  BGCN_CHECK_ARG(num_nodes > 0 && in_feats > 0 && in_feats % 4 == 0 && ldx >= in_feats && ldx % 4 == 0,
                 "bad sizes (in_feats and ldx: multiples of 4)");
  BGCN_CHECK_ARG(x_row_ptr && x_col && x_val && x, "null pointer");
  BGCN_CHECK_ARG((reinterpret_cast<uintptr_t>(x) & 15) == 0, "x must be 16-byte aligned");
  BGCN_CHECK_ARG(x_dtype == BGCN_DTYPE_F32 || x_dtype == BGCN_DTYPE_BF16, "bad x_dtype");
  BGCN_CHECK_ARG(in_feats <= 8192, "in_feats > 8192 (the row is assembled in LDS)");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const size_t smem = size_t(2) * size_t((in_feats + 3) / 4 * 4) * sizeof(float);   // two waves' rows
  const dim3 grid(unsigned(std::min<int64_t>((num_nodes + 1) / 2, 8192)));
  if (x_dtype == BGCN_DTYPE_BF16)
    hipLaunchKernelGGL(k_csr_dense<bf16_t>, grid, dim3(128), smem, s, x_row_ptr, x_col, x_val, num_nodes, in_feats,
                       static_cast<bf16_t*>(x), ldx, status);
  else
    hipLaunchKernelGGL(k_csr_dense<float>, grid, dim3(128), smem, s, x_row_ptr, x_col, x_val, num_nodes, in_feats,
                       static_cast<float*>(x), ldx, status);
  BGCN_CHECK_LAUNCH();
  return BGCN_OK;
}
