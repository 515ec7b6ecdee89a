// Device bodies of the pass over X: a dense row -> its ELL list and spill-pool entries
// (+ conv1), and the same lists from host-fed compacted rows.  Shared by the per-op
// encoder's forward (k_compact_conv1, bgcn_sparse.hip) and the batch preparation
// (k_prep_b, bgcn_prep.hip).
#pragma once

#include "bgcn_bwd.h"
#include "bgcn_internal.h"
#include "bgcn_sparse.h"

namespace bgcn {

// ---------------------------------------------------------------- X compaction + conv1
// One wave per row.  The whole row is requested up front (16-byte pieces per lane:
// 20 KiB of a 5000-wide row in flight per wave) so HBM sees deep, independent streams;
// then the non-zeros are compacted in ascending column order - a 16-byte piece that is
// all zero across the wave (the common case for bag-of-words rows) costs one ballot -
// and Z1[i] = sum val * W1T[col] with each lane owning 2 of the 128 outputs.
constexpr int kRowChunks = 20;  // float4 per lane per pass (F <= 5120 in one pass)

// Z1[i] += sum_s val_s * W1T[col_s] for the (col, val) pairs of lane-held lists: lane s
// (< cnt) holds pair s; the pairs reach the wave by scalar readlane, gathers unconditional
// (clamped column), 8 in flight.
__device__ __forceinline__ float2 conv1_row(const SparseState& S, int cnt, int32_t col_l, float val_l) {
  const int lane = threadIdx.x & 63;
  float2 acc = make_float2(0.f, 0.f);
  for (int s0 = 0; s0 < cnt; s0 += 8) {
    float2 w[8];
    float x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int sl = s0 + u < cnt ? s0 + u : 0;                // wave-uniform
      const int32_t c = min(max(__builtin_amdgcn_readlane(col_l, sl), 0), int32_t(S.F - 1));
      x[u] = s0 + u < cnt ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(val_l), sl)) : 0.f;
      w[u] = *reinterpret_cast<const float2*>(S.w1t + int64_t(c) * (2 * H) + 2 * lane);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      acc.x = fmaf(x[u], w[u].x, acc.x);
      acc.y = fmaf(x[u], w[u].y, acc.y);
    }
  }
  return acc;
}

// Row i of X -> its ELL list (+ conv1).  r: the row's 16-byte chunks (row_chunks<TX>()
// per lane: the whole row, F <= kSparseMaxF), already in flight.
static_assert(kRowChunks * 64 * 4 >= kSparseMaxF, "one pass per row");
template <class TX> constexpr int row_chunks() { return kRowChunks * 4 / XChunk<TX>::kElems; }
// Two ways to place a row's non-zeros in ascending column order.  Per element: a ballot
// per element position of the 16-byte piece, every lane counting the set lanes below it
// (E ballots per piece).  By prefix: each lane's non-zero mask, then the exclusive prefix
// of the per-lane counts - one ballot when no lane holds two non-zeros (the common case
// for bag-of-words rows), else by the counts' bit planes - and a loop over the lane's own
// non-zeros.  The prefix form halves the kernel's registers (205 -> 126-138) and moves bf16
// X at 5.9 instead of 4.3 TB/s alone on the GPU (a bf16 piece holds 8 elements: 8 ballots
// per piece).  Beside the training chain the faster pass costs the chain more: fp32 keeps
// the per-element form (twitter15 0.289 vs 0.298-0.316 ms per step), bf16 takes the
// prefix form paced at one block per CU (weibo_bf16 0.646 vs 0.669 ms, synth1024_bf16
// 0.793 vs 0.811: profiles/r02_compact_ab.txt).  BGCN_COMPACT_PREFIX: 1 bf16 only, 2 both.
#ifndef BGCN_COMPACT_PREFIX
#define BGCN_COMPACT_PREFIX 1
#endif
template <class TX> constexpr bool compact_by_prefix() {
  return BGCN_COMPACT_PREFIX >= 2 || (BGCN_COMPACT_PREFIX == 1 && sizeof(TX) == 2);
}
// Walk a row's non-zeros in ascending column order: emit(pos, col, val) for each, pos =
// its rank in the row (lanes below a lane contribute all their non-zeros first); returns
// the row's count (wave-uniform).
template <class TX, class Emit>
__device__ __forceinline__ int walk_row(const u32x4* r, Emit emit) {
  typedef XChunk<TX> XC;
  constexpr int E = XC::kElems;
  const int lane = threadIdx.x & 63;
  const uint64_t lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  int cnt = 0;
  if constexpr (!compact_by_prefix<TX>()) {
#pragma unroll
  for (int u = 0; u < row_chunks<TX>(); ++u) {
    const u32x4 ru = r[u];                           // past the row: 0 (range-checked load)
    if (__ballot(XC::any(ru)) == 0ull) continue;     // wave-uniform skip
    int pos = cnt;
#pragma unroll
    for (int c = 0; c < E; ++c) {
      const uint64_t m = __ballot(XC::nz(ru, c));
      pos += __popcll(m & lt);
      cnt += __popcll(m);
    }
    const int col0 = (u * 64 + lane) * E;
#pragma unroll
    for (int c = 0; c < E; ++c) {
      if (XC::nz(ru, c)) {
        emit(pos, col0 + c, XC::elem(ru, c));
        ++pos;
      }
    }
  }
  } else {
#pragma unroll
  for (int u = 0; u < row_chunks<TX>(); ++u) {
    const u32x4 ru = r[u];                           // past the row: 0 (range-checked load)
    uint32_t mb = 0;                                 // this lane's non-zero elements
#pragma unroll
    for (int c = 0; c < E; ++c) mb |= uint32_t(XC::nz(ru, c)) << c;
    const uint64_t any = __ballot(mb != 0u);
    if (any == 0ull) continue;                       // wave-uniform skip
    // the exclusive prefix of the per-lane counts, one ballot when no lane holds two (the
    // common case for bag-of-words rows), else by the counts' bit planes
    const int n = __popc(mb);
    int pos = cnt;
    if (__ballot(n > 1) == 0ull) {
      pos += __popcll(any & lt);
      cnt += __popcll(any);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {                  // n <= 8
        const uint64_t bk = __ballot((n >> k) & 1);
        pos += __popcll(bk & lt) << k;
        cnt += __popcll(bk) << k;
      }
    }
    const int col0 = (u * 64 + lane) * E;
    while (mb) {
      const int c = __builtin_ctz(mb);
      mb &= mb - 1u;
      emit(pos, col0 + c, XC::elem(ru, c));
      ++pos;
    }
  }
  }
  return cnt;
}

// The entries past kCap of a long row -> dst[pos] (pos >= kCap), in column order.  The row
// is loaded again one 16-byte piece per lane at a time in a rolled loop: the rare branch
// must not add registers to the pass over X (an unrolled second walk took the fp32 form
// from 205 to 256 + AGPRs, half its occupancy).
template <class TX>
__device__ void spill_walk(__amdgpu_buffer_rsrc_t rs, uint2* dst) {
  typedef XChunk<TX> XC;
  constexpr int E = XC::kElems;
  const int lane = threadIdx.x & 63;
  const uint64_t lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  int cnt = 0;
  constexpr int kG = 5;                              // pieces in flight
  static_assert(row_chunks<TX>() % kG == 0, "spill walk groups");
#pragma unroll 1
  for (int u0 = 0; u0 < row_chunks<TX>(); u0 += kG) {
  u32x4 rg[kG];
#pragma unroll
  for (int v = 0; v < kG; ++v)
    rg[v] = __builtin_amdgcn_raw_buffer_load_b128(rs, ((u0 + v) * 64 + lane) * 16, 0, kAuxNT);
#pragma unroll
  for (int v = 0; v < kG; ++v) {
    const int u = u0 + v;
    const u32x4 ru = rg[v];
    uint32_t mb = 0;
#pragma unroll
    for (int c = 0; c < E; ++c) mb |= uint32_t(XC::nz(ru, c)) << c;
    const int n = __popc(mb);
    int pos = cnt;
#pragma unroll
    for (int k = 0; k < 4; ++k) {                    // n <= 8
      const uint64_t bk = __ballot((n >> k) & 1);
      pos += __popcll(bk & lt) << k;
      cnt += __popcll(bk) << k;
    }
    const int col0 = (u * 64 + lane) * E;
    while (mb) {
      const int c = __builtin_ctz(mb);
      mb &= mb - 1u;
      if (pos >= kCap) dst[pos] = make_uint2(uint32_t(col0 + c), __float_as_uint(XC::elem(ru, c)));
      ++pos;
    }
  }
  }
}

// Row i of X -> its ELL list, the entries past kCap to the spill pool (+ conv1 over both).
template <bool kConv1, class TX>
__device__ __forceinline__ void compact_row(const SparseState& S, int64_t i, const u32x4* r,
                                            __amdgpu_buffer_rsrc_t rs, int32_t* s_col, float* s_val,
                                            float* __restrict__ Z1) {
  const int lane = threadIdx.x & 63;
  const int cnt = walk_row<TX>(r, [&](int pos, int col, float v) {
    if (pos < kCap) {
      s_col[pos] = col;
      s_val[pos] = v;
    }
  });
  if (lane == 0) S.nnz[i] = cnt;
  const int nov = cnt > kCap ? cnt - kCap : 0;       // wave-uniform
  int off = 0;
  if (nov > 0) {
    // a row of more words than the ELL holds (the reference caps none, getTwittergraph.py:
    // 16-24): its tail goes to the batch's spill pool, in column order
    int o = 0;
    if (lane == 0) o = atomicAdd(&S.flags[1], nov);
    o = __builtin_amdgcn_readfirstlane(o);
    if (o < 0 || int64_t(o) + nov > S.ovf_cap) {     // pool full: the batch goes dense
      if (lane == 0) atomicOr(&S.flags[0], 1);
      return;
    }
    if (lane == 0) {
      S.ovf_off[i] = o;
      S.long_rows[atomicAdd(&S.flags[2], 1)] = int32_t(i);   // conv1's long-row blocks
    }
    uint2* dst = S.ovf + o - kCap;
    spill_walk<TX>(rs, dst);
    off = o;
  }
  const int ce = cnt < kCap ? cnt : kCap;
  __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): this wave's LDS writes have landed
  __builtin_amdgcn_wave_barrier();
  const int32_t col_l = lane < ce ? s_col[lane] : 0;
  const float val_l = lane < ce ? s_val[lane] : 0.f;
  if (lane < ce) {
    S.cols[i * kCap + lane] = col_l;
    S.vals[i * kCap + lane] = val_l;
  }
  if (kConv1) {
    float2 acc = conv1_row(S, ce, col_l, val_l);
    if (nov > 0) {   // the spilled entries, 64 at a time (this wave's own stores, read back)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      for (int k0 = 0; k0 < nov; k0 += 64) {
        const int n = min(64, nov - k0);
        const uint2 e = S.ovf[off + k0 + min(lane, n - 1)];
        const float2 p = conv1_row(S, n, int32_t(e.x), __uint_as_float(e.y));
        acc.x += p.x;
        acc.y += p.y;
      }
    }
    *reinterpret_cast<float2*>(Z1 + i * (2 * H) + 2 * lane) = acc;
  }
}

// kConv1 = true: compaction + conv1 in one pass (the encoder's forward); false: the ELL
// only (weight-independent batch preparation, bgcn_prepare_batch).  A wave keeps ~20 KB
// of X in flight: one fp32 row, or two bf16 rows (their loads issued together).
// Body: block bid of nblk 256-thread blocks (grid-stride over rows).
template <bool kConv1, class TX>
__device__ inline void compact_body(const SparseState& S, const TX* __restrict__ X, int64_t ldx,
                                    float* __restrict__ Z1, int bid, int nblk) {
  constexpr int kRows = sizeof(TX) == 2 ? 2 : 1;
  __shared__ int32_t s_col[4][kCap];
  __shared__ float s_val[4][kCap];
  if (S.mode == 1) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // grid-stride over rows (the preparation's grid covers every row once: one fp32 row or
  // two bf16 rows per wave; a capped grid strides)
  const int64_t stride = int64_t(nblk) * 4;
  for (int64_t i0 = int64_t(bid) * 4 + wave; i0 < S.N; i0 += stride * kRows) {
    u32x4 r[kRows][row_chunks<TX>()];
    __amdgpu_buffer_rsrc_t rs[kRows];
#pragma unroll
    for (int k = 0; k < kRows; ++k) {   // all loads in flight; a row past N reads nothing
      const int64_t ik = i0 + k * stride;
      rs[k] = row_rsrc(X + min<int64_t>(ik, S.N - 1) * ldx, ik < S.N ? uint32_t(S.F * sizeof(TX)) : 0u);
#pragma unroll
      for (int u = 0; u < row_chunks<TX>(); ++u)
        r[k][u] = __builtin_amdgcn_raw_buffer_load_b128(rs[k], (u * 64 + lane) * 16, 0, kAuxNT);
    }
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
      const int64_t i = i0 + k * stride;
      if (i < S.N) compact_row<kConv1, TX>(S, i, r[k], rs[k], s_col[wave], s_val[wave], Z1);
    }
  }
}

// The host-fed input form (bgcn_batch.x_row_ptr / x_col / x_val): the rows arrive already
// compacted, in ascending column order, so the ELL list, the spill pool and the long-row
// list are filled from them with the contents compact_row writes from the dense row (the
// step computes the same bits either way).  One 32-lane half-wave per row (a BoW row holds
// ~12 entries), grid-stride; reads nnz x 8 bytes instead of N x F x 4.  The lists come
// from the host, so every row is checked first: a negative start or count, a column
// outside [0, F) or columns not strictly ascending set the batch status bit 0 (the step
// is then rejected like a bad edge index) and the row is written empty, so no later
// kernel indexes by a bad column.
__device__ inline void csr_ell_body(const SparseState& S, const int32_t* __restrict__ rp,
                                    const int32_t* __restrict__ rc, const float* __restrict__ rv, int bid,
                                    int nblk) {
  if (S.mode == 1) return;
  const int lane = threadIdx.x & 31;
  const int half = threadIdx.x & 32;
  const int64_t nhalf = int64_t(nblk) * (blockDim.x / 32);
  for (int64_t i = (int64_t(bid) * blockDim.x + threadIdx.x) / 32; i < S.N; i += nhalf) {
    const int32_t b = rp[i], cnt = rp[i + 1] - b;      // half-wave uniform
    bool bad = b < 0 || cnt < 0;
    int32_t c0 = 0;
    float v0 = 0.f;
    if (!bad) {
      bool lbad = false;
      int32_t prev = -1;
      for (int k0 = 0; k0 < cnt; k0 += 32) {
        const int k = k0 + lane;
        const int32_t c = rc[b + min(k, cnt - 1)];
        if (k0 == 0) {
          c0 = c;
          v0 = rv[b + min(k, cnt - 1)];
        }
        int32_t pc = __shfl_up(c, 1, 32);
        if (lane == 0) pc = prev;
        lbad = lbad || (k < cnt && (c < 0 || c >= S.F || c <= pc));
        prev = __shfl(c, 31, 32);                      // (a later chunk exists only if this one is full)
      }
      bad = ((__ballot(lbad) >> half) & 0xffffffffull) != 0ull;
    }
    if (bad) {
      if (lane == 0) {
        S.nnz[i] = 0;
        if (S.bstatus) atomicOr(S.bstatus, 1);
      }
      continue;
    }
    const int ce = cnt < kCap ? cnt : kCap;
    if (lane < ce) {
      S.cols[i * kCap + lane] = c0;
      S.vals[i * kCap + lane] = v0;
    }
    if (lane == 0) S.nnz[i] = cnt;
    if (cnt > kCap) {   // a long row: its tail to the spill pool, as compact_row does
      const int nov = cnt - kCap;
      int o = 0;
      if (lane == 0) o = atomicAdd(&S.flags[1], nov);
      o = __shfl(o, 0, 32);
      if (o < 0 || int64_t(o) + nov > S.ovf_cap) {     // pool full: results invalid (status bit 2)
        if (lane == 0) atomicOr(&S.flags[0], 1);
        continue;
      }
      if (lane == 0) {
        S.ovf_off[i] = o;
        S.long_rows[atomicAdd(&S.flags[2], 1)] = int32_t(i);
      }
      for (int k = lane; k < nov; k += 32)
        S.ovf[o + k] = make_uint2(uint32_t(rc[b + kCap + k]), __float_as_uint(rv[b + kCap + k]));
    }
  }
}

}  // namespace bgcn
