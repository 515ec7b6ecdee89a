// Device bodies of the CSC of X (the stable counting sort of its non-zeros by column).
// Shared by the per-op encoder's four launches (k_csc_*, bgcn_sparse.hip) and the batch
// preparation, which runs them as roles of merged launches (k_prep_c .. k_prep_f,
// bgcn_prep.hip).
#pragma once

#include "bgcn_internal.h"
#include "bgcn_sparse.h"

namespace bgcn {

// ---------------------------------------------------------------- CSC of X
// Stable counting sort of the non-zeros by column (rows stay in order inside a column):
//   k_csc_hist     per row block (kRowBlock rows, a thread per row): column histogram
//                  in LDS -> hist[r][c]
//   k_csc_prefix   per column: exclusive prefix over the row blocks, column totals
//   k_csc_colscan  one block: column starts/ends = exclusive scan of the totals
//   k_csc_place    per row block: start + the block's prefix, then the rows in order,
//                  32 at a time, rank inside the batch from per-column row bitmasks
// No float atomics, no general sort; deterministic.  Every global load is issued
// unconditionally (clamped index, select afterwards) so the loads of a thread overlap.
// (bodies: kRowBlock threads; hsm / psm = the launch's dynamic shared memory)
// Spilled entries of a group of rows, flattened over the block's threads: pre[r] = the
// group's entries before row r (pre[nrows] = total), off[r] = row r's first pool entry.
// f(r, entry) runs for every entry with four pool loads in flight per thread (a row's
// entries walked by one thread were a serial chain of dependent loads: a 270-word row
// cost the placement ~300 us).
__device__ __forceinline__ int spill_row_of(const int* pre, int nrows, int e) {
  int lo = 0, hi = nrows - 1;   // the last row r with pre[r] <= e (rows of no entries skipped)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (pre[mid] <= e) lo = mid; else hi = mid - 1;
  }
  return lo;
}
template <class Fn>
__device__ __forceinline__ void for_spill(const SparseState& S, const int* pre, const int* off, int nrows,
                                          Fn f) {
  const int total = pre[nrows];
  for (int e0 = int(threadIdx.x); e0 < total; e0 += 4 * int(blockDim.x)) {
    int r[4];
    uint2 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = min(e0 + u * int(blockDim.x), total - 1);
      r[u] = spill_row_of(pre, nrows, e);
      v[u] = S.ovf[off[r[u]] + (e - pre[r[u]])];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (e0 + u * int(blockDim.x) < total) f(r[u], v[u]);
  }
}

__device__ inline void csc_hist_body(const SparseState& S, int bid, int32_t* hsm) {   // hsm [F]
  if (!use_sparse(S)) return;
  for (int64_t c = threadIdx.x; c < S.F; c += kRowBlock) hsm[c] = 0;
  const int64_t i = int64_t(bid) * kRowBlock + threadIdx.x;
  const int64_t ic = min<int64_t>(i, S.N - 1);
  const int nall = i < S.N ? S.nnz[ic] : 0;
  const int n = min(nall, kCap);
  int32_t cl[kCap];
#pragma unroll
  for (int q = 0; q < kCap / 4; ++q) {
    const int4 v = *reinterpret_cast<const int4*>(S.cols + ic * kCap + 4 * q);
    cl[4 * q] = v.x; cl[4 * q + 1] = v.y; cl[4 * q + 2] = v.z; cl[4 * q + 3] = v.w;
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < kCap; ++s)
    if (s < n) atomicAdd(&hsm[cl[s]], 1);
  const int nsp = nall > kCap ? nall - kCap : 0;
  if (__syncthreads_or(nsp)) {   // the block's long rows (rare): their spilled entries
    __shared__ int pre[kRowBlock + 1], off[kRowBlock], wsum[kRowBlock / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int x = nsp;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(x, o, 64);
      if (lane >= o) x += y;
    }
    if (lane == 63) wsum[wv] = x;
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kRowBlock / 64; ++w) {
      base += w < wv ? wsum[w] : 0;
      total += wsum[w];
    }
    pre[threadIdx.x] = base + x - nsp;
    off[threadIdx.x] = nsp ? S.ovf_off[ic] : 0;
    if (threadIdx.x == 0) pre[kRowBlock] = total;
    __syncthreads();
    for_spill(S, pre, off, kRowBlock, [&](int, uint2 v) { atomicAdd(&hsm[v.x], 1); });
  }
  __syncthreads();
  int32_t* out = S.hist + int64_t(bid) * S.F;
  for (int64_t c = threadIdx.x; c < S.F; c += kRowBlock) out[c] = hsm[c];
}

// 64 columns x 4 row-block quarters per block; hist[r][c] becomes the exclusive prefix
// of column c over row blocks < r.  Loads in groups of 8 (independent).
// per column: exclusive prefix of the row-block counts.  A 256-thread block takes
// kPrefixCols columns x kPrefixSegs segments of the row blocks (each segment summed, then
// rewritten as prefixes, eight loads in flight); the segment totals are combined in
// segment order.  16 x 16: a Weibo / 1024-node batch has 370-460 row blocks, and with 4
// segments of a column per thread the two passes took ~30 dependent load rounds.
constexpr int kPrefixCols = 16, kPrefixSegs = 256 / kPrefixCols;
__device__ inline void csc_prefix_body(const SparseState& S, int R, int bid) {
  if (!use_sparse(S)) return;
  __shared__ int32_t part[kPrefixSegs][kPrefixCols];
  const int cl = threadIdx.x % kPrefixCols, q = threadIdx.x / kPrefixCols;
  const int64_t c = min<int64_t>(int64_t(bid) * kPrefixCols + cl, S.F - 1);
  const bool live = int64_t(bid) * kPrefixCols + cl < S.F;
  const int rq = (R + kPrefixSegs - 1) / kPrefixSegs, rb = q * rq, re = min(R, rb + rq);
  int32_t sum = 0;
  for (int r0 = rb; r0 < re; r0 += 8) {
    int32_t v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = S.hist[int64_t(max(min(r0 + u, re - 1), 0)) * S.F + c];
#pragma unroll
    for (int u = 0; u < 8; ++u) sum += r0 + u < re ? v[u] : 0;
  }
  part[q][cl] = sum;
  __syncthreads();
  int32_t run = 0;
  for (int qq = 0; qq < q; ++qq) run += part[qq][cl];
  for (int r0 = rb; r0 < re; r0 += 8) {
    int32_t v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = S.hist[int64_t(max(min(r0 + u, re - 1), 0)) * S.F + c];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (live && r0 + u < re) S.hist[int64_t(r0 + u) * S.F + c] = run;
      run += r0 + u < re ? v[u] : 0;
    }
  }
  if (live && q == kPrefixSegs - 1) S.col_total[c] = run;
}

// column starts: exclusive scan of col_total, one 1024-thread block (thread = run of
// consecutive columns, block scan of the run sums)
// (body: any block size >= 256)
__device__ inline void csc_colscan_body(const SparseState& S) {
  if (!use_sparse(S)) return;
  __shared__ int32_t wsum[1024];
  const int64_t F = S.F;
  const int nth = int(blockDim.x);
  const int64_t per = (F + nth - 1) / nth;
  const int64_t c0 = threadIdx.x * per;
  constexpr int kMaxPer = kSparseMaxF / 256;
  int32_t v[kMaxPer];
  int32_t local = 0;
#pragma unroll
  for (int k = 0; k < kMaxPer; ++k) {
    const int64_t c = c0 + k;
    v[k] = (k < per && c < F) ? S.col_total[min<int64_t>(c, F - 1)] : 0;
    local += v[k];
  }
  wsum[threadIdx.x] = local;
  __syncthreads();
  for (int o = 1; o < nth; o <<= 1) {
    const int32_t t = threadIdx.x >= o ? wsum[threadIdx.x - o] : 0;
    __syncthreads();
    wsum[threadIdx.x] += t;
    __syncthreads();
  }
  int32_t run = wsum[threadIdx.x] - local;
#pragma unroll
  for (int k = 0; k < kMaxPer; ++k) {
    const int64_t c = c0 + k;
    if (k < per && c < F) {
      S.col_start[c] = run;
      S.col_end[c] = run + v[k];
    }
    run += v[k];
  }
}


// Row block of a placement block: the blocks of one XCD (block ids equal mod 8 - the
// dispatcher hands blocks to the XCDs round-robin) take consecutive row blocks, whose
// entries of a column are adjacent in the CSC, so a line of it is mostly written from one
// XCD's L2 instead of from all eight (the placement's stores are scattered by column).
__device__ inline void csc_place_body(const SparseState& S, int bid, int32_t* psm) {
  if (!use_sparse(S)) return;   // psm: [F] counters, [F] row masks
  bid = xcd_contig(bid, int((S.N + kRowBlock - 1) / kRowBlock));
  int32_t* cnt = psm;
  uint32_t* rows = reinterpret_cast<uint32_t*>(psm + S.F);
  const int64_t F = S.F;
  const int32_t* pre = S.hist + int64_t(bid) * F;
  for (int64_t c0 = threadIdx.x; c0 < F; c0 += 4 * 256) {
    int32_t st[4], pr[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t c = min<int64_t>(c0 + 256 * u, F - 1);
      st[u] = S.col_start[c];
      pr[u] = pre[c];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t c = c0 + 256 * u;
      if (c < F) {
        cnt[c] = st[u] + pr[u];
        rows[c] = 0u;
      }
    }
  }
  // all of the block's entries up front: thread t holds entries t + 256k (k < 32) of
  // the row block = slot t % 32 of rows (t / 32) + 8k
  const int64_t r0 = int64_t(bid) * kRowBlock;
  const int s = threadIdx.x % kCap;
  constexpr int kPer = kRowBlock * kCap / 256;   // 32
  int32_t col[kPer], nn[kPer];
  float val[kPer];
  uint32_t rootbits = 0u;   // bit k: row of entry k is a tree root
#pragma unroll
  for (int k = 0; k < kPer; ++k) {   // issue all loads first ...
    const int64_t ic = min<int64_t>(r0 + threadIdx.x / kCap + 8 * k, S.N - 1);
    nn[k] = S.nnz[ic];
    col[k] = S.cols[ic * kCap + s];
    val[k] = S.vals[ic * kCap + s];
    rootbits |= uint32_t(S.root_map[ic] == int32_t(ic)) << k;
  }
  uint32_t smask = 0u;   // bit bt: batch bt (rows 32bt .. 32bt + 31) holds a long row
#pragma unroll
  for (int k = 0; k < kPer; ++k) {   // ... then mask the padding slots
    const int64_t i = r0 + threadIdx.x / kCap + 8 * k;
    col[k] = (i < S.N && s < nn[k]) ? col[k] : -1;
    smask |= (i < S.N && nn[k] > kCap) ? (1u << (k / 4)) : 0u;
  }
  // The block's long rows (rare): their spilled entries are indexed once for the whole
  // block - rpre[t] = the block's spilled entries before row t (a block-wide scan), rslot /
  // roff per row - and staged in LDS (up to kPlaceStage of them; beyond, read from the pool
  // in place), so a batch's passes over them need no dependent global loads.
  constexpr int kPlaceStage = 1024;
  __shared__ int rpre[kRowBlock + 1], roff[kRowBlock], wsum[kRowBlock / 64];
  __shared__ uint32_t rslot[kRowBlock];
  __shared__ uint2 sbuf[kPlaceStage];
  __shared__ uint32_t smask_s;
  if (threadIdx.x == 0) smask_s = 0u;
  __syncthreads();
  if (smask) atomicOr(&smask_s, smask);
  __syncthreads();
  smask = smask_s;
  bool staged = true;
  if (smask) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int64_t i = r0 + t;
    const int na = i < S.N ? S.nnz[i] : 0;
    const int nsp = na > kCap ? na - kCap : 0;
    const int o = nsp ? S.ovf_off[i] : 0;
    const uint32_t sl = nsp ? (uint32_t(i * kCap) | kCscSpillFlag | (S.root_map[i] == int32_t(i) ? kCscRootFlag : 0u))
                            : 0u;
    int x = nsp;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int y = __shfl_up(x, d, 64);
      if (lane >= d) x += y;
    }
    if (lane == 63) wsum[wv] = x;
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kRowBlock / 64; ++w) {
      base += w < wv ? wsum[w] : 0;
      total += wsum[w];
    }
    rpre[t] = base + x - nsp;
    roff[t] = o;
    rslot[t] = sl;
    if (t == 0) rpre[kRowBlock] = total;
    staged = total <= kPlaceStage;
    __syncthreads();
    if (staged) {
      for (int e0 = t; e0 < total; e0 += 4 * kRowBlock) {   // four pool loads in flight
        uint2 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int e = min(e0 + u * kRowBlock, total - 1);
          const int r = spill_row_of(rpre, kRowBlock, e);
          v[u] = S.ovf[roff[r] + (e - rpre[r])];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (e0 + u * kRowBlock < total) sbuf[e0 + u * kRowBlock] = v[u];
      }
    }
    __syncthreads();
  }
  // f(row within the batch, entry, block row) for every spilled entry of batch bt
  auto batch_spill = [&](int bt, auto f) {
    const int lo0 = bt * 32, e1 = rpre[lo0 + 32];
    for (int e = rpre[lo0] + int(threadIdx.x); e < e1; e += int(blockDim.x)) {
      int lo = lo0, hi = lo0 + 31;   // the last row with rpre <= e
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rpre[mid] <= e) lo = mid; else hi = mid - 1;
      }
      const uint2 v = staged ? sbuf[e] : S.ovf[roff[lo] + (e - rpre[lo])];
      f(lo - lo0, v, lo);
    }
  };
  // rows of the block in order, 32 rows (= 1024 slots, 4 per thread) per batch.  The
  // columns of one row are distinct, so an entry's rank among the batch's entries of
  // its column = the number of earlier batch rows holding that column: an OR of row
  // bits per column (order-independent) + popcount.
  constexpr int kBatchRows = 32;
#pragma unroll
  for (int bt = 0; bt < kRowBlock / kBatchRows; ++bt) {
    int rr[4], rank[4];
    const bool spill = (smask >> bt) & 1u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      rr[k] = threadIdx.x / kCap + 8 * k;   // row within the batch
      const int32_t cc = col[4 * bt + k];
      if (cc >= 0) atomicOr(&rows[cc], 1u << rr[k]);
    }
    // spilled entries of the batch's rows (their columns are distinct from the row's ELL
    // columns, so the same row-bit ranks hold), flattened over the block's threads
    if (spill) batch_spill(bt, [&](int r, uint2 v, int) { atomicOr(&rows[v.x], 1u << r); });
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int32_t cc = col[4 * bt + k];
      rank[k] = -1;
      if (cc >= 0) {
        const uint32_t m = rows[cc];
        rank[k] = __popc(m & ((1u << rr[k]) - 1u));
        const int64_t i = r0 + bt * kBatchRows + rr[k];
        const uint32_t flag = ((rootbits >> (4 * bt + k)) & 1u) ? kCscRootFlag : 0u;
        S.csc[cnt[cc] + rank[k]] = make_uint2(uint32_t(i * kCap + s) | flag, __float_as_uint(val[4 * bt + k]));
      }
    }
    if (spill)
      batch_spill(bt, [&](int r, uint2 v, int br) {
        S.csc[cnt[v.x] + __popc(rows[v.x] & ((1u << r) - 1u))] = make_uint2(rslot[br], v.y);
      });
    __syncthreads();
    if (!spill) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int32_t cc = col[4 * bt + k];
        if (rank[k] == 0) {   // the batch's first entry of a column advances its counter
          cnt[cc] += __popc(rows[cc]);
          rows[cc] = 0u;
        }
      }
    } else {   // two phases: the counters (row bits read-only), then the clears
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (rank[k] == 0) cnt[col[4 * bt + k]] += __popc(rows[col[4 * bt + k]]);
      batch_spill(bt, [&](int r, uint2 v, int) {
        if ((rows[v.x] & ((1u << r) - 1u)) == 0u) cnt[v.x] += __popc(rows[v.x]);
      });
      __syncthreads();
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (rank[k] >= 0) rows[col[4 * bt + k]] = 0u;
      batch_spill(bt, [&](int, uint2 v, int) { rows[v.x] = 0u; });
    }
    __syncthreads();
  }
}

}  // namespace bgcn
