// The analysis side of the reference (explain_PHEME.py:91-242, :530-533): after every stage of a
// direction each node's activation row is reduced to one number, and all nodes of a tree are
// ranked by it (torch.topk with k = n: a full descending sort).  Inference only.
//
// bgcn_explain_sums - every per-node stage sum of one direction, without the [N, 64 + F] concat
// the reference materialises per stage.  With r = root of node n's tree, (g, t) the folded bn1:
//   conv1_output_sum              sum h1[n]
//   conv1_output_cat_x_sum        sum h1[n] + sum x[r]
//   conv1_output_cat_x_bn1_sum    sum (g_h h1[n] + t_h) + sum (g_x x[r] + t_x)            (EBGCN only)
//   conv2_input_sum               sum relu(h1[n]) + sum relu(x[r])       (EBGCN: over the bn1 outputs)
//   conv2_output_sum              sum h2[n]                              (h2 = conv2 before its relu)
//   scatter_mean_input_sum        sum relu(h2[n]) + sum h1[r]
// Every root term is a property of the tree: k_explain_roots computes the four of them once per
// tree (one workgroup per tree, one pass over the root's x row), k_explain_nodes adds them to the
// node's own 64-wide sums.  The same launch fills x_sum[n] = sum_f x[n][f] (the reference's
// x_sum_top_k): the one pass over all of X and the only HBM-bound part - one wave per row,
// 16-byte non-temporal loads, four in flight per lane, 4 B written per 4 F B read.
// Sums are taken in a fixed order (lane-strided partial sums, a butterfly, wave sums in wave
// order): no atomics on floats, the bits do not depend on the launch.
//
// bgcn_segment_rank - the batched topk(k = n): for every (stage, tree) the tree's local node
// indices by descending value.  Segment bounds come from the PyG batch vector on the device
// (k_seg_bounds); each (stage, tree) is one workgroup.  The order is a total one - the key of
// node i is (value order bits, i), 64 bits, all keys of a segment distinct - so any correct sort
// gives the same answer:
//   n <= BGCN_SEGMENT_RANK_LDS   bitonic network over the keys in LDS
//   longer                       rank by counting: node i goes to slot #{j : key_j < key_i}, the
//                                segment's keys streamed through LDS in chunks; kRankSplit
//                                workgroups share a segment's nodes.  O(n^2) compares, any n.
#include "bgcn_internal.h"

namespace bgcn {
namespace {

constexpr int kH = 64;
constexpr int kRootTerms = 4;     // per tree: sum x[r], its bn / relu forms, sum h1[r]
constexpr int kRankLds = BGCN_SEGMENT_RANK_LDS;
constexpr int kRankSplit = 8;     // workgroups per (stage, tree) on the counting path
static_assert((kRankLds & (kRankLds - 1)) == 0 && kRankLds >= 256, "the bitonic network sorts a power of two");

// sum of the block's 256 values, the same in every thread: butterfly per wave, the four wave
// sums added in wave order.  sm: 4 floats per call site.
__device__ __forceinline__ float block_sum(float v, float* sm) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sm[0] + sm[1]) + sm[2]) + sm[3];
}

// root[b] = { sum x[r], A, C, sum h1[r] }, r = rootindex[b]:
//   no bn:  A = C = sum relu(x[r])
//   bn:     A = sum (g_x x[r] + t_x),  C = sum relu(g_x x[r] + t_x)
// (gx, tx: bn1's last F channels).  A root outside [0, N) is not read: zeros, status bit 0.
__global__ __launch_bounds__(256) void k_explain_roots(const float* __restrict__ h1, int64_t ldh1,
                                                       const float* __restrict__ x, int64_t ldx,
                                                       const int64_t* __restrict__ rootindex, int64_t N, int64_t F,
                                                       const float* __restrict__ gx, const float* __restrict__ tx,
                                                       float* __restrict__ root, int32_t* __restrict__ status) {
  __shared__ float sm[4][4];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x;
  const int64_t r = rootindex[b];
  if (r < 0 || r >= N) {   // block-uniform
    if (tid < kRootTerms) root[b * kRootTerms + tid] = 0.f;
    if (tid == 0) atomicOr(status, 1);
    return;
  }
  const float* xr = x + r * ldx;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  for (int64_t q = tid; q < F / 4; q += 256) {
    const float4 v = ld4(xr + 4 * q);
    s0 += (v.x + v.y) + (v.z + v.w);
    if (gx) {
      const float4 g = ld4(gx + 4 * q), t = ld4(tx + 4 * q);
      const float4 y = make_float4(fmaf(g.x, v.x, t.x), fmaf(g.y, v.y, t.y), fmaf(g.z, v.z, t.z), fmaf(g.w, v.w, t.w));
      const float4 p = f4relu(y);
      s1 += (y.x + y.y) + (y.z + y.w);
      s2 += (p.x + p.y) + (p.z + p.w);
    } else {
      const float4 p = f4relu(v);
      s1 += (p.x + p.y) + (p.z + p.w);
    }
  }
  if (!gx) s2 = s1;
  const float hv = tid < kH ? h1[r * ldh1 + tid] : 0.f;
  const float a0 = block_sum(s0, sm[0]), a1 = block_sum(s1, sm[1]), a2 = block_sum(s2, sm[2]);
  const float a3 = block_sum(hv, sm[3]);
  if (tid == 0) {
    root[b * kRootTerms + 0] = a0;
    root[b * kRootTerms + 1] = a1;
    root[b * kRootTerms + 2] = a2;
    root[b * kRootTerms + 3] = a3;
  }
}

// One wave per node: lane l holds column l of h1[n] and h2[n]; the stage sums are butterflies
// over the wave plus the tree's root terms.  x_sum (optional): the wave streams the node's x row.
// A tree id outside [0, B) takes zeros for its root terms and sets status bit 0.
__global__ __launch_bounds__(256) void k_explain_nodes(const float* __restrict__ h1, int64_t ldh1,
                                                       const float* __restrict__ h2, int64_t ldh2,
                                                       const float* __restrict__ x, int64_t ldx,
                                                       const int64_t* __restrict__ batch, int64_t N, int64_t B,
                                                       int64_t F, const float* __restrict__ g,
                                                       const float* __restrict__ t, const float* __restrict__ root,
                                                       float* __restrict__ sums, int64_t lds, float* __restrict__ x_sum,
                                                       int32_t* __restrict__ status) {
  const int lane = threadIdx.x & 63;
  const int64_t n = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (n >= N) return;   // wave-uniform
  if (x_sum) {
    const float* xr = x + n * ldx;
    const int64_t Q = F / 4;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int64_t q = lane;
    for (; q + 192 < Q; q += 256) {   // four 16-byte loads in flight per lane
      const float4 v0 = ld4_nt(xr + 4 * q), v1 = ld4_nt(xr + 4 * (q + 64));
      const float4 v2 = ld4_nt(xr + 4 * (q + 128)), v3 = ld4_nt(xr + 4 * (q + 192));
      a0 += (v0.x + v0.y) + (v0.z + v0.w);
      a1 += (v1.x + v1.y) + (v1.z + v1.w);
      a2 += (v2.x + v2.y) + (v2.z + v2.w);
      a3 += (v3.x + v3.y) + (v3.z + v3.w);
    }
    for (; q < Q; q += 64) {
      const float4 v = ld4_nt(xr + 4 * q);
      a0 += (v.x + v.y) + (v.z + v.w);
    }
    const float s = wave_sum((a0 + a1) + (a2 + a3));
    if (lane == 0) x_sum[n] = s;
  }
  const int64_t b = batch[n];
  const bool okb = b >= 0 && b < B;
  float r0 = 0.f, r1 = 0.f, r2 = 0.f, r3 = 0.f;
  if (okb) {
    const float4 rv = ld4(root + b * kRootTerms);
    r0 = rv.x; r1 = rv.y; r2 = rv.z; r3 = rv.w;
  } else if (lane == 0) {
    atomicOr(status, 1);
  }
  const float a = h1[n * ldh1 + lane], c = h2[n * ldh2 + lane];
  const float s_h1 = wave_sum(a);
  const float s_h2 = wave_sum(c);
  const float s_h2r = wave_sum(fmaxf(c, 0.f));
  int s = 0;
  if (g) {
    const float y = fmaf(g[lane], a, t[lane]);
    const float s_bn = wave_sum(y), s_bnr = wave_sum(fmaxf(y, 0.f));
    if (lane == 0) {
      sums[(s++) * lds + n] = s_h1;
      sums[(s++) * lds + n] = s_h1 + r0;
      sums[(s++) * lds + n] = s_bn + r1;
      sums[(s++) * lds + n] = s_bnr + r2;
    }
  } else {
    const float s_h1r = wave_sum(fmaxf(a, 0.f));
    if (lane == 0) {
      sums[(s++) * lds + n] = s_h1;
      sums[(s++) * lds + n] = s_h1 + r0;
      sums[(s++) * lds + n] = s_h1r + r2;
    }
  }
  if (lane == 0) {
    sums[(s++) * lds + n] = s_h2;
    sums[(s++) * lds + n] = s_h2r + r3;
  }
}

struct ExplainWs {
  float* root;   // [B, kRootTerms]
};
size_t carve_explain(Carve& c, int64_t B, ExplainWs* w) {
  w->root = c.take<float>(size_t(B) * kRootTerms);
  return align_up(c.off, 256);
}

// ------------------------------------------------------------------ ranking
// Ascending key order = descending value, equal values by ascending index.  -0.0 equals +0.0;
// every NaN is one value above +inf (torch.topk's order).
__device__ __forceinline__ uint64_t rank_key(float v, uint32_t i) {
  uint32_t u = __float_as_uint(v);
  uint32_t k;
  if ((u & 0x7fffffffu) > 0x7f800000u) {
    k = 0xffffffffu;                                   // NaN
  } else {
    if (u == 0x80000000u) u = 0;                       // -0.0
    k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);    // monotone in the value
  }
  return (uint64_t(~k) << 32) | i;
}

// seg[t] = first node of tree t (seg[B] = N), from the non-decreasing batch vector: position i
// (0 .. N) writes the entries of the trees that begin there, (batch[i - 1], batch[i]].  A step
// down or an id outside [0, B) sets *bad and status bit 0; the sort then does not run.
__global__ __launch_bounds__(256) void k_seg_bounds(const int64_t* __restrict__ batch, int64_t N, int64_t B,
                                                    int32_t* __restrict__ seg, int32_t* __restrict__ bad,
                                                    int32_t* __restrict__ status) {
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (i > N) return;
  const int64_t prev = i == 0 ? -1 : batch[i - 1];
  const int64_t cur = i == N ? B : batch[i];
  const bool in_range = i == N || (cur >= 0 && cur < B);
  if (!in_range || cur < prev) {
    atomicOr(bad, 1);
    atomicOr(status, 1);
    return;
  }
  if (prev < -1 || prev >= B) return;   // position i - 1 has flagged it; nothing is written from a bad id
  for (int64_t tr = prev + 1; tr <= cur; ++tr) seg[tr] = int32_t(i);   // -1 <= prev <= cur <= B
}

// grid (B, S, kRankSplit), one (stage, tree) per (x, y)
__global__ __launch_bounds__(256) void k_segment_rank(const float* __restrict__ values, int64_t ld, int64_t N,
                                                      const int32_t* __restrict__ seg, const int32_t* __restrict__ bad,
                                                      int32_t* __restrict__ order, float* __restrict__ sorted) {
  __shared__ uint64_t sk[kRankLds];
  if (*bad) return;
  const int tid = threadIdx.x;
  const int64_t beg = seg[blockIdx.x], end = seg[blockIdx.x + 1];
  if (beg < 0 || end > N || end <= beg) return;   // an empty tree; the bounds hold whenever *bad == 0
  const int n = int(end - beg);
  const float* v = values + int64_t(blockIdx.y) * ld + beg;
  int32_t* po = order + int64_t(blockIdx.y) * N + beg;
  float* ps = sorted + int64_t(blockIdx.y) * N + beg;
  if (n <= kRankLds) {
    if (blockIdx.z != 0) return;
    int P = 2;
    while (P < n) P <<= 1;
    for (int i = tid; i < P; i += 256) sk[i] = i < n ? rank_key(v[i], uint32_t(i)) : ~uint64_t(0);
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int p = tid; p < P / 2; p += 256) {
          const int lo = ((p & ~(j - 1)) << 1) | (p & (j - 1)), hi = lo | j;
          const uint64_t a = sk[lo], b = sk[hi];
          if ((a > b) == ((lo & k) == 0)) {
            sk[lo] = b;
            sk[hi] = a;
          }
        }
        __syncthreads();
      }
    for (int i = tid; i < n; i += 256) {
      const uint32_t src = uint32_t(sk[i]);   // < n: the padding keys sort last
      po[i] = int32_t(src);
      ps[i] = v[src];
    }
    return;
  }
  // counting path: this workgroup's nodes are the 256-node groups z, z + kRankSplit, ...
  for (int base = int(blockIdx.z) * 256; base < n; base += 256 * kRankSplit) {
    const int i = base + tid;
    const float vi = i < n ? v[i] : 0.f;
    const uint64_t ki = i < n ? rank_key(vi, uint32_t(i)) : 0;
    int cnt = 0;
    for (int c0 = 0; c0 < n; c0 += kRankLds) {
      const int m = min(kRankLds, n - c0);
      __syncthreads();
      for (int j = tid; j < m; j += 256) sk[j] = rank_key(v[c0 + j], uint32_t(c0 + j));
      __syncthreads();
      for (int j = 0; j < m; ++j) cnt += sk[j] < ki ? 1 : 0;
    }
    if (i < n) {   // cnt < n: the keys are distinct and ki is one of them
      po[cnt] = i;
      ps[cnt] = vi;
    }
  }
}

struct RankWs {
  int32_t* seg;   // [B + 1]
  int32_t* bad;   // [1]
};
size_t carve_rank(Carve& c, int64_t B, RankWs* w) {
  w->seg = c.take<int32_t>(size_t(B) + 2);   // seg[B + 1] is `bad`: one memset clears both
  w->bad = w->seg ? w->seg + B + 1 : nullptr;
  return align_up(c.off, 256);
}

}  // namespace

int explain_sums_impl(const float* h1, int64_t ldh1, const float* h2, int64_t ldh2, const float* x, int64_t ldx,
                      const int64_t* batch, const int64_t* rootindex, int64_t N, int64_t B, int64_t F, int64_t hid,
                      const float* g, const float* t, float* sums, int64_t lds, float* x_sum, int32_t* status,
                      void* ws, size_t ws_bytes, hipStream_t s) {
  BGCN_CHECK_ARG(hid == kH, "explain_sums: the hidden size must be 64");
  BGCN_CHECK_ARG(F > 0 && F % 4 == 0, "explain_sums: in_feats must be a positive multiple of 4");
  BGCN_CHECK_ARG(N >= 0 && B >= 0, "explain_sums: negative size");
  BGCN_CHECK_ARG(N < (int64_t(1) << 31) && B < (int64_t(1) << 31), "explain_sums: batch too large");
  if (N == 0) return BGCN_OK;
  BGCN_CHECK_ARG(B > 0, "explain_sums: nodes without a tree");
  BGCN_CHECK_ARG(ldh1 >= kH && ldh2 >= kH && ldx >= F && ldx % 4 == 0 && lds >= N,
                 "explain_sums: leading dimensions must cover the rows (x's a multiple of 4)");
  BGCN_CHECK_ARG(h1 && h2 && x && batch && rootindex && sums && status, "explain_sums: null pointer");
  BGCN_CHECK_ARG((g == nullptr) == (t == nullptr), "explain_sums: bn1's g and t come together");
  BGCN_CHECK_ARG(a16(x) && a16(g) && a16(t), "explain_sums: x, bn_g and bn_t must be 16-byte aligned");
  ExplainWs w;
  Carve c(ws, ws_bytes);
  carve_explain(c, B, &w);
  BGCN_CHECK_ARG(ws && c.ok(), "explain_sums: workspace too small");
  hipLaunchKernelGGL(k_explain_roots, dim3(unsigned(B)), dim3(256), 0, s, h1, ldh1, x, ldx, rootindex, N, F,
                     g ? g + kH : nullptr, t ? t + kH : nullptr, w.root, status);
  BGCN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_explain_nodes, dim3(grid_for(N, 4)), dim3(256), 0, s, h1, ldh1, h2, ldh2, x, ldx, batch, N, B,
                     F, g, t, w.root, sums, lds, x_sum, status);
  BGCN_CHECK_LAUNCH();
  return BGCN_OK;
}

int seg_bounds_impl(const int64_t* batch, int64_t N, int64_t B, int32_t* seg, int32_t* status, hipStream_t s) {
  BGCN_CHECK_HIP(hipMemsetAsync(seg, 0, (size_t(B) + 2) * sizeof(int32_t), s));
  hipLaunchKernelGGL(k_seg_bounds, dim3(grid_for(N + 1, 256)), dim3(256), 0, s, batch, N, B, seg, seg + B + 1, status);
  BGCN_CHECK_LAUNCH();
  return BGCN_OK;
}

int segment_rank_impl(const float* values, int64_t ld, int64_t S, const int64_t* batch, int64_t N, int64_t B,
                      int32_t* order, float* sorted, int32_t* status, void* ws, size_t ws_bytes, hipStream_t s) {
  BGCN_CHECK_ARG(N >= 0 && B >= 0 && S >= 0, "segment_rank: negative size");
  BGCN_CHECK_ARG(N < (int64_t(1) << 31) - 1 && B < (int64_t(1) << 31) - 1 && S <= 65535,
                 "segment_rank: too many nodes, trees or stages");
  if (N == 0 || S == 0) return BGCN_OK;
  BGCN_CHECK_ARG(B > 0, "segment_rank: nodes without a tree");
  BGCN_CHECK_ARG(ld >= N, "segment_rank: the leading dimension must cover a stage");
  BGCN_CHECK_ARG(values && batch && order && sorted && status, "segment_rank: null pointer");
  RankWs w;
  Carve c(ws, ws_bytes);
  carve_rank(c, B, &w);
  BGCN_CHECK_ARG(ws && c.ok(), "segment_rank: workspace too small");
  BGCN_TRY(seg_bounds_impl(batch, N, B, w.seg, status, s));
  hipLaunchKernelGGL(k_segment_rank, dim3(unsigned(B), unsigned(S), kRankSplit), dim3(256), 0, s, values, ld, N,
                     w.seg, w.bad, order, sorted);
  BGCN_CHECK_LAUNCH();
  return BGCN_OK;
}

}  // namespace bgcn

extern "C" size_t bgcn_explain_sums_workspace_size(int64_t num_graphs) {
  if (num_graphs < 0) return 0;
  bgcn::ExplainWs w;
  bgcn::Carve c(nullptr, 0);
  return bgcn::carve_explain(c, num_graphs, &w);
}

extern "C" int bgcn_explain_sums(const float* h1, int64_t ldh1, const float* h2, int64_t ldh2, const float* x,
                                 int64_t ldx, const int64_t* batch, const int64_t* rootindex, int64_t num_nodes,
                                 int64_t num_graphs, int64_t in_feats, int64_t hid, const float* bn_g,
                                 const float* bn_t, float* sums, int64_t ld_sums, float* x_sum, int32_t* status,
                                 void* workspace, size_t workspace_bytes, bgcn_stream_t stream) {
  return bgcn::explain_sums_impl(h1, ldh1, h2, ldh2, x, ldx, batch, rootindex, num_nodes, num_graphs, in_feats, hid,
                                 bn_g, bn_t, sums, ld_sums, x_sum, status, workspace, workspace_bytes,
                                 reinterpret_cast<hipStream_t>(stream));
}

extern "C" size_t bgcn_segment_rank_workspace_size(int64_t num_graphs) {
  if (num_graphs < 0) return 0;
  bgcn::RankWs w;
  bgcn::Carve c(nullptr, 0);
  return bgcn::carve_rank(c, num_graphs, &w);
}

extern "C" int bgcn_segment_rank(const float* values, int64_t ld, int64_t num_stages, const int64_t* batch,
                                 int64_t num_nodes, int64_t num_graphs, int32_t* order, float* sorted,
                                 int32_t* status, void* workspace, size_t workspace_bytes, bgcn_stream_t stream) {
  return bgcn::segment_rank_impl(values, ld, num_stages, batch, num_nodes, num_graphs, order, sorted, status,
                                 workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream));
}
