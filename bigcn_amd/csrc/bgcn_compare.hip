// The comparison side of the reference's explainability study (compare_similarity.py:38-183): a
// tree's nodes are ranked by three graph centralities as well as by the models' stage sums, and
// every pair of rankings is scored per tree with five statistics over the top-k lists.
//
// bgcn_tree_centrality - out-degree, betweenness and closeness centrality of every node of every
// propagation tree, as networkx defines them on the DiGraph of the top-down edges (default
// arguments; the script that wrote the reference's centrality files is not part of it).  For a
// tree of n nodes and a node with c children, depth d and subtree size s (itself included):
//   out_degree  = c / (n - 1)                        (1 when n = 1, as networkx)
//   betweenness = d (s - 1) / ((n - 1)(n - 2))       (0 when n <= 2): d ancestors x s - 1 descendants
//   closeness   = 2 d / ((d + 1)(n - 1))             (0 when d = 0): inward distances 1 .. d over
//                                                    the d ancestors, Wasserman-Faust scaled
// c, d, s, n are integers, computed exactly; each value is ONE fp64 division rounded once to
// fp32, so equal integer keys give bit-equal floats and the ranking's tie rule applies.
//   k_tree_parents     one thread per edge: par[child] = parent (atomicCAS: a second incoming edge
//                      is refused), endpoints range-checked, an edge that leaves its tree refused
//   k_tree_centrality  one workgroup per tree.  Pointer jumping, ceil(log2 n) rounds: with a_r(v)
//                      the 2^r-th ancestor of v (-1: none),
//                        dep_r+1(v) = dep_r(v) + dep_r(a_r(v))     dep_r(v) = min(d(v), 2^r)
//                        acc_r+1(u) = acc_r(u) + sum over {w : a_r(w) = u} of acc_r(w)
//                      acc_r(u) = #descendants of u closer than 2^r, u included (integer atomic
//                      adds: exact, any order).  A pointer still alive after the rounds has walked
//                      n steps without leaving the tree: a cycle.  A tree of at most
//                      BGCN_TREE_CENTRALITY_LDS nodes keeps its seven int32 arrays in LDS (28 B per
//                      node, 56 KiB: two workgroups per CU); a longer one runs the same code on its
//                      slice of the workspace.
// A DropEdge'd forest is fine: depth and subtree size are per component, n the tree's node count.
//
// bgcn_rank_similarity - per tree of more than k nodes, for every ordered pair (i, j) of V
// rankings, over the first k entries x, y of the two (k distinct local node indices each):
//   0 Pearson r    (k Sxy - Sx Sy) / sqrt((k Sxx - Sx^2)(k Syy - Sy^2))   with k Sxy - Sx Sy =
//                  sum over a < b of (x_a - x_b)(y_a - y_b)
//   1 Spearman     the same of the entries' ranks inside their list
//   2 Kendall tau  sum over a < b of sign(x_a - x_b) sign(y_a - y_b) / (k (k - 1) / 2)
//   3 Somers' D    = tau (no ties: tau-b = tau-a = D)
//   4 Jaccard      m / (2 k - m), m = entries in common
// Sums in int64 (exact), one fp64 division (and one sqrt for 0 and 1) per value.  One workgroup
// per tree, the lists and their ranks in LDS, one thread per (i, j).
#include "bgcn_internal.h"

namespace bgcn {
namespace {

constexpr int kCentLds = BGCN_TREE_CENTRALITY_LDS;
constexpr int kCentArrays = 7;   // int32 per node: 2 x ancestor, 2 x depth, 2 x descendants, children
static_assert(kCentLds * kCentArrays * 4 <= 64 * 1024, "two trees per CU: at most 64 KiB of its 160");
constexpr int kMaxK = BGCN_RANK_SIMILARITY_MAX;
constexpr int kMaxV = BGCN_RANK_SIMILARITY_MAX;

// par[d] = s for every edge (s, d); par starts at -1.  tree_bad[t] != 0: tree t is refused.
// *bad (k_seg_bounds, run before): the batch vector is not one, and which tree an edge lies in
// means nothing - that is the one thing reported.
__global__ __launch_bounds__(256) void k_tree_parents(const int64_t* __restrict__ ei, int64_t E,
                                                      const int64_t* __restrict__ batch, int64_t N, int64_t B,
                                                      const int32_t* __restrict__ bad, int32_t* __restrict__ par,
                                                      int32_t* __restrict__ tree_bad, int32_t* __restrict__ status) {
  const int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (e >= E || *bad) return;
  const int64_t s = ei[e], d = ei[E + e];
  const bool s_ok = s >= 0 && s < N, d_ok = d >= 0 && d < N;
  const int64_t bs = s_ok ? batch[s] : -1, bd = d_ok ? batch[d] : -1;
  const bool bs_ok = bs >= 0 && bs < B, bd_ok = bd >= 0 && bd < B;   // (a bad id: k_seg_bounds flags it)
  int32_t flag = 0;
  if (!s_ok || !d_ok) {
    flag = 1;
  } else if (bs != bd) {
    flag = 1 | BGCN_STATUS_CROSS_TREE;
  } else if (bd_ok && atomicCAS(&par[d], -1, int32_t(s)) != -1) {
    flag = 1 | BGCN_STATUS_TWO_PARENTS;
  }
  if (flag) {
    if (bs_ok) atomicOr(&tree_bad[bs], 1);
    if (bd_ok) atomicOr(&tree_bad[bd], 1);
    atomicOr(status, flag);
  }
}

// A word the workgroup's other waves add to with atomics (performed in L2 when the array is in
// global memory): read past the L1.
__device__ __forceinline__ int32_t ld_sum(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The tree's arrays a0 .. cnt (n entries each) live in LDS or in global memory; the code is the
// same.  Returns false (block-uniform) for a cycle.
__device__ __forceinline__ bool tree_body(const int32_t* __restrict__ par, int beg, int n, int32_t* a0, int32_t* a1,
                                          int32_t* d0, int32_t* d1, int32_t* c0, int32_t* c1, int32_t* cnt,
                                          int32_t** dep, int32_t** acc) {
  const int tid = threadIdx.x;
  for (int i = tid; i < n; i += 256) {
    const int32_t p = par[beg + i];
    const int32_t a = p < 0 ? -1 : p - beg;   // in [0, n): the edge stayed inside the tree
    a0[i] = a;
    d0[i] = a >= 0 ? 1 : 0;
    c0[i] = 1;
    cnt[i] = 0;
  }
  __syncthreads();
  for (int i = tid; i < n; i += 256)
    if (a0[i] >= 0) atomicAdd(&cnt[a0[i]], 1);
  for (int span = 1; span < n; span <<= 1) {   // ceil(log2 n) rounds
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
      const int32_t a = a0[i];
      a1[i] = a >= 0 ? a0[a] : -1;
      d1[i] = d0[i] + (a >= 0 ? d0[a] : 0);
      c1[i] = ld_sum(&c0[i]);
    }
    __syncthreads();
    for (int i = tid; i < n; i += 256)
      if (a0[i] >= 0) atomicAdd(&c1[a0[i]], ld_sum(&c0[i]));
    int32_t* t;
    t = a0; a0 = a1; a1 = t;
    t = d0; d0 = d1; d1 = t;
    t = c0; c0 = c1; c1 = t;
  }
  int alive = 0;
  for (int i = tid; i < n; i += 256) alive |= a0[i] >= 0;
  *dep = d0;
  *acc = c0;
  return __syncthreads_or(alive) == 0;   // (also orders the last round's atomics before the reads)
}

__global__ __launch_bounds__(256) void k_tree_centrality(const int32_t* __restrict__ par,
                                                         const int32_t* __restrict__ seg,
                                                         const int32_t* __restrict__ tree_bad, int64_t N,
                                                         int32_t* __restrict__ gws, float* __restrict__ cent,
                                                         int64_t ld, int32_t* __restrict__ status) {
  __shared__ int32_t sm[kCentArrays][kCentLds];
  const int32_t* bad = seg + gridDim.x + 1;
  if (*bad) return;
  const int64_t beg = seg[blockIdx.x], end = seg[blockIdx.x + 1];
  if (beg < 0 || end > N || end <= beg) return;   // an empty tree; the bounds hold whenever *bad == 0
  if (tree_bad[blockIdx.x]) return;
  const int n = int(end - beg);
  int32_t *dep, *acc, *cnt;
  bool ok;
  if (n <= kCentLds) {
    cnt = sm[6];
    ok = tree_body(par, int(beg), n, sm[0], sm[1], sm[2], sm[3], sm[4], sm[5], cnt, &dep, &acc);
  } else {
    int32_t* g = gws + beg;   // array q of the tree: gws[q * N + beg ..]
    cnt = g + 6 * N;
    ok = tree_body(par, int(beg), n, g, g + N, g + 2 * N, g + 3 * N, g + 4 * N, g + 5 * N, cnt, &dep, &acc);
  }
  if (!ok) {
    if (threadIdx.x == 0) atomicOr(status, 1 | BGCN_STATUS_CYCLE);
    return;
  }
  const int64_t n1 = n - 1;
  const double den_b = double(n1 * (n1 - 1));
  for (int i = threadIdx.x; i < n; i += 256) {
    const int64_t c = ld_sum(&cnt[i]), d = dep[i], s = ld_sum(&acc[i]);
    cent[beg + i] = n == 1 ? 1.0f : float(double(c) / double(n1));
    cent[ld + beg + i] = n > 2 ? float(double(d * (s - 1)) / den_b) : 0.0f;
    cent[2 * ld + beg + i] = d > 0 ? float(double(2 * d) / double((d + 1) * n1)) : 0.0f;
  }
}

struct CentWs {
  int32_t* seg;        // [B + 2], seg[B + 1] = bad
  int32_t* tree_bad;   // [B]
  int32_t* par;        // [N]
  int32_t* arrays;     // [kCentArrays][N]: the trees too long for LDS
};
size_t carve_cent(Carve& c, int64_t N, int64_t B, CentWs* w) {
  w->seg = c.take<int32_t>(size_t(B) + 2);
  w->tree_bad = c.take<int32_t>(size_t(B));
  w->par = c.take<int32_t>(size_t(N));
  w->arrays = c.take<int32_t>(size_t(N) * kCentArrays);
  return align_up(c.off, 256);
}

// ------------------------------------------------------------------ rank similarity
// sum over a < b of (x_a - x_b)(y_a - y_b), and of the products of the differences' signs
__device__ __forceinline__ void pair_sums(const int32_t* x, const int32_t* y, int k, int64_t* cov, int32_t* conc) {
  int64_t s = 0;
  int32_t c = 0;
  for (int a = 0; a < k; ++a) {
    const int64_t xa = x[a], ya = y[a];
    for (int b = a + 1; b < k; ++b) {
      const int64_t dx = xa - x[b], dy = ya - y[b];
      s += dx * dy;
      c += ((dx > 0) - (dx < 0)) * ((dy > 0) - (dy < 0));
    }
  }
  *cov = s;
  *conc = c;
}

__global__ __launch_bounds__(256) void k_rank_similarity(const int32_t* __restrict__ orders, int64_t ld, int V,
                                                         const int32_t* __restrict__ seg, int64_t N, int k,
                                                         double* __restrict__ sim, int32_t* __restrict__ valid,
                                                         int32_t* __restrict__ status) {
  __shared__ int32_t sx[kMaxV][kMaxK + 1];   // the lists (+ 1: rows on different banks)
  __shared__ int32_t sr[kMaxV][kMaxK + 1];   // an entry's rank inside its list
  const int32_t* bad = seg + gridDim.x + 1;
  if (*bad) return;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  double* out = sim + b * 5 * V * V;
  const int64_t beg = seg[b], end = seg[b + 1];
  const bool bounds_ok = beg >= 0 && end <= N && end >= beg;   // holds whenever *bad == 0
  const int64_t n = bounds_ok ? end - beg : 0;
  if (n <= k) {   // the reference's `continue`: zeros
    for (int q = tid; q < 5 * V * V; q += 256) out[q] = 0.0;
    if (tid == 0) valid[b] = 0;
    return;
  }
  for (int q = tid; q < V * k; q += 256) sx[q / k][q % k] = orders[int64_t(q / k) * ld + beg + q % k];
  __syncthreads();
  int repeat = 0;
  for (int q = tid; q < V * k; q += 256) {
    const int v = q / k, t = q % k;
    const int32_t xv = sx[v][t];
    int r = 0;
    for (int u = 0; u < k; ++u) {
      r += sx[v][u] < xv;
      repeat |= u != t && sx[v][u] == xv;
    }
    repeat |= xv < 0 || xv >= n;
    sr[v][t] = r;
  }
  if (__syncthreads_or(repeat)) {   // not a ranking
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    for (int q = tid; q < 5 * V * V; q += 256) out[q] = nan;
    if (tid == 0) {
      valid[b] = 0;
      atomicOr(status, 2);
    }
    return;
  }
  const double pairs = double(k * (k - 1) / 2);
  for (int q = tid; q < V * V; q += 256) {
    const int i = q / V, j = q % V;
    int64_t cxy, cxx, cyy, rxy, rxx, ryy;
    int32_t conc, unused;
    pair_sums(sx[i], sx[j], k, &cxy, &conc);
    pair_sums(sx[i], sx[i], k, &cxx, &unused);
    pair_sums(sx[j], sx[j], k, &cyy, &unused);
    pair_sums(sr[i], sr[j], k, &rxy, &unused);
    pair_sums(sr[i], sr[i], k, &rxx, &unused);
    pair_sums(sr[j], sr[j], k, &ryy, &unused);
    int m = 0;
    for (int a = 0; a < k; ++a)
      for (int c = 0; c < k; ++c) m += sx[i][a] == sx[j][c];
    const double tau = double(conc) / pairs;
    out[0 * V * V + q] = double(cxy) / sqrt(double(cxx) * double(cyy));
    out[1 * V * V + q] = double(rxy) / sqrt(double(rxx) * double(ryy));
    out[2 * V * V + q] = tau;
    out[3 * V * V + q] = tau;
    out[4 * V * V + q] = double(m) / double(2 * k - m);
  }
  if (tid == 0) valid[b] = 1;
}

struct SimWs {
  int32_t* seg;   // [B + 2], seg[B + 1] = bad
};
size_t carve_sim(Carve& c, int64_t B, SimWs* w) {
  w->seg = c.take<int32_t>(size_t(B) + 2);
  return align_up(c.off, 256);
}

}  // namespace

int tree_centrality_impl(const int64_t* ei, int64_t E, const int64_t* batch, int64_t N, int64_t B, float* cent,
                         int64_t ld, int32_t* status, void* ws, size_t ws_bytes, hipStream_t s) {
  BGCN_CHECK_ARG(N >= 0 && B >= 0 && E >= 0, "tree_centrality: negative size");
  BGCN_CHECK_ARG(N < (int64_t(1) << 31) - 1 && B < (int64_t(1) << 31) - 1 && E < (int64_t(1) << 31),
                 "tree_centrality: too many nodes, trees or edges");
  if (N == 0) return BGCN_OK;
  BGCN_CHECK_ARG(B > 0, "tree_centrality: nodes without a tree");
  BGCN_CHECK_ARG(ld >= N, "tree_centrality: the leading dimension must cover a row");
  BGCN_CHECK_ARG((ei || E == 0) && batch && cent && status, "tree_centrality: null pointer");
  CentWs w;
  Carve c(ws, ws_bytes);
  carve_cent(c, N, B, &w);
  BGCN_CHECK_ARG(ws && c.ok(), "tree_centrality: workspace too small");
  BGCN_TRY(seg_bounds_impl(batch, N, B, w.seg, status, s));
  BGCN_CHECK_HIP(hipMemsetAsync(w.tree_bad, 0, size_t(B) * sizeof(int32_t), s));
  BGCN_CHECK_HIP(hipMemsetAsync(w.par, 0xff, size_t(N) * sizeof(int32_t), s));
  if (E > 0) {
    hipLaunchKernelGGL(k_tree_parents, dim3(grid_for(E, 256)), dim3(256), 0, s, ei, E, batch, N, B, w.seg + B + 1,
                       w.par, w.tree_bad, status);
    BGCN_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_tree_centrality, dim3(unsigned(B)), dim3(256), 0, s, w.par, w.seg, w.tree_bad, N, w.arrays,
                     cent, ld, status);
  BGCN_CHECK_LAUNCH();
  return BGCN_OK;
}

int rank_similarity_impl(const int32_t* orders, int64_t ld, int64_t V, const int64_t* batch, int64_t N, int64_t B,
                         int32_t k, double* sim, int32_t* valid, int32_t* status, void* ws, size_t ws_bytes,
                         hipStream_t s) {
  BGCN_CHECK_ARG(N >= 0 && B >= 0, "rank_similarity: negative size");
  BGCN_CHECK_ARG(k >= 2 && k <= kMaxK, "rank_similarity: k must be in [2, 32]");
  BGCN_CHECK_ARG(V >= 1 && V <= kMaxV, "rank_similarity: the number of rankings must be in [1, 32]");
  // k Sxy - Sx Sy < k^2 n^2 / 2 must fit int64
  BGCN_CHECK_ARG(N < (int64_t(1) << 26) && B < (int64_t(1) << 31) - 1, "rank_similarity: too many nodes or trees");
  if (B == 0) return BGCN_OK;
  BGCN_CHECK_ARG(ld >= N, "rank_similarity: the leading dimension must cover a ranking");
  BGCN_CHECK_ARG((orders || N == 0) && (batch || N == 0) && sim && valid && status, "rank_similarity: null pointer");
  SimWs w;
  Carve c(ws, ws_bytes);
  carve_sim(c, B, &w);
  BGCN_CHECK_ARG(ws && c.ok(), "rank_similarity: workspace too small");
  BGCN_TRY(seg_bounds_impl(batch, N, B, w.seg, status, s));
  hipLaunchKernelGGL(k_rank_similarity, dim3(unsigned(B)), dim3(256), 0, s, orders, ld, int(V), w.seg, N, int(k), sim,
                     valid, status);
  BGCN_CHECK_LAUNCH();
  return BGCN_OK;
}

}  // namespace bgcn

extern "C" size_t bgcn_tree_centrality_workspace_size(int64_t num_nodes, int64_t num_graphs) {
  if (num_nodes < 0 || num_graphs < 0) return 0;
  bgcn::CentWs w;
  bgcn::Carve c(nullptr, 0);
  return bgcn::carve_cent(c, num_nodes, num_graphs, &w);
}

extern "C" int bgcn_tree_centrality(const int64_t* edge_index, int64_t num_edges, const int64_t* batch,
                                    int64_t num_nodes, int64_t num_graphs, float* cent, int64_t ld, int32_t* status,
                                    void* workspace, size_t workspace_bytes, bgcn_stream_t stream) {
  return bgcn::tree_centrality_impl(edge_index, num_edges, batch, num_nodes, num_graphs, cent, ld, status, workspace,
                                    workspace_bytes, reinterpret_cast<hipStream_t>(stream));
}

extern "C" size_t bgcn_rank_similarity_workspace_size(int64_t num_graphs) {
  if (num_graphs < 0) return 0;
  bgcn::SimWs w;
  bgcn::Carve c(nullptr, 0);
  return bgcn::carve_sim(c, num_graphs, &w);
}

extern "C" int bgcn_rank_similarity(const int32_t* orders, int64_t ld, int64_t num_lists, const int64_t* batch,
                                    int64_t num_nodes, int64_t num_graphs, int32_t k, double* sim, int32_t* valid,
                                    int32_t* status, void* workspace, size_t workspace_bytes, bgcn_stream_t stream) {
  return bgcn::rank_similarity_impl(orders, ld, num_lists, batch, num_nodes, num_graphs, k, sim, valid, status,
                                    workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream));
}
