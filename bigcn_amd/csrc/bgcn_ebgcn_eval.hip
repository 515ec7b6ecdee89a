// bgcn_ebgcn_eval_step: the EBGCN test loop body (model/Twitter/EBGCN.py:328-354) as one launch
// sequence on the caller's stream, everything in the caller's workspace:
//
//   k_eval_fold       the four eval-mode BatchNorms (bn1, sim_valnorm0; TD, BU) folded to (g, t)
//   pair build        K1, unweighted: both directions' CSR structure and conv1's values, once
//   k_eval_slots      each edge's entry in the by-target CSR (and the edge of each entry on the
//                     degree side), from what the build left in its workspace
//   seg bounds        the trees' node ranges
//   conv1             one X W1^T pass for both directions (128 columns) + one aggregation launch
//   per direction     k_edge_infer -> edge_pred; conv2's lin (bgcn_ebgcn_conv2_lin)
//   k_eval_degree     reweight, pass 1: the weighted degree in row order, self loop last -> dinv
//   k_eval_reweight   reweight, pass 2: dinv[src] * edge_pred * dinv[dst] into a second value
//                     array over the same t_ptr / t_col (the only reuse is dinv)
//   conv2             one aggregation launch for both directions (+ bias, relu)
//   k_eval_readout    one workgroup per tree: mean of relu(h2) in node order, h1[root], the head
//                     row (BU first), fc, log_softmax, the NLL term, the argmax
//   k_eval_finish     one workgroup: mean loss and correct count over the trees, fixed order
//
// The existing path (bigcn_amd/ebgcn.py forward) builds each direction's graph twice - the
// second, edge-weighted build sorts and places every edge again only to change the values.
#include "bgcn_graph_body.h"
#include "bgcn_internal.h"

namespace bgcn {

int build_graphs_impl(const GraphArgs* ga, int count, int64_t N, int degree_on, hipStream_t s, const int64_t* batch);
int edge_infer_impl(const float* h, int64_t ldh, int64_t N, int64_t hid, const int64_t* ei, int64_t E,
                    const float* Wc, const float* g, const float* t, const float* wout, const float* bout,
                    const float* fc1, int32_t K, float* pred, int32_t* status, hipStream_t s);
int conv2_lin_impl(const float* h1, int64_t ldh, const float* x, int64_t ldx, const int64_t* batch,
                   const int64_t* rootindex, int64_t N, int64_t B, int64_t F, int64_t hid, const float* w2,
                   const float* g, const float* t, float* z2, int64_t ldz, int32_t* status, void* ws, size_t ws_bytes,
                   hipStream_t s);

namespace {

constexpr int kH = 64;
constexpr int kLd = 2 * kH;   // per-node matrices are [N, 128]: TD in columns [0, 64), BU in [64, 128)

// ---- folded norms: job j = 2 * dir + (0: bn1 over [64 + F], 1: sim_valnorm0 over [64])
struct FoldJob {
  const float *gamma, *beta, *mean, *var;
  float eps;
  int64_t C;
  float *g, *t;
};
struct FoldArgs {
  FoldJob j[4];
  int32_t* status;   // zeroed here: this is the call's first launch
};
__global__ __launch_bounds__(256) void k_eval_fold(FoldArgs a) {
  const FoldJob& j = a.j[blockIdx.y];
  const int64_t c = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *a.status = 0;
  if (c >= j.C) return;
  bn_fold(j.gamma[c], j.beta[c], j.mean[c], j.var[c], j.eps, j.g[c], j.t[c]);
}

// ---- edge slots.  slot[e] = the entry of edge e in the by-target CSR (as fill_nodes / rank_norm
// placed it: run rank when grouped, else the rank by edge id), -1 for an edge the build left
// out; eid[p] = the edge at entry p of the degree side's CSR (by target for BGCN_DEGREE_ON_COL,
// by source for _ROW), written for every entry but the self loops.
struct SlotArgs {
  int32_t* slot[2];
  int32_t* eid[2];
};
__device__ __forceinline__ int64_t rank_slot(const int32_t* ptr, const int32_t* cnt, const int32_t* tmp,
                                             int64_t key, int64_t e) {
  const int64_t a = ptr[key], n = cnt[key];
  int r = 0;
  for (int64_t q = 0; q < n; ++q) r += tmp[a + q] < e;
  return a + r;
}
__global__ __launch_bounds__(256) void k_eval_slots(GraphBatch gb, SlotArgs sa) {
  const GraphIO& G = gb.g[blockIdx.y];
  const int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (e >= G.E) return;
  int64_t src, dst;
  bool valid;
  if (!edge_kept(G.ei, G.E, gb.N, e, src, dst, valid)) {
    sa.slot[blockIdx.y][e] = -1;
    return;
  }
  const int64_t pt = graph_grouped_t(G) ? G.t_ptr[dst] + (e - G.run_t[dst])
                                        : rank_slot(G.t_ptr, G.cnt_t, G.tmp_t, dst, e);
  sa.slot[blockIdx.y][e] = int32_t(pt);
  int64_t pd = pt;
  if (gb.degree_on != BGCN_DEGREE_ON_COL)
    pd = graph_grouped_s(G) ? G.s_ptr[src] + (e - G.run_s[src]) : rank_slot(G.s_ptr, G.cnt_s, G.tmp_s, src, e);
  sa.eid[blockIdx.y][pd] = int32_t(e);
}

// ---- reweight (per direction d = blockIdx.y; on == 0: nothing to do)
struct Reweight {
  int on;
  int64_t E;
  const int64_t* ei;
  const float* pred;        // [E]
  const int32_t* d_ptr;     // [N + 1] row pointers of the degree side
  const int32_t* eid;       // edge of each of its entries
  const int32_t* t_ptr;     // [N + 1]
  const int32_t* slot;      // [E]
  float* dinv;              // [N]
  float* w2;                // [E + N]
};
struct ReweightArgs {
  Reweight d[2];
  int64_t N;
};
// pass 1, node i: scatter_add of the weights at i in edge order (= row order), then the self
// loop's 1 (k_nodes' order), deg^-1/2 with inf -> 0
__global__ __launch_bounds__(256) void k_eval_degree(ReweightArgs a) {
  const Reweight& R = a.d[blockIdx.y];
  if (!R.on) return;
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (i >= a.N) return;
  const int64_t p0 = R.d_ptr[i], p1 = int64_t(R.d_ptr[i + 1]) - 1;   // the loop is the row's last entry
  float deg = 0.f;
  int64_t p = p0;
  for (; p + 4 <= p1; p += 4) {   // four gathers in flight, added in order
    const float w0 = R.pred[R.eid[p]], w1 = R.pred[R.eid[p + 1]], w2 = R.pred[R.eid[p + 2]],
                w3 = R.pred[R.eid[p + 3]];
    deg += w0; deg += w1; deg += w2; deg += w3;
  }
  for (; p < p1; ++p) deg += R.pred[R.eid[p]];
  deg += 1.f;
  float d = 1.0f / sqrtf(deg);
  if (isinf(d)) d = 0.f;
  R.dinv[i] = d;
}
// pass 2, thread idx over [0, E + N): edge idx -> its entry; node idx - E -> its loop's entry;
// entry idx past the valid ones -> 0 (the aggregation kernels read the capacity tail)
__global__ __launch_bounds__(256) void k_eval_reweight(ReweightArgs a) {
  const Reweight& R = a.d[blockIdx.y];
  if (!R.on) return;
  const int64_t idx = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (idx >= R.E + a.N) return;
  if (idx < R.E) {
    const int32_t p = R.slot[idx];
    if (p >= 0) R.w2[p] = (R.dinv[R.ei[idx]] * R.pred[idx]) * R.dinv[R.ei[R.E + idx]];
  } else {
    const int64_t i = idx - R.E;
    const float d = R.dinv[i];
    R.w2[R.t_ptr[i + 1] - 1] = (d * 1.f) * d;
  }
  if (idx >= R.t_ptr[a.N]) R.w2[idx] = 0.f;
}

// ---- readout + head, workgroup b = tree b.  Threads [0, 128): column c of the [N, 128]
// relu(h2) (the aggregation's relu epilogue stored it), summed over the tree's nodes in node
// order; threads [128, 256): h1[root].  Head row (EBGCN.py:227, :86-92):
//   [0, 64) BU mean relu(h2) | [64, 128) BU h1[root] | [128, 192) TD mean | [192, 256) TD h1[root]
// then wave 0 evaluates fc -> log_softmax -> NLL term / argmax with k_head_fwd's expressions.
struct ReadoutArgs {
  const float *h1, *h2;
  const int64_t *batch, *rootindex;
  const int32_t* seg;   // [B + 2]: node range starts, N, `bad`
  int64_t N, B;
  const float *W, *bias;
  const int64_t* y;
  int C;
  float *logp, *loss_row;
  int32_t* predw;
  int64_t* pred;
  int32_t* status;
};
__global__ __launch_bounds__(256) void k_eval_readout(ReadoutArgs a) {
  __shared__ __attribute__((aligned(16))) float head[kHeadIn];
  __shared__ int s_cnt;
  const int t = threadIdx.x;
  const int64_t b = blockIdx.x;
  const bool bad = a.seg[a.B + 1] != 0;
  float rootv = 0.f;
  if (t >= kLd) {
    const int64_t r = a.rootindex[b];
    if (r >= 0 && r < a.N) rootv = a.h1[r * kLd + (t - kLd)];
    else if (t == kLd) atomicOr(a.status, 1);
  } else {
    const float* col = a.h2 + t;
    float sum = 0.f;
    int64_t cnt = 0;
    if (!bad) {
      const int64_t s = a.seg[b], e = a.seg[b + 1];
      cnt = e - s;
      int64_t i = s;
      for (; i + 8 <= e; i += 8) {   // eight row loads in flight, added in node order
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = col[(i + u) * kLd];
#pragma unroll
        for (int u = 0; u < 8; ++u) sum += v[u];
      }
      for (; i < e; ++i) sum += col[i * kLd];
    } else {   // not usable as segments: pick the tree's nodes out of the whole vector
      for (int64_t i = 0; i < a.N; ++i)
        if (a.batch[i] == b) {
          sum += col[i * kLd];
          ++cnt;
        }
    }
    if (t == 0) {
      s_cnt = cnt > 0;
      if (bad && b == 0) atomicOr(a.status, BGCN_STATUS_BATCH_UNSORTED);
    }
    head[t < kH ? 2 * kH + t : t - kH] = cnt > 0 ? sum / float(cnt) : 0.f;
  }
  __syncthreads();
  if (t >= kLd) head[t < kLd + kH ? 3 * kH + (t - kLd) : t - kLd] = s_cnt ? rootv : 0.f;
  __syncthreads();
  if (t >= kWave) return;
  const int l = t, C = a.C;
  const float4 h = ld4(&head[4 * l]);
  float z[kMaxClasses];
  float mx = -INFINITY;
#pragma unroll
  for (int c = 0; c < kMaxClasses; ++c) {
    z[c] = 0.f;
    if (c < C) {   // C is uniform: the shuffles stay convergent
      const float4 w = ld4(a.W + int64_t(c) * kHeadIn + 4 * l);
      float p = h.x * w.x + h.y * w.y + h.z * w.z + h.w * w.w;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) p += __shfl_xor(p, o);
      z[c] = p + a.bias[c];
      mx = fmaxf(mx, z[c]);
    }
  }
  float se = 0.f;
#pragma unroll
  for (int c = 0; c < kMaxClasses; ++c)
    if (c < C) se += expf(z[c] - mx);
  const float lse = mx + logf(se);
  const int64_t yb = a.y ? a.y[b] : 0;
  const bool yok = a.y && yb >= 0 && yb < C;
  int best = 0;
  float bv = z[0] - lse, ly = 0.f;
#pragma unroll
  for (int c = 0; c < kMaxClasses; ++c) {
    if (c < C) {
      const float lp = z[c] - lse;
      if (l == c && a.logp) a.logp[b * C + c] = lp;
      if (c > 0 && lp > bv) {   // the first maximal class, as torch's max
        bv = lp;
        best = c;
      }
      if (yok && c == yb) ly = lp;
    }
  }
  if (l == 0) {
    a.loss_row[b] = yok ? -ly : 0.f;
    a.predw[b] = best;
    if (a.pred) a.pred[b] = best;
    if (a.y && !yok) atomicOr(a.status, 2);
  }
}

// the mean NLL and the correct count over the trees: strided thread sums, then a halving tree
// (k_eval_finish's order)
__global__ __launch_bounds__(256) void k_eval_finish2(const float* __restrict__ loss_row,
                                                      const int32_t* __restrict__ predw,
                                                      const int64_t* __restrict__ y, int64_t B,
                                                      float* __restrict__ loss, int32_t* __restrict__ correct) {
  __shared__ float ls[256];
  __shared__ int32_t cs[256];
  const int t = threadIdx.x;
  float s = 0.f;
  int32_t n = 0;
  for (int64_t b = t; b < B; b += 256) {
    s += loss_row[b];
    n += (y && y[b] == int64_t(predw[b])) ? 1 : 0;
  }
  ls[t] = s;
  cs[t] = n;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
      ls[t] += ls[t + o];
      cs[t] += cs[t + o];
    }
    __syncthreads();
  }
  if (t == 0) {
    *loss = ls[0] / float(B);
    *correct = cs[0];
  }
}

struct EvalWs {
  bgcn_csr_out csr[2];
  float* t_w2[2];
  int32_t *slot[2], *eid[2];
  float* dinv[2];
  float* pred[2];
  float *bn_g[2], *bn_t[2], *sim_g[2], *sim_t[2];
  float *z1, *h1, *z2, *h2;
  float* part[2];
  int32_t *seg, *scratch, *predw;
  float* loss_row;
  void* gws;
  size_t gws_bytes;
  void* c2ws;
  size_t c2_bytes;
};

size_t carve_eval(Carve& c, int64_t N, int64_t B, int64_t F, const int64_t E[2], EvalWs* w) {
  const size_t n = size_t(N), nb = size_t(B);
  for (int k = 0; k < 2; ++k) {
    const size_t cap = size_t(E[k] + N), e1 = size_t(E[k] > 0 ? E[k] : 1);
    bgcn_csr_out& g = w->csr[k];
    g.t_ptr = c.take<int32_t>(n + 1); g.t_row = c.take<int32_t>(cap); g.t_col = c.take<int32_t>(cap);
    g.t_w = c.take<float>(cap);
    g.s_ptr = c.take<int32_t>(n + 1); g.s_row = c.take<int32_t>(cap); g.s_col = c.take<int32_t>(cap);
    g.s_w = c.take<float>(cap);
    w->t_w2[k] = c.take<float>(cap);
    w->slot[k] = c.take<int32_t>(e1);
    w->eid[k] = c.take<int32_t>(cap);
    w->dinv[k] = c.take<float>(n);
    w->pred[k] = c.take<float>(e1);
    w->bn_g[k] = c.take<float>(size_t(kH + F));
    w->bn_t[k] = c.take<float>(size_t(kH + F));
    w->sim_g[k] = c.take<float>(kH);
    w->sim_t[k] = c.take<float>(kH);
    w->part[k] = reinterpret_cast<float*>(c.take<char>(spmm_ws_size(E[k] + N, kH)));
  }
  w->z1 = c.take<float>(n * kLd);
  w->h1 = c.take<float>(n * kLd);
  w->z2 = c.take<float>(n * kLd);
  w->h2 = c.take<float>(n * kLd);
  w->seg = c.take<int32_t>(nb + 2);
  w->scratch = c.take<int32_t>(4);
  w->predw = c.take<int32_t>(nb);
  w->loss_row = c.take<float>(nb);
  w->gws_bytes = bgcn_graph_pair_workspace_size(E[0], E[1], N);
  w->gws = c.take<char>(w->gws_bytes);
  w->c2_bytes = bgcn_ebgcn_conv2_lin_workspace_size(N, B, F);
  w->c2ws = c.take<char>(w->c2_bytes);
  return align_up(c.off, 256);
}

bool sizes_ok(int64_t N, int64_t B, int64_t F, int64_t Etd, int64_t Ebu) {
  return N > 0 && B > 0 && F > 0 && Etd >= 0 && Ebu >= 0 && N < (int64_t(1) << 31) - 1 &&
         B < (int64_t(1) << 31) - 1 && F < (int64_t(1) << 31) && Etd + N < (int64_t(1) << 31) &&
         Ebu + N < (int64_t(1) << 31);
}

bool dir_complete(const bgcn_ebgcn_dir& d) {
  return d.conv1_w && d.conv1_b && d.conv2_w && d.conv2_b && d.bn1_weight && d.bn1_bias && d.bn1_mean &&
         d.bn1_var && d.sim_conv_w && d.sim_norm_weight && d.sim_norm_bias && d.sim_norm_mean && d.sim_norm_var &&
         d.sim_out_w && d.sim_out_b && d.fc1_w;
}

}  // namespace

int ebgcn_eval_impl(const bgcn_ebgcn_eval_args* a, void* ws, size_t ws_bytes, hipStream_t s) {
  BGCN_CHECK_ARG(a, "null args");
  const bgcn_batch& bt = a->batch;
  const int64_t N = bt.num_nodes, B = bt.num_graphs, F = a->in_feats, C = a->num_classes;
  const int64_t E[2] = {bt.td_num_edges, bt.bu_num_edges};
  BGCN_CHECK_ARG(sizes_ok(N, B, F, E[0], E[1]), "bad sizes");
  BGCN_CHECK_ARG(C >= 1 && C <= kMaxClasses, "num_classes must be in [1, 16]");
  BGCN_CHECK_ARG(a->edge_num >= 1 && a->edge_num <= 8, "edge_num must be in [1, 8]");
  BGCN_CHECK_ARG(a->degree_on == BGCN_DEGREE_ON_COL || a->degree_on == BGCN_DEGREE_ON_ROW,
                 "degree_on must be 0 (col) or 1 (row)");
  BGCN_CHECK_ARG(bt.td_droprate == 0.0 && bt.bu_droprate == 0.0,
                 "the evaluation step drops no edges (the test set's BiGraphDataset)");
  BGCN_CHECK_ARG(bt.x && bt.x_dtype == BGCN_DTYPE_F32, "the EBGCN evaluation step takes dense fp32 x");
  BGCN_CHECK_ARG(F % 4 == 0 && bt.ldx >= F && bt.ldx % 4 == 0, "bad in_feats / ldx");
  BGCN_CHECK_ARG(bt.batch && bt.rootindex, "null pointer");
  BGCN_CHECK_ARG((E[0] == 0 || bt.td_edge_index) && (E[1] == 0 || bt.bu_edge_index), "null edge_index");
  BGCN_CHECK_ARG(dir_complete(a->td) && dir_complete(a->bu) && a->fc_w && a->fc_b, "null parameter pointer");
  BGCN_CHECK_ARG(a->td.bn1_eps >= 0.f && a->td.sim_norm_eps >= 0.f && a->bu.bn1_eps >= 0.f &&
                     a->bu.sim_norm_eps >= 0.f, "eps must not be negative");
  BGCN_CHECK_ARG(a->loss && a->correct && a->status, "null pointer");
  BGCN_CHECK_ARG(a16(bt.x) && a16(a->fc_w) && a16(a->td.conv1_w) && a16(a->bu.conv1_w) && a16(a->td.conv2_w) &&
                     a16(a->bu.conv2_w) && a16(a->td.conv1_b) && a16(a->bu.conv1_b) && a16(a->td.conv2_b) &&
                     a16(a->bu.conv2_b),
                 "x, fc_w and the conv weights / biases must be 16-byte aligned");
  EvalWs w;
  Carve c(ws, ws_bytes);
  carve_eval(c, N, B, F, E, &w);
  BGCN_CHECK_ARG(ws && c.ok(), "workspace too small");

  const float* x = static_cast<const float*>(bt.x);
  const bgcn_ebgcn_dir* dir[2] = {&a->td, &a->bu};
  const int64_t* ei[2] = {bt.td_edge_index, bt.bu_edge_index};
  float* pred[2] = {a->td_edge_pred ? a->td_edge_pred : w.pred[0], a->bu_edge_pred ? a->bu_edge_pred : w.pred[1]};
  bool rew[2];
  for (int k = 0; k < 2; ++k) rew[k] = dir[k]->infer != 0 && E[k] > 0;

  FoldArgs fa{};
  for (int k = 0; k < 2; ++k) {
    const bgcn_ebgcn_dir& d = *dir[k];
    fa.j[2 * k] = FoldJob{d.bn1_weight, d.bn1_bias, d.bn1_mean, d.bn1_var, d.bn1_eps, kH + F, w.bn_g[k], w.bn_t[k]};
    fa.j[2 * k + 1] = FoldJob{d.sim_norm_weight, d.sim_norm_bias, d.sim_norm_mean, d.sim_norm_var, d.sim_norm_eps,
                              kH, w.sim_g[k], w.sim_t[k]};
  }
  fa.status = a->status;
  hipLaunchKernelGGL(k_eval_fold, dim3(grid_for(kH + F, 256), 4), dim3(256), 0, s, fa);
  BGCN_CHECK_LAUNCH();

  // the structure of both directions and conv1's values, once
  GraphArgs ga[2];
  graph_pair_args(ei[0], E[0], ei[1], E[1], &w.csr[0], &w.csr[1], a->status, w.gws, w.gws_bytes, ga);
  BGCN_TRY(build_graphs_impl(ga, 2, N, a->degree_on, s, nullptr));
  SpmmPlan plan[2][2];
  graph_pair_plans(w.gws, w.gws_bytes, E[0], E[1], N, plan[0], plan[1]);
  const int64_t Emax = std::max(E[0], E[1]);
  if (rew[0] || rew[1]) {
    GraphBatch gb;
    size_t zero_bytes[kMaxGraphs];
    BGCN_TRY(graph_batch_setup(ga, 2, N, a->degree_on, &gb, zero_bytes, nullptr));
    SlotArgs sa{{w.slot[0], w.slot[1]}, {w.eid[0], w.eid[1]}};
    hipLaunchKernelGGL(k_eval_slots, dim3(grid_for(Emax, 256), 2), dim3(256), 0, s, gb, sa);
    BGCN_CHECK_LAUNCH();
  }
  BGCN_TRY(seg_bounds_impl(bt.batch, N, B, w.seg, w.scratch, s));

  // conv1, both directions: Z1 = X [W1_td; W1_bu]^T, H1 = A Z1 + b1
  BGCN_TRY(gemm_xwt_impl(x, bt.ldx, a->td.conv1_w, a->bu.conv1_w, F, kH, w.z1, kLd, N, kLd, F, s, nullptr));
  SpmmBatch sb{};
  sb.rows = N;
  sb.F = kH;
  sb.epi = BGCN_EPI_NONE;
  for (int k = 0; k < 2; ++k) {
    const bgcn_csr_out& g = w.csr[k];
    sb.p[k] = SpmmProb{g.t_ptr, g.t_row, g.t_col, g.t_w, w.z1 + kH * k, kLd, w.h1 + kH * k, kLd, dir[k]->conv1_b,
                       w.part[k], spmm_groups(E[k] + N, kH), E[k] + N, plan[k][0]};
  }
  BGCN_TRY(spmm_batch_impl(sb, 2, s));

  for (int k = 0; k < 2; ++k) {
    const bgcn_ebgcn_dir& d = *dir[k];
    if (rew[k])
      BGCN_TRY(edge_infer_impl(w.h1 + kH * k, kLd, N, kH, ei[k], E[k], d.sim_conv_w, w.sim_g[k], w.sim_t[k],
                               d.sim_out_w, d.sim_out_b, d.fc1_w, a->edge_num, pred[k], a->status, s));
    // bn1 is skipped for a one-node batch (EBGCN.py:80)
    BGCN_TRY(conv2_lin_impl(w.h1 + kH * k, kLd, x, bt.ldx, bt.batch, bt.rootindex, N, B, F, kH, d.conv2_w,
                            N != 1 ? w.bn_g[k] : nullptr, N != 1 ? w.bn_t[k] : nullptr, w.z2 + kH * k, kLd,
                            a->status, w.c2ws, w.c2_bytes, s));
  }

  if (rew[0] || rew[1]) {
    ReweightArgs ra{};
    ra.N = N;
    for (int k = 0; k < 2; ++k) {
      const bgcn_csr_out& g = w.csr[k];
      ra.d[k] = Reweight{rew[k] ? 1 : 0, E[k], ei[k], pred[k],
                         a->degree_on == BGCN_DEGREE_ON_COL ? g.t_ptr : g.s_ptr, w.eid[k], g.t_ptr, w.slot[k],
                         w.dinv[k], w.t_w2[k]};
    }
    hipLaunchKernelGGL(k_eval_degree, dim3(grid_for(N, 256), 2), dim3(256), 0, s, ra);
    BGCN_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_eval_reweight, dim3(grid_for(Emax + N, 256), 2), dim3(256), 0, s, ra);
    BGCN_CHECK_LAUNCH();
  }

  // conv2's aggregation: H2 = relu(A' Z2 + b2)
  sb.epi = BGCN_EPI_RELU;
  for (int k = 0; k < 2; ++k) {
    sb.p[k].w = rew[k] ? w.t_w2[k] : w.csr[k].t_w;
    sb.p[k].in = w.z2 + kH * k;
    sb.p[k].out = w.h2 + kH * k;
    sb.p[k].bias = dir[k]->conv2_b;
  }
  BGCN_TRY(spmm_batch_impl(sb, 2, s));

  ReadoutArgs ro{w.h1, w.h2, bt.batch, bt.rootindex, w.seg, N, B, a->fc_w, a->fc_b, a->y, int(C),
                 a->logp, w.loss_row, w.predw, a->pred, a->status};
  hipLaunchKernelGGL(k_eval_readout, dim3(unsigned(B)), dim3(256), 0, s, ro);
  BGCN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_eval_finish2, dim3(1), dim3(256), 0, s, w.loss_row, w.predw, a->y, B, a->loss, a->correct);
  BGCN_CHECK_LAUNCH();
  return BGCN_OK;
}

}  // namespace bgcn

extern "C" size_t bgcn_ebgcn_eval_workspace_size(int64_t num_nodes, int64_t num_graphs, int64_t in_feats,
                                                 int64_t td_num_edges, int64_t bu_num_edges, int edge_num) {
  if (!bgcn::sizes_ok(num_nodes, num_graphs, in_feats, td_num_edges, bu_num_edges) || edge_num < 1 || edge_num > 8)
    return 0;
  bgcn::EvalWs w;
  bgcn::Carve c(nullptr, 0);
  const int64_t E[2] = {td_num_edges, bu_num_edges};
  return bgcn::carve_eval(c, num_nodes, num_graphs, in_feats, E, &w);
}

extern "C" int bgcn_ebgcn_eval_step(const bgcn_ebgcn_eval_args* args, void* workspace, size_t workspace_bytes,
                                    bgcn_stream_t stream) {
  return bgcn::ebgcn_eval_impl(args, workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int bgcn_ebgcn_eval_saved(void* workspace, size_t workspace_bytes, int64_t num_nodes, int64_t num_graphs,
                                     int64_t in_feats, int64_t td_num_edges, int64_t bu_num_edges, int edge_num,
                                     int dir, bgcn_ebgcn_eval_view* out) {
  using namespace bgcn;
  BGCN_CHECK_ARG(sizes_ok(num_nodes, num_graphs, in_feats, td_num_edges, bu_num_edges), "bad sizes");
  BGCN_CHECK_ARG(edge_num >= 1 && edge_num <= 8, "edge_num must be in [1, 8]");
  BGCN_CHECK_ARG(out && (dir == 0 || dir == 1), "null pointer / dir must be 0 (TD) or 1 (BU)");
  EvalWs w;
  Carve c(workspace, workspace_bytes);
  const int64_t E[2] = {td_num_edges, bu_num_edges};
  carve_eval(c, num_nodes, num_graphs, in_feats, E, &w);
  BGCN_CHECK_ARG(workspace && c.ok(), "workspace too small");
  const bgcn_csr_out& g = w.csr[dir];
  *out = bgcn_ebgcn_eval_view{g.t_ptr, g.t_col, g.t_w, w.t_w2[dir], w.slot[dir]};
  return BGCN_OK;
}
