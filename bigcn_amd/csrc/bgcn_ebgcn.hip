// EBGCN (model/Twitter/EBGCN.py) in eval mode: the two pieces it adds over BiGCN.
//
// bgcn_edge_infer - TDrumorGCN.edge_infer / BUrumorGCN.edge_infer (EBGCN.py:95-116, :189-212)
// without the Bayesian branch, whose only product (the KL edge loss) the evaluation loop drops
// (EBGCN.py:338).  Per edge e, with a = h[(row_e - 1) mod N], b = h[(col_e - 1) mod N]:
//   D[c][l] = |a[c] - b[l]|                        x_ij = abs(x_i - x_j)            (:97-99)
//   Y[o][l] = sum_c Wc[o][c] D[c][l]               sim_valconv0 (Conv1d k = 1, no bias)
//   Z[o][l] = leaky_relu(g[o] Y[o][l] + t[o])      sim_valnorm0 (eval, folded) + LeakyReLU(0.01)
//   s[l]    = sum_o w_out[o] Z[o][l] + b_out       sim_valconv_out
//   p[k]    = sigmoid(sum_l fc1[k][l] s[l])        fc1 + sigmoid                    (:101-102)
//   edge_pred[e] = mean_k p[k]                                                      (:116)
// The "- 1" is the reference's `x[row - 1]` as written: node ids are used one lower than the
// edge list says, and id 0 reads the LAST node (Python's negative index).  It is reproduced
// here, not corrected.
//
// Y is a 64 x 64 x 64 product per edge (524,288 FLOP, ~16 GFLOP per direction at the reference
// batch).  It runs on the fp32 MFMA; the product and the epilogue on its accumulators (affine,
// leaky, the w_out sum over o) are bgcn_edge_tile.h's, shared with the training kernels of
// bgcn_ebgcn_train.hip; the fc1 sum over l follows here.  One wave per edge, a workgroup takes
// kEdgeTile edges; no atomics on floats, no scratch: an edge's bits depend on nothing but its
// own rows.
//
// bgcn_ebgcn_conv2_lin - conv2's lin (EBGCN.py:72-84) in eval mode:
//   z2[i] = relu(g_h . h1[i] + t_h) W2[:, :64]^T + r[batch[i]],
//   r[b]  = relu(g_x . x[rootindex[b]] + t_x) W2[:, 64:]^T
// with (g, t) the folded bn1 over the [64 + F] concat (NULL: bn1 skipped, the reference's
// one-node batch, :80).  The root block of the concat is the same row for every node of a
// tree, so its F-wide product is done once per tree (bgcn_gemm_xwt on a [B, F] table), not
// per node.  No dropout: the reference's EBGCN forward applies none.
#include "bgcn_edge_tile.h"
#include "bgcn_internal.h"

namespace bgcn {
namespace {

constexpr int kEdgeTile = BGCN_EDGE_INFER_TILE;   // edges per workgroup: 4 waves x 8 edges
static_assert(kEdgeTile % 4 == 0, "one wave per edge, four waves per workgroup");

__global__ __launch_bounds__(256, 2) void k_edge_infer(
    const float* __restrict__ h, int64_t ldh, int64_t N, const int64_t* __restrict__ ei, int64_t E,
    const float* __restrict__ Wc, const float* __restrict__ g, const float* __restrict__ t,
    const float* __restrict__ wout, const float* __restrict__ bout, const float* __restrict__ fc1, int K,
    float* __restrict__ pred, int32_t* __restrict__ status) {
  __shared__ float sW[kH * kWLd];
  __shared__ __attribute__((aligned(16))) float sG[kH];
  __shared__ __attribute__((aligned(16))) float sT[kH];
  __shared__ __attribute__((aligned(16))) float sO[kH];
  __shared__ float sF[kMaxEdgeNum * kH];
  const int tid = threadIdx.x;
  stage_w(Wc, sW);
  if (tid < kH) {
    sG[tid] = g[tid];
    sT[tid] = t[tid];
    sO[tid] = wout[tid];
  }
  for (int i = tid; i < K * kH; i += 256) sF[i] = fc1[i];
  __syncthreads();
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), r32 = lane & 31, hh = lane >> 5;
  float wa[2][32];
  load_wa(sW, r32, hh, wa);
  const float bo = *bout;
  const float invK = 1.0f / float(K);

  const int64_t e0 = int64_t(blockIdx.x) * kEdgeTile + wave;
  for (int i = 0; i < kEdgeTile / 4; ++i) {
    const int64_t e = e0 + 4 * i;
    if (e >= E) break;
    int64_t ia, ib;
    if (!edge_ends(ei, E, N, e, ia, ib)) {
      if (lane == 0) {
        atomicOr(status, 1);
        pred[e] = 0.f;
      }
      continue;
    }
    const float av = h[ia * ldh + lane];
    const float b0 = h[ib * ldh + r32], b1 = h[ib * ldh + 32 + r32];
    f32x16 acc[2][2];
    y_tile(wa, av, b0, b1, hh, acc);
    const float2 sv = edge_out_sums(acc, sG, sT, sO, hh);
    const float s0 = sv.x + bo, s1 = sv.y + bo;
    float sum = 0.f;
    for (int k = 0; k < K; ++k) {   // K is uniform: the shuffles stay convergent
      float p = fmaf(sF[k * kH + r32], s0, sF[k * kH + 32 + r32] * s1);
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) p += __shfl_xor(p, o);
      sum += 1.0f / (1.0f + expf(-p));
    }
    if (lane == 0) pred[e] = sum * invK;
  }
}

// eval-mode BatchNorm1d as one multiply-add: bn_fold of the running statistics
__global__ __launch_bounds__(256) void k_bn_fold(const float* __restrict__ gamma, const float* __restrict__ beta,
                                                 const float* __restrict__ mean, const float* __restrict__ var,
                                                 float eps, int64_t C, float* __restrict__ g, float* __restrict__ t) {
  const int64_t c = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (c >= C) return;
  bn_fold(gamma[c], beta[c], mean[c], var[c], eps, g[c], t[c]);
}

// out[i][4q ..] = relu(g . in[src(i)][4q ..] + t), src(i) = gather[i] (or i); C4 = C / 4
// float4 groups per row.  A gather index outside [0, src_rows) writes zeros and sets status bit 0.
__global__ __launch_bounds__(256) void k_affine_relu_rows(const float* __restrict__ in, int64_t ld_in,
                                                          const int64_t* __restrict__ gather, int64_t rows,
                                                          int64_t src_rows, int64_t C4, const float* __restrict__ g,
                                                          const float* __restrict__ t, float* __restrict__ out,
                                                          int64_t ld_out, int32_t* __restrict__ status) {
  const int64_t idx = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (idx >= rows * C4) return;
  const int64_t i = idx / C4, q = idx - i * C4;
  const int64_t src = gather ? gather[i] : i;
  float4 v = f4zero();
  if (src >= 0 && src < src_rows) {
    v = ld4(in + src * ld_in + 4 * q);
    if (g) v = f4affine(ld4(g + 4 * q), v, ld4(t + 4 * q));
    v = f4relu(v);
  } else if (q == 0) {
    atomicOr(status, 1);
  }
  st4(out + i * ld_out + 4 * q, v);
}

// z[i][:64] += r[batch[i]][:64]; a tree id outside [0, B) adds nothing and sets status bit 0
__global__ __launch_bounds__(256) void k_add_tree_rows(float* __restrict__ z, int64_t ldz, const float* __restrict__ r,
                                                       const int64_t* __restrict__ batch, int64_t N, int64_t B,
                                                       int32_t* __restrict__ status) {
  const int64_t idx = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (idx >= N * (kH / 4)) return;
  const int64_t i = idx >> 4;
  const int q = int(idx & 15);
  const int64_t b = batch[i];
  if (b < 0 || b >= B) {
    if (q == 0) atomicOr(status, 1);
    return;
  }
  float* p = z + i * ldz + 4 * q;
  st4(p, f4add(ld4(p), ld4(r + b * kH + 4 * q)));
}

struct Conv2LinWs {
  float* root;   // [B, F]  relu(bn1(x[rootindex]))
  float* act;    // [N, 64] relu(bn1(h1))
  float* r;      // [B, 64] root block of the product
};
size_t carve_conv2_lin(Carve& c, int64_t N, int64_t B, int64_t F, Conv2LinWs* w) {
  w->root = c.take<float>(size_t(B) * size_t(F));
  w->act = c.take<float>(size_t(N) * kH);
  w->r = c.take<float>(size_t(B) * kH);
  return align_up(c.off, 256);
}

}  // namespace

int edge_infer_impl(const float* h, int64_t ldh, int64_t N, int64_t hid, const int64_t* ei, int64_t E,
                    const float* Wc, const float* g, const float* t, const float* wout, const float* bout,
                    const float* fc1, int32_t K, float* pred, int32_t* status, hipStream_t s) {
  BGCN_CHECK_ARG(hid == kH, "edge_infer: the hidden size must be 64");
  BGCN_CHECK_ARG(K >= 1 && K <= kMaxEdgeNum, "edge_infer: edge_num must be in [1, 8]");
  BGCN_CHECK_ARG(N > 0 && E >= 0 && ldh >= kH, "edge_infer: bad shape");
  BGCN_CHECK_ARG(E < (int64_t(1) << 31) * kEdgeTile, "edge_infer: too many edges");
  BGCN_CHECK_ARG(h && Wc && g && t && wout && bout && fc1 && status, "edge_infer: null pointer");
  if (E == 0) return BGCN_OK;
  BGCN_CHECK_ARG(ei && pred, "edge_infer: null pointer");
  hipLaunchKernelGGL(k_edge_infer, dim3(grid_for(E, kEdgeTile)), dim3(256), 0, s, h, ldh, N, ei, E, Wc, g, t, wout,
                     bout, fc1, int(K), pred, status);
  BGCN_CHECK_LAUNCH();
  return BGCN_OK;
}

int bn_fold_impl(const float* gamma, const float* beta, const float* mean, const float* var, float eps, int64_t C,
                 float* g, float* t, hipStream_t s) {
  BGCN_CHECK_ARG(C > 0 && C < (int64_t(1) << 31), "bn_fold: bad channel count");
  BGCN_CHECK_ARG(eps >= 0.f, "bn_fold: eps must not be negative");
  BGCN_CHECK_ARG(gamma && beta && mean && var && g && t, "bn_fold: null pointer");
  hipLaunchKernelGGL(k_bn_fold, dim3(grid_for(C, 256)), dim3(256), 0, s, gamma, beta, mean, var, eps, C, g, t);
  BGCN_CHECK_LAUNCH();
  return BGCN_OK;
}

int conv2_lin_impl(const float* h1, int64_t ldh, const float* x, int64_t ldx, const int64_t* batch,
                   const int64_t* rootindex, int64_t N, int64_t B, int64_t F, int64_t hid, const float* w2,
                   const float* g, const float* t, float* z2, int64_t ldz, int32_t* status, void* ws, size_t ws_bytes,
                   hipStream_t s) {
  BGCN_CHECK_ARG(hid == kH, "conv2_lin: the hidden size must be 64");
  BGCN_CHECK_ARG(F > 0 && F % 4 == 0, "conv2_lin: in_feats must be a positive multiple of 4");
  BGCN_CHECK_ARG(N > 0 && B > 0, "conv2_lin: need N > 0 and B > 0");
  BGCN_CHECK_ARG(N * (F / 4 + 16) < (int64_t(1) << 38) && B * (F / 4) < (int64_t(1) << 38), "conv2_lin: batch too large");
  BGCN_CHECK_ARG(ldh >= kH && ldh % 4 == 0 && ldx >= F && ldx % 4 == 0 && ldz >= kH && ldz % 4 == 0,
                 "conv2_lin: leading dimensions must be multiples of 4 and cover the rows");
  BGCN_CHECK_ARG(h1 && x && batch && rootindex && w2 && z2 && status, "conv2_lin: null pointer");
  BGCN_CHECK_ARG((g == nullptr) == (t == nullptr), "conv2_lin: bn1's g and t come together");
  BGCN_CHECK_ARG(a16(h1) && a16(x) && a16(w2) && a16(z2) && a16(g) && a16(t), "conv2_lin: pointers must be 16-byte aligned");
  Conv2LinWs w;
  Carve c(ws, ws_bytes);
  carve_conv2_lin(c, N, B, F, &w);
  BGCN_CHECK_ARG(ws && c.ok(), "conv2_lin: workspace too small");
  const int64_t ldw = kH + F;
  // the root block, once per tree: [B, F] table, then its F-wide product
  hipLaunchKernelGGL(k_affine_relu_rows, dim3(grid_for(B * (F / 4), 256)), dim3(256), 0, s, x, ldx, rootindex, B, N,
                     F / 4, g ? g + kH : nullptr, t ? t + kH : nullptr, w.root, F, status);
  BGCN_CHECK_LAUNCH();
  BGCN_TRY(gemm_xwt_impl(w.root, F, w2 + kH, nullptr, ldw, kH, w.r, kH, B, kH, F, s, nullptr));
  // conv1's columns of the concat, per node
  hipLaunchKernelGGL(k_affine_relu_rows, dim3(grid_for(N * (kH / 4), 256)), dim3(256), 0, s, h1, ldh,
                     static_cast<const int64_t*>(nullptr), N, N, int64_t(kH / 4), g, t, w.act, int64_t(kH), status);
  BGCN_CHECK_LAUNCH();
  BGCN_TRY(gemm_xwt_impl(w.act, kH, w2, nullptr, ldw, kH, z2, ldz, N, kH, kH, s, nullptr));
  hipLaunchKernelGGL(k_add_tree_rows, dim3(grid_for(N * (kH / 4), 256)), dim3(256), 0, s, z2, ldz, w.r, batch, N, B,
                     status);
  BGCN_CHECK_LAUNCH();
  return BGCN_OK;
}

}  // namespace bgcn

extern "C" int bgcn_edge_infer(const float* h, int64_t ldh, int64_t num_nodes, int64_t hid,
                               const int64_t* edge_index, int64_t num_edges, const float* conv_w,
                               const float* bn_g, const float* bn_t, const float* out_w, const float* out_b,
                               const float* fc1_w, int32_t edge_num, float* edge_pred, int32_t* status,
                               bgcn_stream_t stream) {
  return bgcn::edge_infer_impl(h, ldh, num_nodes, hid, edge_index, num_edges, conv_w, bn_g, bn_t, out_w, out_b,
                               fc1_w, edge_num, edge_pred, status, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int bgcn_bn_fold(const float* gamma, const float* beta, const float* running_mean,
                            const float* running_var, float eps, int64_t channels, float* g, float* t,
                            bgcn_stream_t stream) {
  return bgcn::bn_fold_impl(gamma, beta, running_mean, running_var, eps, channels, g, t,
                            reinterpret_cast<hipStream_t>(stream));
}

extern "C" size_t bgcn_ebgcn_conv2_lin_workspace_size(int64_t num_nodes, int64_t num_graphs, int64_t in_feats) {
  if (num_nodes < 0 || num_graphs < 0 || in_feats < 0) return 0;
  bgcn::Conv2LinWs w;
  bgcn::Carve c(nullptr, 0);
  return bgcn::carve_conv2_lin(c, num_nodes, num_graphs, in_feats, &w);
}

extern "C" int bgcn_ebgcn_conv2_lin(const float* h1, int64_t ldh, const float* x, int64_t ldx,
                                    const int64_t* batch, const int64_t* rootindex, int64_t num_nodes,
                                    int64_t num_graphs, int64_t in_feats, int64_t hid, const float* w2,
                                    const float* bn_g, const float* bn_t, float* z2, int64_t ldz, int32_t* status,
                                    void* workspace, size_t workspace_bytes, bgcn_stream_t stream) {
  return bgcn::conv2_lin_impl(h1, ldh, x, ldx, batch, rootindex, num_nodes, num_graphs, in_feats, hid, w2, bn_g,
                              bn_t, z2, ldz, status, workspace, workspace_bytes,
                              reinterpret_cast<hipStream_t>(stream));
}
