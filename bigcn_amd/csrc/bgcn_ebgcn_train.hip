// EBGCN edge inference in TRAINING mode (model/Twitter/EBGCN.py:95-116, :189-212): the five
// per-edge networks with batch-statistics BatchNorm, the Bayesian branch, the KL edge loss, and
// the backward through the sim network, fc1 and h.  include/bgcn.h states the mathematics.
//
// Per edge and network Y = Wc D is a 64 x 64 x 64 product on the fp32 MFMA, with D = |a - b^T|
// made in registers from the two 256-byte rows: bgcn_edge_tile.h has the product and the networks'
// epilogue, which k_edge_infer of bgcn_ebgcn.hip runs too.  Nothing [E, 64, 64] is ever stored:
// every pass that needs Y computes it again.
//
// Forward (grid.y = network for the two MFMA passes):
//   k_train_dbar      sum_{e,l} D[e][c][l] per block, valid-edge count, status     (no MFMA)
//   k_train_mu        mu0_n = Wc_n Dbar: the batch mean, from the partials in fp64
//   k_train_stats     sum (Y - mu0), sum (Y - mu0)^2 per channel and block         (MFMA)
//   k_train_stats_fin fp64 merge -> mu, biased / unbiased variance, folded affine
//   k_train_apply     out_n[e][l] = conv_out(leaky(bn(Y)))                         (MFMA)
//   k_train_combine   p, edge_pred, the Bayesian draw, p_y, the edge's KL term
//   k_train_loss      mean of the KL terms in a fixed order
// The variance is a two-pass one: the mean is known (exactly, up to rounding) before the pass
// that sums squares, so that pass sums squares of centred values; the small residual sum
// corrects both moments in fp64.
//
// Backward:
//   k_train_bwd_edge  dp, du, ds [E, 64]; block partials of d_fc1 and d_b_out
//   k_train_bwd_stats recompute 1: block partials of d_beta, d_gamma, d_w_out      (MFMA)
//   k_train_bwd_fin1  fixed-order sums of the partials above
//   k_train_bwd_dw    recompute 2a: Y^T -> dY^T -> d_Wc^T += D dY^T                (MFMA)
//   k_train_bwd_finw  fixed-order sum of the d_Wc partials
//   k_train_bwd_dd    recompute 2b: Y -> dY -> dD = Wc^T dY -> d_a, d_b per edge   (MFMA)
//   k_train_dh_*      counting sort of the 2E (node, edge end) pairs, entries ranked by
//                     id inside each node's segment (through LDS), then one ordered sum per node
// The second recompute pass is two kernels: d_Wc wants dY with the channel on the lanes, dD
// wants it with the channel on the registers; each form comes straight out of the MFMA by
// swapping its operands, and one kernel holding both would need 320 accumulator registers.
// No float atomics: every cross-block sum goes through per-block partials and a fixed-order
// second step, so two runs give the same bits.
#include "bgcn_edge_tile.h"
#include "bgcn_internal.h"

namespace bgcn {
namespace {

constexpr int kTile = 32;           // edges per tile: 4 waves x 8 edges
constexpr int kNets = 5;            // sim, W_mean, W_bias, B_mean, B_bias
constexpr int kMaxBlocks = 512;     // blocks of a pass (each walks tiles b, b + grid, ...)
constexpr int kMaxBlocksW = 256;    // blocks of the d_Wc pass (a 16 KB partial each)

struct NetW {
  const float* w[kNets];
};

__device__ __forceinline__ float half_sum(float v) {   // over the 32 lanes that share hh
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float sgn(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }

// ------------------------------------------------------------------------------- forward
__global__ __launch_bounds__(256) void k_train_dbar(const float* __restrict__ h, int64_t ldh, int64_t N,
                                                    const int64_t* __restrict__ ei, int64_t E, int64_t tiles,
                                                    float* __restrict__ part_d, int32_t* __restrict__ part_cnt,
                                                    int32_t* __restrict__ status) {
  __shared__ float sD[4][kH];
  __shared__ int sC[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float acc = 0.f;
  int cnt = 0;
  bool bad = false;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x)
    for (int i = 0; i < kTile / 4; ++i) {
      const int64_t e = tile * kTile + wave + 4 * i;
      if (e >= E) break;
      int64_t ia, ib;
      if (!edge_ends(ei, E, N, e, ia, ib)) {
        bad = true;
        continue;
      }
      ++cnt;
      const float av = h[ia * ldh + lane], bv = h[ib * ldh + lane];
      float t = 0.f;
#pragma unroll 16
      for (int l = 0; l < kH; ++l) t += fabsf(av - __shfl(bv, l));
      acc += t;
    }
  if (bad && lane == 0) atomicOr(status, 1);
  sD[wave][lane] = acc;
  if (lane == 0) sC[wave] = cnt;
  __syncthreads();
  if (threadIdx.x < kH) {
    const int c = threadIdx.x;
    part_d[int64_t(blockIdx.x) * kH + c] = ((sD[0][c] + sD[1][c]) + sD[2][c]) + sD[3][c];
  }
  if (threadIdx.x == 0) part_cnt[blockIdx.x] = sC[0] + sC[1] + sC[2] + sC[3];
}

// mu0[n][o] = sum_c Wc_n[o][c] Dbar[c]; 320 threads
__global__ __launch_bounds__(320) void k_train_mu(const float* __restrict__ part_d, const int32_t* __restrict__ part_cnt,
                                                  int G, NetW nets, float* __restrict__ mu0,
                                                  int32_t* __restrict__ num_valid) {
  __shared__ double sD[kH];
  __shared__ int sN;
  const int tid = threadIdx.x;
  if (tid < kH) {
    double a = 0.0;
    for (int g = 0; g < G; ++g) a += double(part_d[int64_t(g) * kH + tid]);
    sD[tid] = a;
  }
  if (tid == kH) {
    int c = 0;
    for (int g = 0; g < G; ++g) c += part_cnt[g];
    sN = c;
    *num_valid = c;
  }
  __syncthreads();
  const int n = tid >> 6, o = tid & 63;
  const float* W = nets.w[n];
  double m = 0.0;
  for (int c = 0; c < kH; ++c) m += double(W[o * kH + c]) * sD[c];
  mu0[tid] = sN > 0 ? float(m / (64.0 * double(sN))) : 0.f;
}

__global__ __launch_bounds__(256, 2) void k_train_stats(const float* __restrict__ h, int64_t ldh, int64_t N,
                                                        const int64_t* __restrict__ ei, int64_t E, int64_t tiles,
                                                        NetW nets, const float* __restrict__ mu0,
                                                        float* __restrict__ pS, float* __restrict__ pQ) {
  __shared__ float sW[kH * kWLd];
  __shared__ __attribute__((aligned(16))) float sM[kH];
  __shared__ float sRS[4][kH];
  __shared__ float sRQ[4][kH];
  const int tid = threadIdx.x, n = blockIdx.y;
  stage_w(nets.w[n], sW);
  if (tid < kH) sM[tid] = mu0[n * kH + tid];
  __syncthreads();
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), r32 = lane & 31, hh = lane >> 5;
  float wa[2][32];
  load_wa(sW, r32, hh, wa);
  float S[2][16], Q[2][16];
#pragma unroll
  for (int tt = 0; tt < 2; ++tt)
#pragma unroll
    for (int r = 0; r < 16; ++r) S[tt][r] = Q[tt][r] = 0.f;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x)
    for (int i = 0; i < kTile / 4; ++i) {
      const int64_t e = tile * kTile + wave + 4 * i;
      if (e >= E) break;
      int64_t ia, ib;
      if (!edge_ends(ei, E, N, e, ia, ib)) continue;
      const float av = h[ia * ldh + lane];
      const float b0 = h[ib * ldh + r32], b1 = h[ib * ldh + 32 + r32];
      f32x16 acc[2][2];
      y_tile(wa, av, b0, b1, hh, acc);
#pragma unroll
      for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 M = *reinterpret_cast<const float4*>(&sM[32 * tt + 8 * q + 4 * hh]);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float m = f4at(M, j);
            const float d0 = acc[tt][0][4 * q + j] - m, d1 = acc[tt][1][4 * q + j] - m;
            S[tt][4 * q + j] += d0 + d1;
            Q[tt][4 * q + j] = fmaf(d0, d0, fmaf(d1, d1, Q[tt][4 * q + j]));
          }
        }
    }
#pragma unroll
  for (int tt = 0; tt < 2; ++tt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float s = half_sum(S[tt][r]), q = half_sum(Q[tt][r]);
      if (r32 == 0) {
        const int o = 32 * tt + 8 * (r >> 2) + 4 * hh + (r & 3);
        sRS[wave][o] = s;
        sRQ[wave][o] = q;
      }
    }
  __syncthreads();
  if (tid < kH) {
    const int64_t at = (int64_t(n) * gridDim.x + blockIdx.x) * kH + tid;
    pS[at] = ((sRS[0][tid] + sRS[1][tid]) + sRS[2][tid]) + sRS[3][tid];
    pQ[at] = ((sRQ[0][tid] + sRQ[1][tid]) + sRQ[2][tid]) + sRQ[3][tid];
  }
}

struct NetNorm {
  const float* gamma[kNets];
  const float* beta[kNets];
  float eps[kNets];
};

// grid 5 x 64 threads: the batch statistics of network n, channel o
__global__ __launch_bounds__(64) void k_train_stats_fin(const float* __restrict__ pS, const float* __restrict__ pQ, int G,
                                                        const float* __restrict__ mu0,
                                                        const int32_t* __restrict__ num_valid, NetNorm nn,
                                                        float* __restrict__ batch_mean, float* __restrict__ batch_var,
                                                        float* __restrict__ fold_g, float* __restrict__ fold_t,
                                                        float* __restrict__ sim_mean, float* __restrict__ sim_rstd) {
  const int n = blockIdx.x, o = threadIdx.x;
  double S = 0.0, Q = 0.0;
  for (int g = 0; g < G; ++g) {
    S += double(pS[(int64_t(n) * G + g) * kH + o]);
    Q += double(pQ[(int64_t(n) * G + g) * kH + o]);
  }
  const double cnt = 64.0 * double(*num_valid);
  double mean = 0.0, var = 0.0, unb = 0.0;
  if (cnt > 0.0) {
    const double d = S / cnt;
    mean = double(mu0[n * kH + o]) + d;
    var = Q / cnt - d * d;
    if (var < 0.0) var = 0.0;
    unb = var * cnt / (cnt - 1.0);
  }
  const double rstd = 1.0 / sqrt(var + double(nn.eps[n]));
  const float g = float(double(nn.gamma[n][o]) * rstd);
  batch_mean[n * kH + o] = float(mean);
  batch_var[n * kH + o] = float(unb);
  fold_g[n * kH + o] = g;
  fold_t[n * kH + o] = float(double(nn.beta[n][o]) - mean * double(nn.gamma[n][o]) * rstd);
  if (n == 0) {
    sim_mean[o] = float(mean);
    sim_rstd[o] = float(rstd);
  }
}

struct NetOut {
  const float* w[kNets];
  const float* b[kNets];
};

// out_n[e][l] = sum_o w_out[o] leaky(g[o] Y[o][l] + t[o]) + b_out; network 0 writes s
__global__ __launch_bounds__(256, 2) void k_train_apply(const float* __restrict__ h, int64_t ldh, int64_t N,
                                                        const int64_t* __restrict__ ei, int64_t E, int64_t tiles,
                                                        NetW nets, NetOut no, const float* __restrict__ fold_g,
                                                        const float* __restrict__ fold_t, float* __restrict__ s_out,
                                                        float* __restrict__ outs) {
  __shared__ float sW[kH * kWLd];
  __shared__ __attribute__((aligned(16))) float sG[kH];
  __shared__ __attribute__((aligned(16))) float sT[kH];
  __shared__ __attribute__((aligned(16))) float sO[kH];
  const int tid = threadIdx.x, n = blockIdx.y;
  stage_w(nets.w[n], sW);
  if (tid < kH) {
    sG[tid] = fold_g[n * kH + tid];
    sT[tid] = fold_t[n * kH + tid];
    sO[tid] = no.w[n][tid];
  }
  __syncthreads();
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), r32 = lane & 31, hh = lane >> 5;
  float wa[2][32];
  load_wa(sW, r32, hh, wa);
  const float bo = *no.b[n];
  float* dst = n == 0 ? s_out : outs + int64_t(n - 1) * E * kH;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x)
    for (int i = 0; i < kTile / 4; ++i) {
      const int64_t e = tile * kTile + wave + 4 * i;
      if (e >= E) break;
      int64_t ia, ib;
      if (!edge_ends(ei, E, N, e, ia, ib)) {
        if (hh == 0) dst[e * kH + r32] = dst[e * kH + 32 + r32] = 0.f;
        continue;
      }
      const float av = h[ia * ldh + lane];
      const float b0 = h[ib * ldh + r32], b1 = h[ib * ldh + 32 + r32];
      f32x16 acc[2][2];
      y_tile(wa, av, b0, b1, hh, acc);
      const float2 sv = edge_out_sums(acc, sG, sT, sO, hh);
      if (hh == 0) {
        dst[e * kH + r32] = sv.x + bo;
        dst[e * kH + 32 + r32] = sv.y + bo;
      }
    }
}

// one wave per edge, lane = l
__global__ __launch_bounds__(256) void k_train_combine(const int64_t* __restrict__ ei, int64_t E, int64_t N,
                                                       const float* __restrict__ s_in, const float* __restrict__ outs,
                                                       const float* __restrict__ noise, const float* __restrict__ fc1,
                                                       const float* __restrict__ fc2, int K, float* __restrict__ pred,
                                                       float* __restrict__ p_out, float* __restrict__ py_out,
                                                       float* __restrict__ kl) {
  const int lane = threadIdx.x & 63;
  const int64_t e = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (e >= E) return;
  int64_t ia, ib;
  if (!edge_ends(ei, E, N, e, ia, ib)) {
    if (lane == 0) {
      pred[e] = 0.f;
      kl[e] = 0.f;
    }
    if (lane < K) p_out[e * K + lane] = py_out[e * K + lane] = 0.f;
    return;
  }
  const int64_t at = e * kH + lane, EH = E * kH;
  const float s = s_in[at];
  const float wm = outs[at], wb = outs[EH + at], bm = outs[2 * EH + at], bb = outs[3 * EH + at];
  const float mean = fmaf(wm, s, bm);
  const float sd = fmaxf(logf(fmaf(s * s, expf(wb), expf(bb))), 0.f);
  const float y = 1.0f / (1.0f + expf(-fmaf(sd, noise[at], mean)));
  float p[kMaxEdgeNum], q[kMaxEdgeNum];
  float psum = 0.f, pmax = -1e30f, qmax = -1e30f;
#pragma unroll
  for (int k = 0; k < kMaxEdgeNum; ++k) {
    p[k] = q[k] = 0.f;
    if (k < K) {   // K is uniform: the shuffles stay convergent
      const float u = wave_sum(fc1[k * kH + lane] * s);
      p[k] = 1.0f / (1.0f + expf(-u));
      q[k] = wave_sum(fc2[k * kH + lane] * y);
      psum += p[k];
      pmax = fmaxf(pmax, p[k]);
      qmax = fmaxf(qmax, q[k]);
    }
  }
  float pe = 0.f, qe = 0.f;
#pragma unroll
  for (int k = 0; k < kMaxEdgeNum; ++k)
    if (k < K) {
      pe += expf(p[k] - pmax);
      qe += expf(q[k] - qmax);
    }
  const float plse = pmax + logf(pe), qlse = qmax + logf(qe);
  float t = 0.f;
#pragma unroll
  for (int k = 0; k < kMaxEdgeNum; ++k)
    if (k < K) {
      const float lpy = q[k] - qlse, py = expf(lpy);
      t += py * (lpy - (p[k] - plse));
      if (lane == 0) {
        p_out[e * K + k] = p[k];
        py_out[e * K + k] = py;
      }
    }
  if (lane == 0) {
    pred[e] = psum / float(K);
    kl[e] = t;
  }
}

__global__ __launch_bounds__(256) void k_train_loss(const float* __restrict__ kl, int64_t E,
                                                    const int32_t* __restrict__ num_valid, float* __restrict__ loss) {
  __shared__ double sm[256];
  double a = 0.0;
  for (int64_t e = threadIdx.x; e < E; e += 256) a += double(kl[e]);
  sm[threadIdx.x] = a;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (int(threadIdx.x) < o) sm[threadIdx.x] += sm[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss = *num_valid > 0 ? float(sm[0] / double(*num_valid)) : 0.f;
}

// ------------------------------------------------------------------------------- backward
// one wave per edge, lane = l: ds[e][l]; block partials pf [G][8][64] (d_fc1) and pb [G][64]
__global__ __launch_bounds__(256) void k_train_bwd_edge(const int64_t* __restrict__ ei, int64_t E, int64_t N,
                                                        int64_t tiles, const float* __restrict__ s_in,
                                                        const float* __restrict__ p_in, const float* __restrict__ py_in,
                                                        const float* __restrict__ fc1, int K,
                                                        const float* __restrict__ d_pred, const float* __restrict__ d_loss,
                                                        const int32_t* __restrict__ num_valid, float* __restrict__ ds,
                                                        float* __restrict__ pf, float* __restrict__ pb) {
  __shared__ float sF[4][kMaxEdgeNum + 1][kH];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nv = *num_valid;
  const float gl = nv > 0 ? *d_loss / float(nv) : 0.f;
  const float invK = 1.0f / float(K);
  float f1[kMaxEdgeNum], facc[kMaxEdgeNum], bacc = 0.f;
#pragma unroll
  for (int k = 0; k < kMaxEdgeNum; ++k) {
    f1[k] = k < K ? fc1[k * kH + lane] : 0.f;
    facc[k] = 0.f;
  }
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x)
    for (int i = 0; i < kTile / 4; ++i) {
      const int64_t e = tile * kTile + wave + 4 * i;
      if (e >= E) break;
      int64_t ia, ib;
      if (!edge_ends(ei, E, N, e, ia, ib)) {
        ds[e * kH + lane] = 0.f;
        continue;
      }
      float p[kMaxEdgeNum], pmax = -1e30f;
#pragma unroll
      for (int k = 0; k < kMaxEdgeNum; ++k) {
        p[k] = k < K ? p_in[e * K + k] : 0.f;
        if (k < K) pmax = fmaxf(pmax, p[k]);
      }
      float pe = 0.f;
#pragma unroll
      for (int k = 0; k < kMaxEdgeNum; ++k)
        if (k < K) pe += expf(p[k] - pmax);
      const float dpe = d_pred[e] * invK, sv = s_in[e * kH + lane];
      float dsl = 0.f;
#pragma unroll
      for (int k = 0; k < kMaxEdgeNum; ++k)
        if (k < K) {
          const float sm = expf(p[k] - pmax) / pe;
          const float dp = fmaf(gl, sm - py_in[e * K + k], dpe);
          const float du = dp * p[k] * (1.0f - p[k]);
          facc[k] = fmaf(du, sv, facc[k]);
          dsl = fmaf(f1[k], du, dsl);
        }
      ds[e * kH + lane] = dsl;
      bacc += dsl;
    }
#pragma unroll
  for (int k = 0; k < kMaxEdgeNum; ++k) sF[wave][k][lane] = facc[k];
  sF[wave][kMaxEdgeNum][lane] = bacc;
  __syncthreads();
  for (int i = threadIdx.x; i < (kMaxEdgeNum + 1) * kH; i += 256) {
    const int k = i >> 6, l = i & 63;
    const float v = ((sF[0][k][l] + sF[1][k][l]) + sF[2][k][l]) + sF[3][k][l];
    if (k < kMaxEdgeNum)
      pf[(int64_t(blockIdx.x) * kMaxEdgeNum + k) * kH + l] = v;
    else
      pb[int64_t(blockIdx.x) * kH + l] = v;
  }
}

// the sim network's per-channel constants of the backward
struct SimBwd {
  const float* Wc;
  const float* gamma;
  const float* beta;
  const float* wout;
  const float* mean;
  const float* rstd;
};

// recompute 1: block partials p1 [G][3][64] of d_w_out, d_beta, d_gamma
// (three accumulator sets beside Wc and Y: at two blocks per CU it spilled 88 bytes per lane)
__global__ __launch_bounds__(256) void k_train_bwd_stats(const float* __restrict__ h, int64_t ldh, int64_t N,
                                                            const int64_t* __restrict__ ei, int64_t E, int64_t tiles,
                                                            SimBwd sb, const float* __restrict__ ds,
                                                            float* __restrict__ p1) {
  __shared__ float sW[kH * kWLd];
  __shared__ __attribute__((aligned(16))) float sC[5][kH];   // mu, rstd, gamma, beta, w_out
  __shared__ float sR[4][3][kH];
  const int tid = threadIdx.x;
  stage_w(sb.Wc, sW);
  if (tid < kH) {
    sC[0][tid] = sb.mean[tid];
    sC[1][tid] = sb.rstd[tid];
    sC[2][tid] = sb.gamma[tid];
    sC[3][tid] = sb.beta[tid];
    sC[4][tid] = sb.wout[tid];
  }
  __syncthreads();
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), r32 = lane & 31, hh = lane >> 5;
  float wa[2][32];
  load_wa(sW, r32, hh, wa);
  float A0[2][16], A1[2][16], A2[2][16];
#pragma unroll
  for (int tt = 0; tt < 2; ++tt)
#pragma unroll
    for (int r = 0; r < 16; ++r) A0[tt][r] = A1[tt][r] = A2[tt][r] = 0.f;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x)
    for (int i = 0; i < kTile / 4; ++i) {
      const int64_t e = tile * kTile + wave + 4 * i;
      if (e >= E) break;
      int64_t ia, ib;
      if (!edge_ends(ei, E, N, e, ia, ib)) continue;
      const float av = h[ia * ldh + lane];
      const float b0 = h[ib * ldh + r32], b1 = h[ib * ldh + 32 + r32];
      const float ds0 = ds[e * kH + r32], ds1 = ds[e * kH + 32 + r32];
      f32x16 acc[2][2];
      y_tile(wa, av, b0, b1, hh, acc);
#pragma unroll
      for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int o0 = 32 * tt + 8 * q + 4 * hh;
          const float4 Mu = *reinterpret_cast<const float4*>(&sC[0][o0]);
          const float4 Rs = *reinterpret_cast<const float4*>(&sC[1][o0]);
          const float4 Ga = *reinterpret_cast<const float4*>(&sC[2][o0]);
          const float4 Be = *reinterpret_cast<const float4*>(&sC[3][o0]);
          const float4 Wo = *reinterpret_cast<const float4*>(&sC[4][o0]);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int r = 4 * q + j;
            const float mu = f4at(Mu, j), rs = f4at(Rs, j), ga = f4at(Ga, j), be = f4at(Be, j), wo = f4at(Wo, j);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
              const float dsl = u ? ds1 : ds0;
              const float yh = (acc[tt][u][r] - mu) * rs;
              const float pre = fmaf(ga, yh, be);
              const bool pos = pre > 0.f;
              const float z = pos ? pre : kSlope * pre;
              const float dA = wo * dsl * (pos ? 1.0f : kSlope);
              A0[tt][r] = fmaf(dsl, z, A0[tt][r]);
              A1[tt][r] += dA;
              A2[tt][r] = fmaf(dA, yh, A2[tt][r]);
            }
          }
        }
    }
#pragma unroll
  for (int tt = 0; tt < 2; ++tt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float a0 = half_sum(A0[tt][r]), a1 = half_sum(A1[tt][r]), a2 = half_sum(A2[tt][r]);
      if (r32 == 0) {
        const int o = 32 * tt + 8 * (r >> 2) + 4 * hh + (r & 3);
        sR[wave][0][o] = a0;
        sR[wave][1][o] = a1;
        sR[wave][2][o] = a2;
      }
    }
  __syncthreads();
  if (tid < 3 * kH) {
    const int k = tid >> 6, o = tid & 63;
    p1[(int64_t(blockIdx.x) * 3 + k) * kH + o] = ((sR[0][k][o] + sR[1][k][o]) + sR[2][k][o]) + sR[3][k][o];
  }
}

// fixed-order sums of the partials: d_w_out, d_beta, d_gamma, d_fc1, d_b_out; one block
__global__ __launch_bounds__(256) void k_train_bwd_fin1(const float* __restrict__ p1, const float* __restrict__ pf,
                                                        const float* __restrict__ pb, int G, int K,
                                                        float* __restrict__ d_wout, float* __restrict__ d_beta,
                                                        float* __restrict__ d_gamma, float* __restrict__ d_fc1,
                                                        float* __restrict__ d_bout) {
  __shared__ double sB[kH];
  const int tid = threadIdx.x;
  if (tid < 3 * kH) {
    const int k = tid >> 6, o = tid & 63;
    double a = 0.0;
    for (int g = 0; g < G; ++g) a += double(p1[(int64_t(g) * 3 + k) * kH + o]);
    (k == 0 ? d_wout : k == 1 ? d_beta : d_gamma)[o] = float(a);
  } else {
    const int l = tid - 3 * kH;
    double a = 0.0;
    for (int g = 0; g < G; ++g) a += double(pb[int64_t(g) * kH + l]);
    sB[l] = a;
  }
  for (int i = tid; i < K * kH; i += 256) {
    const int k = i >> 6, l = i & 63;
    double a = 0.0;
    for (int g = 0; g < G; ++g) a += double(pf[(int64_t(g) * kMaxEdgeNum + k) * kH + l]);
    d_fc1[i] = float(a);
  }
  __syncthreads();
  if (tid == 0) {
    double a = 0.0;
    for (int l = 0; l < kH; ++l) a += sB[l];
    *d_bout = float(a);
  }
}

// recompute 2a: Y^T -> dY^T; d_Wc^T[c][o] += sum_l D[c][l] dY[o][l]; block partials pW [G][64 o][64 c]
__global__ __launch_bounds__(256) void k_train_bwd_dw(const float* __restrict__ h, int64_t ldh, int64_t N,
                                                      const int64_t* __restrict__ ei, int64_t E, int64_t tiles,
                                                      SimBwd sb, const float* __restrict__ d_beta,
                                                      const float* __restrict__ d_gamma,
                                                      const int32_t* __restrict__ num_valid, const float* __restrict__ ds,
                                                      float* __restrict__ pW) {
  __shared__ float sW[kH * kWLd];
  const int tid = threadIdx.x;
  stage_w(sb.Wc, sW);
  __syncthreads();
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), r32 = lane & 31, hh = lane >> 5;
  float wa[2][32];
  load_wa(sW, r32, hh, wa);
  __syncthreads();   // sW is reused for the cross-wave sum below
  const int nv = *num_valid;
  const float inv_n = nv > 0 ? 1.0f / (64.0f * float(nv)) : 0.f;
  // per-lane channel constants: o = 32 tt + r32
  float mu[2], rs[2], ga[2], be[2], c1[2], c2[2], c3[2];
#pragma unroll
  for (int tt = 0; tt < 2; ++tt) {
    const int o = 32 * tt + r32;
    mu[tt] = sb.mean[o];
    rs[tt] = sb.rstd[o];
    ga[tt] = sb.gamma[o];
    be[tt] = sb.beta[o];
    const float gr = ga[tt] * rs[tt];
    c1[tt] = gr * sb.wout[o];
    c2[tt] = gr * d_beta[o] * inv_n;
    c3[tt] = gr * d_gamma[o] * inv_n;
  }
  f32x16 accW[2][2];   // [t2][tt][r] = d_Wc[o = 32 tt + r32][c = 32 t2 + 8 (r >> 2) + 4 hh + (r & 3)]
  zero_acc(accW);
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x)
    for (int i = 0; i < kTile / 4; ++i) {
      const int64_t e = tile * kTile + wave + 4 * i;
      if (e >= E) break;
      int64_t ia, ib;
      if (!edge_ends(ei, E, N, e, ia, ib)) continue;
      const float av = h[ia * ldh + lane];
      const float b0 = h[ib * ldh + r32], b1 = h[ib * ldh + 32 + r32];
      const float a2[2] = {h[ia * ldh + r32], h[ia * ldh + 32 + r32]};
      f32x16 acc[2][2];
      yt_tile(wa, av, b0, b1, hh, acc);
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int l0 = 32 * u + 8 * q + 4 * hh;
          const float4 B4 = ld4(h + ib * ldh + l0);
          const float4 D4 = ld4(ds + e * kH + l0);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int r = 4 * q + j;
            const float bl = f4at(B4, j), dsl = f4at(D4, j);
            float dy[2];
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
              const float yh = (acc[tt][u][r] - mu[tt]) * rs[tt];
              const float sl = fmaf(ga[tt], yh, be[tt]) > 0.f ? 1.0f : kSlope;
              dy[tt] = c1[tt] * dsl * sl - c2[tt] - yh * c3[tt];
            }
            const float d0 = fabsf(a2[0] - bl), d1 = fabsf(a2[1] - bl);
            accW[0][0] = mfma32x32x2(d0, dy[0], accW[0][0]);
            accW[0][1] = mfma32x32x2(d0, dy[1], accW[0][1]);
            accW[1][0] = mfma32x32x2(d1, dy[0], accW[1][0]);
            accW[1][1] = mfma32x32x2(d1, dy[1], accW[1][1]);
          }
        }
    }
  // the four waves' sums, in wave order
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int at = (32 * tt + r32) * kH + 32 * t2 + 8 * (r >> 2) + 4 * hh + (r & 3);
            sW[at] = w == 0 ? accW[t2][tt][r] : sW[at] + accW[t2][tt][r];
          }
    }
    __syncthreads();
  }
  for (int i = tid; i < kH * kH; i += 256) pW[int64_t(blockIdx.x) * kH * kH + i] = sW[i];
}

__global__ __launch_bounds__(256) void k_train_bwd_finw(const float* __restrict__ pW, int G, float* __restrict__ d_wc) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  double a = 0.0;
  for (int g = 0; g < G; ++g) a += double(pW[int64_t(g) * kH * kH + i]);
  d_wc[i] = float(a);
}

// recompute 2b: Y -> dY; dD = Wc^T dY; the edge's d_a, d_b rows -> dab [E][2][64]
__global__ __launch_bounds__(256) void k_train_bwd_dd(const float* __restrict__ h, int64_t ldh, int64_t N,
                                                      const int64_t* __restrict__ ei, int64_t E, int64_t tiles,
                                                      SimBwd sb, const float* __restrict__ d_beta,
                                                      const float* __restrict__ d_gamma,
                                                      const int32_t* __restrict__ num_valid, const float* __restrict__ ds,
                                                      float* __restrict__ dab) {
  __shared__ float sW[kH * kWLd];
  __shared__ __attribute__((aligned(16))) float sC[7][kH];   // mu, rstd, gamma, beta, c1, c2, c3
  const int tid = threadIdx.x;
  stage_w(sb.Wc, sW);
  if (tid < kH) {
    const int nv = *num_valid;
    const float inv_n = nv > 0 ? 1.0f / (64.0f * float(nv)) : 0.f;
    const float gr = sb.gamma[tid] * sb.rstd[tid];
    sC[0][tid] = sb.mean[tid];
    sC[1][tid] = sb.rstd[tid];
    sC[2][tid] = sb.gamma[tid];
    sC[3][tid] = sb.beta[tid];
    sC[4][tid] = gr * sb.wout[tid];
    sC[5][tid] = gr * d_beta[tid] * inv_n;
    sC[6][tid] = gr * d_gamma[tid] * inv_n;
  }
  __syncthreads();
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), r32 = lane & 31, hh = lane >> 5;
  float wa[2][32];
  load_wa(sW, r32, hh, wa);
  // A operand of dD = Wc^T dY, its k steps in the accumulators' channel order:
  // wt[t2][16 tt + r] = Wc[o = 32 tt + 8 (r >> 2) + 4 hh + (r & 3)][c = 32 t2 + r32]
  float wt[2][32];
#pragma unroll
  for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        wt[t2][16 * tt + r] = sW[(32 * tt + 8 * (r >> 2) + 4 * hh + (r & 3)) * kWLd + 32 * t2 + r32];
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x)
    for (int i = 0; i < kTile / 4; ++i) {
      const int64_t e = tile * kTile + wave + 4 * i;
      if (e >= E) break;
      int64_t ia, ib;
      if (!edge_ends(ei, E, N, e, ia, ib)) continue;
      const float av = h[ia * ldh + lane];
      const float b0 = h[ib * ldh + r32], b1 = h[ib * ldh + 32 + r32];
      const float ds0 = ds[e * kH + r32], ds1 = ds[e * kH + 32 + r32];
      f32x16 acc[2][2];
      y_tile(wa, av, b0, b1, hh, acc);
      f32x16 accD[2][2];   // [t2][u][r] = dD[c = 32 t2 + 8 (r >> 2) + 4 hh + (r & 3)][l = 32 u + r32]
      zero_acc(accD);
#pragma unroll
      for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int o0 = 32 * tt + 8 * q + 4 * hh;
          const float4 Mu = *reinterpret_cast<const float4*>(&sC[0][o0]);
          const float4 Rs = *reinterpret_cast<const float4*>(&sC[1][o0]);
          const float4 Ga = *reinterpret_cast<const float4*>(&sC[2][o0]);
          const float4 Be = *reinterpret_cast<const float4*>(&sC[3][o0]);
          const float4 C1 = *reinterpret_cast<const float4*>(&sC[4][o0]);
          const float4 C2 = *reinterpret_cast<const float4*>(&sC[5][o0]);
          const float4 C3 = *reinterpret_cast<const float4*>(&sC[6][o0]);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int r = 4 * q + j;
            const float mu = f4at(Mu, j), rs = f4at(Rs, j), ga = f4at(Ga, j), be = f4at(Be, j);
            const float k1 = f4at(C1, j), k2 = f4at(C2, j), k3 = f4at(C3, j);
            float dy[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
              const float yh = (acc[tt][u][r] - mu) * rs;
              const float sl = fmaf(ga, yh, be) > 0.f ? 1.0f : kSlope;
              dy[u] = k1 * (u ? ds1 : ds0) * sl - k2 - yh * k3;
            }
            accD[0][0] = mfma32x32x2(wt[0][16 * tt + r], dy[0], accD[0][0]);
            accD[0][1] = mfma32x32x2(wt[0][16 * tt + r], dy[1], accD[0][1]);
            accD[1][0] = mfma32x32x2(wt[1][16 * tt + r], dy[0], accD[1][0]);
            accD[1][1] = mfma32x32x2(wt[1][16 * tt + r], dy[1], accD[1][1]);
          }
        }
      // d_a[c] = sum_l dD[c][l] sign(a[c] - b[l]),  d_b[l] = -sum_c dD[c][l] sign(a[c] - b[l])
      float da[32], db0 = 0.f, db1 = 0.f;
#pragma unroll
      for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 A4 = ld4(h + ia * ldh + 32 * t2 + 8 * q + 4 * hh);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int r = 4 * q + j;
            const float ac = f4at(A4, j);
            const float t0 = accD[t2][0][r] * sgn(ac - b0), t1 = accD[t2][1][r] * sgn(ac - b1);
            da[16 * t2 + r] = t0 + t1;
            db0 += t0;
            db1 += t1;
          }
        }
      float mine = 0.f;   // lane r32 keeps the sum of register m = r32
#pragma unroll
      for (int m = 0; m < 32; ++m) {
        const float v = half_sum(da[m]);
        mine = r32 == m ? v : mine;
      }
      db0 += __shfl_xor(db0, 32);
      db1 += __shfl_xor(db1, 32);
      const int c = 32 * (r32 >> 4) + 8 * ((r32 & 15) >> 2) + 4 * hh + (r32 & 3);
      dab[(e * 2 + 0) * kH + c] = mine;
      if (hh == 0) {
        dab[(e * 2 + 1) * kH + r32] = -db0;
        dab[(e * 2 + 1) * kH + 32 + r32] = -db1;
      }
    }
}

// ---- dh[i] = sum of the d_a / d_b rows whose shifted index is i, in entry order (entry 2 e +
// side: the row dab[2 e + side])
__global__ __launch_bounds__(256) void k_zero_i32(int32_t* __restrict__ p, int64_t n) {
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (i < n) p[i] = 0;
}
__global__ __launch_bounds__(256) void k_train_dh_count(const int64_t* __restrict__ ei, int64_t E, int64_t N,
                                                        int32_t* __restrict__ cnt) {
  const int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (e >= E) return;
  int64_t ia, ib;
  if (!edge_ends(ei, E, N, e, ia, ib)) return;
  atomicAdd(&cnt[ia], 1);
  atomicAdd(&cnt[ib], 1);
}
// exclusive scan of cnt [N] in place (cnt[N] = total) and a copy into cursor [N]; one block
__global__ __launch_bounds__(1024) void k_train_dh_scan(int32_t* __restrict__ cnt, int32_t* __restrict__ cursor, int64_t N) {
  __shared__ int32_t sm[1024];
  const int t = threadIdx.x;
  const int64_t per = (N + 1023) / 1024, beg = min<int64_t>(N, t * per), end = min<int64_t>(N, beg + per);
  int32_t s = 0;
  for (int64_t i = beg; i < end; ++i) s += cnt[i];
  sm[t] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int32_t v = t >= o ? sm[t - o] : 0;
    __syncthreads();
    sm[t] += v;
    __syncthreads();
  }
  int32_t run = sm[t] - s;
  for (int64_t i = beg; i < end; ++i) {
    const int32_t c = cnt[i];
    cnt[i] = run;
    cursor[i] = run;
    run += c;
  }
  if (t == 1023) cnt[N] = sm[1023];
}
__global__ __launch_bounds__(256) void k_train_dh_fill(const int64_t* __restrict__ ei, int64_t E, int64_t N,
                                                       int32_t* __restrict__ cursor, int32_t* __restrict__ ids) {
  const int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (e >= E) return;
  int64_t ia, ib;
  if (!edge_ends(ei, E, N, e, ia, ib)) return;
  ids[atomicAdd(&cursor[ia], 1)] = int32_t(2 * e);
  ids[atomicAdd(&cursor[ib], 1)] = int32_t(2 * e + 1);
}
// the cursor leaves a node's entries in any order: rank them by id.  One block per node; the
// segment goes through LDS in chunks of kRankChunk ids, so a hub of L entries costs L^2 / 256
// LDS compares per thread (a BU root of 3,000 edge ends: ~35k)
constexpr int kRankChunk = 1024;
__global__ __launch_bounds__(256) void k_train_dh_rank(const int32_t* __restrict__ ptr, const int32_t* __restrict__ ids,
                                                       int32_t* __restrict__ sorted) {
  __shared__ int32_t sI[kRankChunk];
  const int64_t i = blockIdx.x;
  const int32_t beg = ptr[i], len = ptr[i + 1] - beg;   // block-uniform
  const int t = threadIdx.x;
  for (int32_t jb = 0; jb < len; jb += 256) {
    const int32_t j = jb + t;
    const int32_t id = j < len ? ids[beg + j] : 0x7fffffff;
    int32_t r = 0;
    for (int32_t c0 = 0; c0 < len; c0 += kRankChunk) {
      const int32_t n = min(kRankChunk, len - c0);
      __syncthreads();
      for (int32_t k = t; k < n; k += 256) sI[k] = ids[beg + c0 + k];
      __syncthreads();
      for (int32_t k = 0; k < n; ++k) r += sI[k] < id ? 1 : 0;
    }
    if (j < len) sorted[beg + r] = id;
  }
}
// lane = column; the four waves take the segment's quarters, combined in wave order
__global__ __launch_bounds__(256) void k_train_dh_sum(const int32_t* __restrict__ ptr, const int32_t* __restrict__ sorted,
                                                      const float* __restrict__ dab, float* __restrict__ dh, int64_t ldd) {
  __shared__ float sA[4][kH];
  const int64_t i = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int32_t beg = ptr[i], len = ptr[i + 1] - beg;
  const int32_t q = (len + 3) / 4, b0 = min(len, wave * q), b1 = min(len, b0 + q);
  float acc = 0.f;
  int32_t j = b0;
  for (; j + 8 <= b1; j += 8) {   // eight rows in flight, added in entry order
    int32_t id[8];
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) id[u] = sorted[beg + j + u];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = dab[int64_t(id[u]) * kH + lane];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc += v[u];
  }
  for (; j < b1; ++j) acc += dab[int64_t(sorted[beg + j]) * kH + lane];
  sA[wave][lane] = acc;
  __syncthreads();
  if (wave == 0) dh[i * ldd + lane] = ((sA[0][lane] + sA[1][lane]) + sA[2][lane]) + sA[3][lane];
}

// ------------------------------------------------------------------------------- host
int64_t tiles_of(int64_t E) { return (E + kTile - 1) / kTile; }
int blocks_of(int64_t E, int cap) { return int(std::min<int64_t>(tiles_of(E), cap)); }

struct FwdWs {
  float *part_d, *mu0, *fold_g, *fold_t, *pS, *pQ, *outs, *kl;
  int32_t* part_cnt;
};
struct BwdWs {
  float *ds, *pf, *pb, *p1, *pW, *dab;
  int32_t *cnt, *cursor, *ids, *sorted;
};
size_t carve_fwd(Carve& c, int64_t E, FwdWs* w) {
  const size_t G = size_t(blocks_of(E, kMaxBlocks));
  w->part_d = c.take<float>(G * kH);
  w->part_cnt = c.take<int32_t>(G);
  w->mu0 = c.take<float>(kNets * kH);
  w->fold_g = c.take<float>(kNets * kH);
  w->fold_t = c.take<float>(kNets * kH);
  w->pS = c.take<float>(kNets * G * kH);
  w->pQ = c.take<float>(kNets * G * kH);
  w->outs = c.take<float>(size_t(kNets - 1) * size_t(E) * kH);
  w->kl = c.take<float>(size_t(E));
  return align_up(c.off, 256);
}
size_t carve_bwd(Carve& c, int64_t N, int64_t E, BwdWs* w) {
  const size_t G = size_t(blocks_of(E, kMaxBlocks)), GW = size_t(blocks_of(E, kMaxBlocksW));
  w->ds = c.take<float>(size_t(E) * kH);
  w->pf = c.take<float>(G * kMaxEdgeNum * kH);
  w->pb = c.take<float>(G * kH);
  w->p1 = c.take<float>(G * 3 * kH);
  w->pW = c.take<float>(GW * kH * kH);
  w->dab = c.take<float>(size_t(E) * 2 * kH);
  w->cnt = c.take<int32_t>(size_t(N) + 1);
  w->cursor = c.take<int32_t>(size_t(N));
  w->ids = c.take<int32_t>(size_t(E) * 2);
  w->sorted = c.take<int32_t>(size_t(E) * 2);
  return align_up(c.off, 256);
}

int check_shape(int64_t hid, int32_t K, int64_t N, int64_t E, int64_t ldh, const float* h) {
  BGCN_CHECK_ARG(hid == kH, "edge_infer_train: the hidden size must be 64");
  BGCN_CHECK_ARG(K >= 1 && K <= kMaxEdgeNum, "edge_infer_train: edge_num must be in [1, 8]");
  BGCN_CHECK_ARG(E > 0, "edge_infer_train: needs at least one edge");
  BGCN_CHECK_ARG(N > 0 && N < (int64_t(1) << 31) && E < (int64_t(1) << 30), "edge_infer_train: bad shape");
  BGCN_CHECK_ARG(ldh >= kH && ldh % 4 == 0 && h && a16(h), "edge_infer_train: h must be 16-byte aligned rows of 64");
  return BGCN_OK;
}

}  // namespace

int edge_infer_train_fwd_impl(const bgcn_edge_train_fwd_args* a, void* ws, size_t ws_bytes, hipStream_t s) {
  BGCN_CHECK_ARG(a, "edge_infer_train: null arguments");
  BGCN_TRY(check_shape(a->hid, a->edge_num, a->num_nodes, a->num_edges, a->ldh, a->h));
  NetW nw;
  NetNorm nn;
  NetOut no;
  for (int n = 0; n < kNets; ++n) {
    const bgcn_edge_net& t = a->net[n];
    BGCN_CHECK_ARG(t.conv_w && t.norm_weight && t.norm_bias && t.out_w && t.out_b, "edge_infer_train: null parameter pointer");
    BGCN_CHECK_ARG(t.eps >= 0.f, "edge_infer_train: eps must not be negative");
    nw.w[n] = t.conv_w;
    nn.gamma[n] = t.norm_weight;
    nn.beta[n] = t.norm_bias;
    nn.eps[n] = t.eps;
    no.w[n] = t.out_w;
    no.b[n] = t.out_b;
  }
  BGCN_CHECK_ARG(a->edge_index && a->fc1_w && a->fc2_w && a->noise, "edge_infer_train: null pointer");
  BGCN_CHECK_ARG(a->edge_pred && a->edge_loss && a->s && a->p && a->p_y && a->sim_mean && a->sim_rstd &&
                     a->num_valid && a->batch_mean && a->batch_var && a->status,
                 "edge_infer_train: null output pointer");
  const int64_t E = a->num_edges, N = a->num_nodes, tiles = tiles_of(E);
  FwdWs w;
  Carve c(ws, ws_bytes);
  carve_fwd(c, E, &w);
  BGCN_CHECK_ARG(ws && c.ok(), "edge_infer_train: workspace too small");
  const int G = blocks_of(E, kMaxBlocks);
  hipLaunchKernelGGL(k_train_dbar, dim3(G), dim3(256), 0, s, a->h, a->ldh, N, a->edge_index, E, tiles, w.part_d,
                     w.part_cnt, a->status);
  BGCN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_train_mu, dim3(1), dim3(320), 0, s, w.part_d, w.part_cnt, G, nw, w.mu0, a->num_valid);
  BGCN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_train_stats, dim3(G, kNets), dim3(256), 0, s, a->h, a->ldh, N, a->edge_index, E, tiles, nw,
                     w.mu0, w.pS, w.pQ);
  BGCN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_train_stats_fin, dim3(kNets), dim3(64), 0, s, w.pS, w.pQ, G, w.mu0, a->num_valid, nn,
                     a->batch_mean, a->batch_var, w.fold_g, w.fold_t, a->sim_mean, a->sim_rstd);
  BGCN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_train_apply, dim3(G, kNets), dim3(256), 0, s, a->h, a->ldh, N, a->edge_index, E, tiles, nw, no,
                     w.fold_g, w.fold_t, a->s, w.outs);
  BGCN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_train_combine, dim3(grid_for(E, 4)), dim3(256), 0, s, a->edge_index, E, N, a->s, w.outs,
                     a->noise, a->fc1_w, a->fc2_w, int(a->edge_num), a->edge_pred, a->p, a->p_y, w.kl);
  BGCN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_train_loss, dim3(1), dim3(256), 0, s, w.kl, E, a->num_valid, a->edge_loss);
  BGCN_CHECK_LAUNCH();
  return BGCN_OK;
}

int edge_infer_train_bwd_impl(const bgcn_edge_train_bwd_args* a, void* ws, size_t ws_bytes, hipStream_t s) {
  BGCN_CHECK_ARG(a, "edge_infer_train: null arguments");
  BGCN_TRY(check_shape(a->hid, a->edge_num, a->num_nodes, a->num_edges, a->ldh, a->h));
  const bgcn_edge_net& t = a->sim;
  BGCN_CHECK_ARG(t.conv_w && t.norm_weight && t.norm_bias && t.out_w, "edge_infer_train: null parameter pointer");
  BGCN_CHECK_ARG(a->edge_index && a->fc1_w && a->s && a->p && a->p_y && a->sim_mean && a->sim_rstd && a->num_valid &&
                     a->d_pred && a->d_loss,
                 "edge_infer_train: null pointer");
  BGCN_CHECK_ARG(a->d_h && a->d_conv_w && a->d_norm_weight && a->d_norm_bias && a->d_out_w && a->d_out_b && a->d_fc1_w,
                 "edge_infer_train: null gradient pointer");
  BGCN_CHECK_ARG(a->ldd >= kH, "edge_infer_train: d_h rows must hold 64 values");
  const int64_t E = a->num_edges, N = a->num_nodes, tiles = tiles_of(E);
  BwdWs w;
  Carve c(ws, ws_bytes);
  carve_bwd(c, N, E, &w);
  BGCN_CHECK_ARG(ws && c.ok(), "edge_infer_train: workspace too small");
  const int G = blocks_of(E, kMaxBlocks), GW = blocks_of(E, kMaxBlocksW), K = int(a->edge_num);
  const SimBwd sb{t.conv_w, t.norm_weight, t.norm_bias, t.out_w, a->sim_mean, a->sim_rstd};
  hipLaunchKernelGGL(k_train_bwd_edge, dim3(G), dim3(256), 0, s, a->edge_index, E, N, tiles, a->s, a->p, a->p_y,
                     a->fc1_w, K, a->d_pred, a->d_loss, a->num_valid, w.ds, w.pf, w.pb);
  BGCN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_train_bwd_stats, dim3(G), dim3(256), 0, s, a->h, a->ldh, N, a->edge_index, E, tiles, sb, w.ds,
                     w.p1);
  BGCN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_train_bwd_fin1, dim3(1), dim3(256), 0, s, w.p1, w.pf, w.pb, G, K, a->d_out_w, a->d_norm_bias,
                     a->d_norm_weight, a->d_fc1_w, a->d_out_b);
  BGCN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_train_bwd_dw, dim3(GW), dim3(256), 0, s, a->h, a->ldh, N, a->edge_index, E, tiles, sb,
                     a->d_norm_bias, a->d_norm_weight, a->num_valid, w.ds, w.pW);
  BGCN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_train_bwd_finw, dim3(kH * kH / 256), dim3(256), 0, s, w.pW, GW, a->d_conv_w);
  BGCN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_train_bwd_dd, dim3(G), dim3(256), 0, s, a->h, a->ldh, N, a->edge_index, E, tiles, sb,
                     a->d_norm_bias, a->d_norm_weight, a->num_valid, w.ds, w.dab);
  BGCN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_zero_i32, dim3(grid_for(N + 1, 256)), dim3(256), 0, s, w.cnt, N + 1);
  BGCN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_train_dh_count, dim3(grid_for(E, 256)), dim3(256), 0, s, a->edge_index, E, N, w.cnt);
  BGCN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_train_dh_scan, dim3(1), dim3(1024), 0, s, w.cnt, w.cursor, N);
  BGCN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_train_dh_fill, dim3(grid_for(E, 256)), dim3(256), 0, s, a->edge_index, E, N, w.cursor, w.ids);
  BGCN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_train_dh_rank, dim3(unsigned(N)), dim3(256), 0, s, w.cnt, w.ids, w.sorted);
  BGCN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_train_dh_sum, dim3(unsigned(N)), dim3(256), 0, s, w.cnt, w.sorted, w.dab, a->d_h, a->ldd);
  BGCN_CHECK_LAUNCH();
  return BGCN_OK;
}

size_t edge_infer_train_ws_size(int64_t N, int64_t E) {
  FwdWs f;
  BwdWs b;
  Carve cf(nullptr, 0), cb(nullptr, 0);
  return std::max(carve_fwd(cf, E, &f), carve_bwd(cb, N, E, &b));
}

}  // namespace bgcn

extern "C" size_t bgcn_edge_infer_train_workspace_size(int64_t num_nodes, int64_t num_edges) {
  if (num_nodes <= 0 || num_edges <= 0 || num_edges >= (int64_t(1) << 30)) return 0;
  return bgcn::edge_infer_train_ws_size(num_nodes, num_edges);
}

extern "C" int bgcn_edge_infer_train_fwd(const bgcn_edge_train_fwd_args* args, void* workspace, size_t workspace_bytes,
                                         bgcn_stream_t stream) {
  return bgcn::edge_infer_train_fwd_impl(args, workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int bgcn_edge_infer_train_bwd(const bgcn_edge_train_bwd_args* args, void* workspace, size_t workspace_bytes,
                                         bgcn_stream_t stream) {
  return bgcn::edge_infer_train_bwd_impl(args, workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream));
}
