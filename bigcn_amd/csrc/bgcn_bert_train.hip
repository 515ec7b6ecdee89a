// bgcn_bert_train_grad: one iteration of the TreeBERT baseline's training loop up to the optimiser
// (model/Twitter/BERT_Twitter.py:89-119: BertModel in training mode, mean NLL, accuracy, backward)
// for a whole batch of trees as one launch sequence on the caller's stream, everything in the
// caller's workspace.  Root-only by construction: position 0 attends to itself only, the pooler
// reads position 0 and dropout is element-wise, so the loss is a function of each tree's first row
// and the whole call is a chain on [B, hidden].  The gradient of a softmax over one unmasked key
// is exactly 0: no attention backward, zero q / k gradients.
//
// Dropout draw of (site, sequence b, j = column or head):
//   hash = mix32(mix32(mix32(b ^ lo32(seed)) ^ (site * 0x9E3779B9 + hi32(seed))) ^ (j * 0x85EBCA6B))
//   kept iff hash >= thr, thr = floor(p * 2^32 + 0.5) (p the fp32 rate, in double); a kept value is
//   multiplied by the fp32 1.0f / (1.0f - p).  Sites: 0 after the embeddings' LN; layer l: 3l + 1 the
//   attention probabilities (rate attn_dropout, j = head), 3l + 2 after attention.output.dense,
//   3l + 3 after output.dense (rate hidden_dropout, j = column).  Masks are regenerated in the
//   backward, never stored.
//
//   forward   bert_setup (k_bert_setup); k_bt_embed; per layer the products of bgcn_bert_eval's
//             root-only chain with k_bt_ctx (v + bias, the head's draw), k_bt_add_ln (dropout,
//             residual, LN; keeps the normalised row and 1 / sqrt(var + eps)), k_bt_inter (bias, the
//             pre-GELU value kept, GELU); bert_head (k_bert_head, seq_finish)
//   backward  k_bt_head_bwd (dz, pooled, d pooler output), k_bt_fc_grad (d fc, skip_flag), the pooler;
//             per layer L-1 .. 0: k_bt_ln_bwd, k_bt_colsum (d gamma, d beta, d bias), output.dense,
//             k_bt_gelu_bwd, intermediate.dense, k_bt_ln_bwd with the residual add,
//             attention.output.dense, k_bt_head_mask, value; k_bt_zero for q / k;
//             the embeddings' k_bt_ln_bwd, the column sums into row 0 of d position / d type,
//             k_bt_zero for their other rows, k_bt_dx_zero + k_bt_dx_roots
//   dW = dY^T X (reduction over the B rows, also B = 1), dX = dY W.
//
// The three products (Y = X W^T, dX = dY W, dW = dY^T X) are a policy the two entry points instantiate:
// TiledGemms (gemm_xwt_impl, gemm_xw2_impl, gemm_tn_impl: bgcn_bert_train_grad, whose forward has
// bgcn_bert_eval's bits) and SkinnyGemms (bgcn_gemm_skinny.hip: bgcn_bert_train_grad_skinny).  The row
// kernels and the launch order are one text.
//
// Stream order is the only dependency between the launches.  No float atomics; every sum has a
// fixed order.
#include <cmath>

#include "bgcn_bert.h"

namespace bgcn {
namespace {

struct Drop {
  uint64_t seed;
  uint32_t thr_h, thr_a;   // kept iff hash >= thr
  float scale_h, scale_a;
};
// the part of the hash shared by every j of one (site, b)
__device__ __forceinline__ uint32_t drop_base(uint64_t seed, uint32_t site, uint32_t b) {
  return mix32(mix32(b ^ uint32_t(seed)) ^ (site * 0x9E3779B9u + uint32_t(seed >> 32)));
}
__device__ __forceinline__ bool drop_keep(uint32_t base, uint32_t j, uint32_t thr) {
  return mix32(base ^ (j * 0x85EBCA6Bu)) >= thr;
}
__device__ __forceinline__ float drop_h(float v, uint32_t base, uint32_t j, const Drop& d) {
  return drop_keep(base, j, d.thr_h) ? v * d.scale_h : 0.f;
}

// ---- embeddings at position 0, one wave per sequence: h[b] = dropout(LN(x[start] + pos_emb[0] +
// type_emb)), xhat[b] the normalised row, inv[b]; an emptied sequence gets zeros in all three (its
// LN backward then gives zeros)
struct EmbedTArgs {
  const float* x;
  int64_t ldx;
  const float *pos_emb, *type_emb, *g, *be;
  SeqInfo sq;
  float *h, *xhat, *inv;   // [B, H], [B, H], [B]
  int64_t B;
  int H;
  float eps;
  Drop d;
};
__global__ __launch_bounds__(256) void k_bt_embed(EmbedTArgs a) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, H = a.H, per = H >> 6;
  const int64_t b = int64_t(blockIdx.x) * 4 + w;
  if (b >= a.B) return;
  float *dst = a.h + b * H, *xh = a.xhat + b * H;
  if (a.sq.len[b] == 0) {
    for (int c = l; c < H; c += kWave) dst[c] = xh[c] = 0.f;
    if (l == 0) a.inv[b] = 0.f;
    return;
  }
  const float* xr = a.x + int64_t(a.sq.start[b]) * a.ldx;
  float v[kMaxPer];
#pragma unroll
  for (int i = 0; i < kMaxPer; ++i)
    if (i < per) {
      const int c = l + kWave * i;
      v[i] = (xr[c] + a.pos_emb[c]) + a.type_emb[c];
    }
  const float inv = ln_row(v, per, H, a.g, a.be, a.eps, l, dst, nullptr);
  const uint32_t base = drop_base(a.d.seed, 0, uint32_t(b));
#pragma unroll
  for (int i = 0; i < kMaxPer; ++i)
    if (i < per) {
      const int c = l + kWave * i;
      xh[c] = v[i] * inv;
      dst[c] = drop_h(dst[c], base, c, a.d);   // the lane's own store of ln_row
    }
  if (l == 0) a.inv[b] = inv;
}

// ---- out[r] = LN(dropout(y[r] + bias) + res[r]), one wave per row (k_bert_add_ln with the draw of
// `site`); xhat[r] the normalised row, inv[r]
struct AddLnTArgs {
  const float *y, *bias, *res, *g, *be;
  float *out, *xhat, *inv;
  int64_t M;
  int H;
  float eps;
  Drop d;
  uint32_t site;
};
__global__ __launch_bounds__(256) void k_bt_add_ln(AddLnTArgs a) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, H = a.H, per = H >> 6;
  const int64_t r = int64_t(blockIdx.x) * 4 + w;
  if (r >= a.M) return;
  const float *y = a.y + r * H, *res = a.res + r * H;
  float* xh = a.xhat + r * H;
  const uint32_t base = drop_base(a.d.seed, a.site, uint32_t(r));
  float v[kMaxPer];
#pragma unroll
  for (int i = 0; i < kMaxPer; ++i)
    if (i < per) {
      const int c = l + kWave * i;
      v[i] = drop_h(y[c] + a.bias[c], base, c, a.d) + res[c];
    }
  const float inv = ln_row(v, per, H, a.g, a.be, a.eps, l, a.out + r * H, nullptr);
#pragma unroll
  for (int i = 0; i < kMaxPer; ++i)
    if (i < per) xh[l + kWave * i] = v[i] * inv;
  if (l == 0) a.inv[r] = inv;
}

// ---- ctx[b][c] = keep(site, b, head c / 64) (y[b][c] + bias[c]) / (1 - p_attn) in place over [M, H]
__global__ __launch_bounds__(256) void k_bt_ctx(float* __restrict__ y, const float* __restrict__ bias, int64_t total4,
                                                int C4, Drop d, uint32_t site) {
  for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < total4; i += int64_t(gridDim.x) * 256) {
    const int c = int(i % C4) * 4;
    const uint32_t b = uint32_t(i / C4);
    const float4 v = f4add(ld4(y + i * 4), ld4(bias + c));
    const float s = drop_keep(drop_base(d.seed, site, b), uint32_t(c) >> 6, d.thr_a) ? d.scale_a : 0.f;
    st4(y + i * 4, s != 0.f ? make_float4(v.x * s, v.y * s, v.z * s, v.w * s) : f4zero());
  }
}

// ---- m = m + bias in place (the pre-GELU value the backward reads), g = gelu(m), over [M, C]
__global__ __launch_bounds__(256) void k_bt_inter(float* __restrict__ m, const float* __restrict__ bias,
                                                  float* __restrict__ g, int64_t total4, int C4) {
  for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < total4; i += int64_t(gridDim.x) * 256) {
    const int c = int(i % C4) * 4;
    const float4 v = f4add(ld4(m + i * 4), ld4(bias + c));
    st4(m + i * 4, v);
    st4(g + i * 4, make_float4(gelu_erf(v.x), gelu_erf(v.y), gelu_erf(v.z), gelu_erf(v.w)));
  }
}

// ---- head backward, workgroup b = sequence b: dz = (softmax - onehot(y)) / B (zeros for a label
// outside [0, C): the head has flagged it), pooled = tanh(P + pooler bias) as k_bert_head computes
// it, dP = (dz W) (1 - pooled^2)
struct HeadBwdTArgs {
  const float *P, *pb, *W, *logp;   // [B, H], [H], [C, H], [B, C]
  const int64_t* y;
  int64_t B;
  int H, C;
  float *dz, *pooled, *dP;          // [B, C], [B, H], [B, H]
};
__global__ __launch_bounds__(256) void k_bt_head_bwd(HeadBwdTArgs a) {
  __shared__ float dzs[kMaxOut];
  const int t = threadIdx.x, H = a.H;
  const int64_t b = blockIdx.x;
  if (t < a.C) {
    const int64_t yb = a.y[b];
    const bool yok = yb >= 0 && yb < a.C;
    const float g = yok ? (expf(a.logp[b * a.C + t]) - (t == yb ? 1.f : 0.f)) / float(a.B) : 0.f;
    dzs[t] = g;
    a.dz[b * a.C + t] = g;
  }
  __syncthreads();
  for (int k = t; k < H; k += 256) {
    const float p = tanhf(a.P[b * H + k] + a.pb[k]);
    float acc = 0.f;
    for (int c = 0; c < a.C; ++c) acc = fmaf(dzs[c], a.W[int64_t(c) * H + k], acc);
    a.pooled[b * H + k] = p;
    a.dP[b * H + k] = acc * (1.0f - p * p);
  }
}

// ---- d fc.weight [C, H], d fc.bias [C], skip_flag.  Block (x, c < C): columns 256 x .. of row c,
// the sequences in order; block (0, C): the bias and the flag.
struct FcGradTArgs {
  const float *dz, *pooled;   // [B, C], [B, H]
  int64_t B;
  int C, H;
  float *dW, *db;
  const int32_t* status;
  float* skip_flag;
};
__global__ __launch_bounds__(256) void k_bt_fc_grad(FcGradTArgs a) {
  const int t = threadIdx.x, c = blockIdx.y;
  if (c == a.C) {
    if (blockIdx.x != 0) return;
    if (t < a.C) {
      float s = 0.f;
      for (int64_t b = 0; b < a.B; ++b) s += a.dz[b * a.C + t];
      a.db[t] = s;
    }
    if (t == 0) *a.skip_flag = *a.status != 0 ? 1.0f : 0.0f;   // every status bit is known after the head
    return;
  }
  const int k = blockIdx.x * 256 + t;
  if (k >= a.H) return;
  float acc = 0.f;
  for (int64_t b = 0; b < a.B; ++b) acc = fmaf(a.dz[b * a.C + c], a.pooled[b * a.H + k], acc);
  a.dW[int64_t(c) * a.H + k] = acc;
}

// ---- LayerNorm backward, one wave per row with the row in registers.  dy = dyA + dyB (dyB may be
// null), times the mask of in_site when in_site >= 0 (the dropout between this LN's output and its
// readers).  With xh the saved normalised row and g = gamma:
//   du = inv (dy g - mean(dy g) - xh mean(dy g xh))
// dy and term = dy xh go out for the column sums (d beta, d gamma); du is the gradient of the LN's
// input (the residual's share), dbr = mask(out_site) du the dense branch's (null: not wanted).
struct LnBwdArgs {
  const float *dyA, *dyB, *xhat, *inv, *g;
  float *dy, *term, *du, *dbr;
  int64_t M;
  int H;
  Drop d;
  int in_site, out_site;
};
__global__ __launch_bounds__(256) void k_bt_ln_bwd(LnBwdArgs a) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, H = a.H, per = H >> 6;
  const int64_t r = int64_t(blockIdx.x) * 4 + w;
  if (r >= a.M) return;
  const int64_t o = r * H;
  const uint32_t bin = drop_base(a.d.seed, uint32_t(a.in_site), uint32_t(r));
  const uint32_t bout = drop_base(a.d.seed, uint32_t(a.out_site), uint32_t(r));
  float dy[kMaxPer], xh[kMaxPer];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int i = 0; i < kMaxPer; ++i)
    if (i < per) {
      const int c = l + kWave * i;
      float t = a.dyA[o + c];
      if (a.dyB) t += a.dyB[o + c];
      if (a.in_site >= 0) t = drop_h(t, bin, c, a.d);
      dy[i] = t;
      xh[i] = a.xhat[o + c];
      a.dy[o + c] = t;
      a.term[o + c] = t * xh[i];
      const float dg = t * a.g[c];
      s1 += dg;
      s2 = fmaf(dg, xh[i], s2);
    }
  s1 = wave_sum(s1) / float(H);
  s2 = wave_sum(s2) / float(H);
  const float inv = a.inv[r];
#pragma unroll
  for (int i = 0; i < kMaxPer; ++i)
    if (i < per) {
      const int c = l + kWave * i;
      const float du = inv * ((dy[i] * a.g[c] - s1) - xh[i] * s2);
      a.du[o + c] = du;
      if (a.dbr) a.dbr[o + c] = drop_h(du, bout, c, a.d);
    }
}

// ---- out_j[c] = sum over the rows of A_j[r][c] for up to four [rows, C] matrices (C % 64 == 0):
// block (x, j) takes 64 columns; wave q sums the rows q, q + 4, .. in order, the four wave sums are
// added in wave order
struct ColsumArgs {
  const float* A[4];
  float* out[4];
  int64_t rows;
  int C;
};
__global__ __launch_bounds__(256) void k_bt_colsum(ColsumArgs a) {
  __shared__ float red[4][kWave];
  const int q = threadIdx.x >> 6, l = threadIdx.x & 63, c = blockIdx.x * kWave + l;
  const float* A = a.A[blockIdx.y] + c;
  float acc = 0.f;
  int64_t r = q;
  for (; r + 12 < a.rows; r += 16) {   // four loads in flight
    const float v0 = A[r * a.C], v1 = A[(r + 4) * a.C], v2 = A[(r + 8) * a.C], v3 = A[(r + 12) * a.C];
    acc += v0; acc += v1; acc += v2; acc += v3;
  }
  for (; r < a.rows; r += 4) acc += A[r * a.C];
  red[q][l] = acc;
  __syncthreads();
  if (q == 0) a.out[blockIdx.y][c] = ((red[0][l] + red[1][l]) + red[2][l]) + red[3][l];
}

// ---- dm = dg gelu'(m) in place over dg; gelu'(x) = 0.5 (1 + erf(x / sqrt 2)) + x exp(-x^2 / 2) / sqrt(2 pi)
__device__ __forceinline__ float gelu_erf_grad(float x) {
  return fmaf(x * 0.39894228040143267794f, expf(-0.5f * x * x), 0.5f * (1.0f + erff(x * 0.70710678118654752440f)));
}
__global__ __launch_bounds__(256) void k_bt_gelu_bwd(float* __restrict__ dg, const float* __restrict__ m,
                                                     int64_t total4) {
  for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < total4; i += int64_t(gridDim.x) * 256) {
    const float4 d = ld4(dg + i * 4), x = ld4(m + i * 4);
    st4(dg + i * 4, make_float4(d.x * gelu_erf_grad(x.x), d.y * gelu_erf_grad(x.y), d.z * gelu_erf_grad(x.z),
                                d.w * gelu_erf_grad(x.w)));
  }
}

// ---- dv = keep(site, b, head) dctx / (1 - p_attn) in place over [M, H]
__global__ __launch_bounds__(256) void k_bt_head_mask(float* __restrict__ dctx, int64_t total4, int C4, Drop d,
                                                      uint32_t site) {
  for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < total4; i += int64_t(gridDim.x) * 256) {
    const int c = int(i % C4) * 4;
    const uint32_t b = uint32_t(i / C4);
    const float4 v = ld4(dctx + i * 4);
    const float s = drop_keep(drop_base(d.seed, site, b), uint32_t(c) >> 6, d.thr_a) ? d.scale_a : 0.f;
    st4(dctx + i * 4, s != 0.f ? make_float4(v.x * s, v.y * s, v.z * s, v.w * s) : f4zero());
  }
}

// ---- zeros into up to four buffers of n4[j] float4 each (16-byte aligned), job blockIdx.y
struct ZeroArgs {
  float* p[4];
  int64_t n4[4];
};
__global__ __launch_bounds__(256) void k_bt_zero(ZeroArgs a) {
  float* p = a.p[blockIdx.y];
  const int64_t n4 = a.n4[blockIdx.y];
  for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < n4; i += int64_t(gridDim.x) * 256) st4(p + i * 4, f4zero());
}

// ---- dx: zeros in the H columns of all N rows, then (the next launch) the sequences' first rows.
// An emptied sequence (len 0) writes nothing.
__global__ __launch_bounds__(256) void k_bt_dx_zero(float* __restrict__ dx, int64_t ldx, int64_t N, int H4) {
  const int64_t total = N * H4;
  for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < total; i += int64_t(gridDim.x) * 256)
    st4(dx + (i / H4) * ldx + (i % H4) * 4, f4zero());
}
__global__ __launch_bounds__(256) void k_bt_dx_roots(const float* __restrict__ de, SeqInfo sq, int H,
                                                     float* __restrict__ dx, int64_t ldx) {
  const int64_t b = blockIdx.x;
  if (sq.len[b] == 0) return;
  float* dst = dx + int64_t(sq.start[b]) * ldx;
  for (int c = threadIdx.x * 4; c < H; c += 1024) st4(dst + c, ld4(de + b * H + c));
}

// ---- host
struct BertTrainWs {
  float* hs[BGCN_BERT_MAX_LAYERS + 1];   // [B, H]: the embeddings' output, then every layer's
  float *ctx[BGCN_BERT_MAX_LAYERS], *a[BGCN_BERT_MAX_LAYERS];       // [B, H]
  float *m[BGCN_BERT_MAX_LAYERS], *g[BGCN_BERT_MAX_LAYERS];         // [B, I] before / after GELU
  float *xh1[BGCN_BERT_MAX_LAYERS], *xh2[BGCN_BERT_MAX_LAYERS];     // [B, H] normalised LN inputs
  float *inv1[BGCN_BERT_MAX_LAYERS], *inv2[BGCN_BERT_MAX_LAYERS];   // [B]
  float *xh0, *inv0;
  float *t, *P, *pooled, *dz, *dP;   // [B, H] x 3, [B, 64], [B, H]
  float *gA, *gB, *gX, *dy, *term, *dbr, *lin;   // [B, H] backward rows
  float* dI;                                      // [B, I]
  void* gemm;                                     // the products' own workspace (the policy's)
  size_t gemm_bytes;
  SeqInfo sq;
  float* loss_row;
  int32_t* predw;
  int64_t* first;
};

// ---- the chain's three products, as the two entry points run them (all operands contiguous):
//   xwt  Y[M, Nc] = X[M, K] . W[Nc, K]^T     xw  Y[M, K] = G[M, Nc] . W[Nc, K]     tn  dW[Nc, K] = G[M, Nc]^T . X[M, K]
// ws_bytes: what they need of the call's workspace for the weights [H, H], [I, H] and [H, I].
struct TiledGemms {   // bgcn_gemm.hip's block-tiled kernels: bgcn_bert_train_grad
  void* ws;
  size_t bytes;
  hipStream_t s;
  static size_t ws_bytes(int64_t B, int64_t H, int64_t I) {
    return std::max(std::max(tn_ws_size(H, I, B), tn_ws_size(I, H, B)), tn_ws_size(H, H, B));
  }
  int xwt(const float* X, const float* W, float* Y, int64_t M, int64_t Nc, int64_t K) const {
    return gemm_xwt_impl(X, K, W, nullptr, K, Nc, Y, Nc, M, Nc, K, s, nullptr);
  }
  int xw(const float* G, const float* W, float* Y, int64_t M, int64_t Nc, int64_t K) const {
    return gemm_xw2_impl(G, Nc, W, nullptr, K, Nc, Y, K, M, K, Nc, s);
  }
  int tn(const float* G, const float* X, float* dW, int64_t M, int64_t Nc, int64_t K) const {
    return gemm_tn_impl(G, Nc, X, K, dW, nullptr, K, Nc, Nc, K, M, ws, bytes, s, -1, nullptr);
  }
};
struct SkinnyGemms {   // bgcn_gemm_skinny.hip's split kernels: bgcn_bert_train_grad_skinny
  void* ws;
  size_t bytes;
  hipStream_t s;
  static size_t ws_bytes(int64_t B, int64_t H, int64_t I) {
    return sizeof(float) * std::max(std::max(skinny_part_floats(B, H, I), skinny_part_floats(B, I, H)),
                                    skinny_part_floats(B, H, H));
  }
  int xwt(const float* X, const float* W, float* Y, int64_t M, int64_t Nc, int64_t K) const {
    return gemm_xwt_skinny_impl(X, K, W, K, nullptr, Y, Nc, M, Nc, K, static_cast<float*>(ws), s);
  }
  int xw(const float* G, const float* W, float* Y, int64_t M, int64_t Nc, int64_t K) const {
    return gemm_xw_skinny_impl(G, Nc, W, K, Y, K, M, Nc, K, static_cast<float*>(ws), s);
  }
  int tn(const float* G, const float* X, float* dW, int64_t M, int64_t Nc, int64_t K) const {
    return gemm_tn_skinny_impl(G, Nc, X, K, dW, K, M, Nc, K, s);
  }
};

template <class Gemms>
size_t carve_bert_train(Carve& c, int64_t B, int64_t H, int64_t I, int64_t L, BertTrainWs* w) {
  const size_t nb = size_t(B), bh = nb * size_t(H), bi = nb * size_t(I);
  for (int l = 0; l <= L; ++l) w->hs[l] = c.take<float>(bh);
  for (int l = 0; l < L; ++l) {
    w->ctx[l] = c.take<float>(bh);
    w->a[l] = c.take<float>(bh);
    w->m[l] = c.take<float>(bi);
    w->g[l] = c.take<float>(bi);
    w->xh1[l] = c.take<float>(bh);
    w->xh2[l] = c.take<float>(bh);
    w->inv1[l] = c.take<float>(nb);
    w->inv2[l] = c.take<float>(nb);
  }
  w->xh0 = c.take<float>(bh);
  w->inv0 = c.take<float>(nb);
  float** rows[] = {&w->t, &w->P, &w->pooled, &w->dP, &w->gA, &w->gB, &w->gX, &w->dy, &w->term, &w->dbr, &w->lin};
  for (float** p : rows) *p = c.take<float>(bh);
  w->dz = c.take<float>(nb * kMaxOut);
  w->dI = c.take<float>(bi);
  w->gemm_bytes = Gemms::ws_bytes(B, H, I);
  w->gemm = c.take<char>(w->gemm_bytes);
  w->sq.start = c.take<int32_t>(nb);
  w->sq.len = c.take<int32_t>(nb);
  w->loss_row = c.take<float>(nb);
  w->predw = c.take<int32_t>(nb);
  w->first = c.take<int64_t>(1);
  return align_up(c.off, 256);
}

bool rate_ok(float p) { return p >= 0.f && p < 1.f; }   // false for a NaN
uint32_t drop_threshold(float p) { return uint32_t(std::floor(double(p) * 4294967296.0 + 0.5)); }

template <class Gemms>
int bert_train_grad_impl(const bgcn_bert_train_args* ta, void* ws, size_t ws_bytes, hipStream_t s) {
  BGCN_CHECK_ARG(ta, "null args");
  const bgcn_bert_args* a = &ta->fwd;
  BGCN_TRY(bert_check_args(a, ws));
  const int64_t N = a->num_nodes, B = a->num_seqs, H = a->hidden, I = a->intermediate, C = a->out_feats;
  const int L = int(a->num_layers);
  BGCN_CHECK_ARG(!a->hidden_out && !a->hidden_sum && !a->attn_sum,
                 "training is root-only: hidden_out, hidden_sum and attn_sum must be null");
  BGCN_CHECK_ARG(a->y && ta->skip_flag, "null pointer");
  BGCN_CHECK_ARG(rate_ok(ta->hidden_dropout) && rate_ok(ta->attn_dropout), "a dropout rate must lie in [0, 1)");
  BGCN_CHECK_ARG(a16(ta->dx), "x and dx rows must be 16-byte aligned (ldx % 4)");
  float* top[] = {ta->d_pos_emb, ta->d_type_emb, ta->d_emb_ln_w, ta->d_emb_ln_b,
                  ta->d_pooler_w, ta->d_pooler_b, ta->d_fc_w, ta->d_fc_b};
  for (float* p : top) BGCN_CHECK_ARG(p && a16(p), "null or unaligned BERT weight gradient");
  for (int l = 0; l < L; ++l) {
    const bgcn_bert_layer& y = ta->d_layer[l];
    const float* lw[] = {y.q_w, y.q_b, y.k_w, y.k_b, y.v_w, y.v_b, y.ao_w, y.ao_b, y.ao_ln_w, y.ao_ln_b,
                         y.i_w, y.i_b, y.o_w, y.o_b, y.o_ln_w, y.o_ln_b};
    for (const float* p : lw) BGCN_CHECK_ARG(p && a16(p), "null or unaligned BERT weight gradient");
  }
  BertTrainWs w;
  Carve c(ws, ws_bytes);
  carve_bert_train<Gemms>(c, B, H, I, L, &w);
  BGCN_CHECK_ARG(ws && align_up(c.off, 256) <= ws_bytes, "workspace too small");   // the entry's own size function's figure
  const Gemms mm{w.gemm, w.gemm_bytes, s};

  Drop d{ta->drop_seed, drop_threshold(ta->hidden_dropout), drop_threshold(ta->attn_dropout),
         1.0f / (1.0f - ta->hidden_dropout), 1.0f / (1.0f - ta->attn_dropout)};
  const unsigned rows4 = grid_for(B, 4);
  const int iH = int(H), iI = int(I);
  const auto ew_grid = [](int64_t total4) { return dim3(unsigned(std::min<int64_t>((total4 + 255) / 256, 4096))); };
  const auto grad = [](const float* p) { return const_cast<float*>(p); };

  // ---- forward
  bert_setup(a, w.sq, w.first, s);
  EmbedTArgs em{a->x, a->ldx, a->pos_emb, a->type_emb, a->emb_ln_w, a->emb_ln_b, w.sq, w.hs[0], w.xh0, w.inv0,
                B, iH, a->ln_eps, d};
  hipLaunchKernelGGL(k_bt_embed, dim3(rows4), dim3(256), 0, s, em);
  BGCN_CHECK_LAUNCH();
  for (int l = 0; l < L; ++l) {
    const bgcn_bert_layer& y = a->layer[l];
    const uint32_t site = 3u * uint32_t(l);
    BGCN_TRY(mm.xwt(w.hs[l], y.v_w, w.ctx[l], B, H, H));
    hipLaunchKernelGGL(k_bt_ctx, ew_grid(B * H / 4), dim3(256), 0, s, w.ctx[l], y.v_b, B * H / 4, int(H / 4), d,
                       site + 1);
    BGCN_CHECK_LAUNCH();
    BGCN_TRY(mm.xwt(w.ctx[l], y.ao_w, w.t, B, H, H));
    AddLnTArgs l1{w.t, y.ao_b, w.hs[l], y.ao_ln_w, y.ao_ln_b, w.a[l], w.xh1[l], w.inv1[l], B, iH, a->ln_eps, d, site + 2};
    hipLaunchKernelGGL(k_bt_add_ln, dim3(rows4), dim3(256), 0, s, l1);
    BGCN_TRY(mm.xwt(w.a[l], y.i_w, w.m[l], B, I, H));
    hipLaunchKernelGGL(k_bt_inter, ew_grid(B * I / 4), dim3(256), 0, s, w.m[l], y.i_b, w.g[l], B * I / 4, int(I / 4));
    BGCN_TRY(mm.xwt(w.g[l], y.o_w, w.t, B, H, I));
    AddLnTArgs l2{w.t, y.o_b, w.a[l], y.o_ln_w, y.o_ln_b, w.hs[l + 1], w.xh2[l], w.inv2[l], B, iH, a->ln_eps, d, site + 3};
    hipLaunchKernelGGL(k_bt_add_ln, dim3(rows4), dim3(256), 0, s, l2);
    BGCN_CHECK_LAUNCH();
  }
  BGCN_TRY(mm.xwt(w.hs[L], a->pooler_w, w.P, B, H, H));
  BGCN_TRY(bert_head(a, w.P, w.loss_row, w.predw, s));

  // ---- backward: the head and the pooler
  const auto tn = [&](const float* G, int64_t Nc, const float* X, int64_t K, float* dW) {
    return mm.tn(G, X, dW, B, Nc, K);
  };
  const auto colsum = [&](int jobs, int Cc, const float* A0, float* o0, const float* A1 = nullptr, float* o1 = nullptr,
                          const float* A2 = nullptr, float* o2 = nullptr, const float* A3 = nullptr, float* o3 = nullptr) {
    ColsumArgs cs{{A0, A1, A2, A3}, {o0, o1, o2, o3}, B, Cc};
    hipLaunchKernelGGL(k_bt_colsum, dim3(unsigned(Cc / kWave), unsigned(jobs)), dim3(256), 0, s, cs);
  };
  HeadBwdTArgs hb{w.P, a->pooler_b, a->fc_w, a->logp, a->y, B, iH, int(C), w.dz, w.pooled, w.dP};
  hipLaunchKernelGGL(k_bt_head_bwd, dim3(unsigned(B)), dim3(256), 0, s, hb);
  FcGradTArgs fg{w.dz, w.pooled, B, int(C), iH, ta->d_fc_w, ta->d_fc_b, a->status, ta->skip_flag};
  hipLaunchKernelGGL(k_bt_fc_grad, dim3(grid_for(H, 256), unsigned(C + 1)), dim3(256), 0, s, fg);
  colsum(1, iH, w.dP, ta->d_pooler_b);
  BGCN_CHECK_LAUNCH();
  BGCN_TRY(tn(w.dP, H, w.hs[L], H, ta->d_pooler_w));
  BGCN_TRY(mm.xw(w.dP, a->pooler_w, w.gA, B, H, H));

  // ---- backward through the layers: the layer output's gradient is gA (+ gB below the last layer)
  const float* gB = nullptr;
  for (int l = L - 1; l >= 0; --l) {
    const bgcn_bert_layer &y = a->layer[l], &dl = ta->d_layer[l];
    const int site = 3 * l;
    LnBwdArgs b2{w.gA, gB, w.xh2[l], w.inv2[l], y.o_ln_w, w.dy, w.term, w.gX, w.dbr, B, iH, d, -1, site + 3};
    hipLaunchKernelGGL(k_bt_ln_bwd, dim3(rows4), dim3(256), 0, s, b2);
    colsum(3, iH, w.term, grad(dl.o_ln_w), w.dy, grad(dl.o_ln_b), w.dbr, grad(dl.o_b));
    BGCN_CHECK_LAUNCH();
    BGCN_TRY(tn(w.dbr, H, w.g[l], I, grad(dl.o_w)));
    BGCN_TRY(mm.xw(w.dbr, y.o_w, w.dI, B, H, I));
    hipLaunchKernelGGL(k_bt_gelu_bwd, ew_grid(B * I / 4), dim3(256), 0, s, w.dI, w.m[l], B * I / 4);
    colsum(1, iI, w.dI, grad(dl.i_b));
    BGCN_CHECK_LAUNCH();
    BGCN_TRY(tn(w.dI, I, w.a[l], H, grad(dl.i_w)));
    BGCN_TRY(mm.xw(w.dI, y.i_w, w.lin, B, I, H));
    LnBwdArgs b1{w.gX, w.lin, w.xh1[l], w.inv1[l], y.ao_ln_w, w.dy, w.term, w.gA, w.dbr, B, iH, d, -1, site + 2};
    hipLaunchKernelGGL(k_bt_ln_bwd, dim3(rows4), dim3(256), 0, s, b1);
    colsum(3, iH, w.term, grad(dl.ao_ln_w), w.dy, grad(dl.ao_ln_b), w.dbr, grad(dl.ao_b));
    BGCN_CHECK_LAUNCH();
    BGCN_TRY(tn(w.dbr, H, w.ctx[l], H, grad(dl.ao_w)));
    BGCN_TRY(mm.xw(w.dbr, y.ao_w, w.lin, B, H, H));
    hipLaunchKernelGGL(k_bt_head_mask, ew_grid(B * H / 4), dim3(256), 0, s, w.lin, B * H / 4, int(H / 4), d,
                       uint32_t(site + 1));
    colsum(1, iH, w.lin, grad(dl.v_b));
    ZeroArgs zq{{grad(dl.q_w), grad(dl.k_w), grad(dl.q_b), grad(dl.k_b)}, {H * H / 4, H * H / 4, H / 4, H / 4}};
    hipLaunchKernelGGL(k_bt_zero, dim3(unsigned(std::min<int64_t>((H * H / 4 + 255) / 256, 1024)), 4), dim3(256), 0, s,
                       zq);
    BGCN_CHECK_LAUNCH();
    BGCN_TRY(tn(w.lin, H, w.hs[l], H, grad(dl.v_w)));
    BGCN_TRY(mm.xw(w.lin, y.v_w, w.gB, B, H, H));
    gB = w.gB;
  }

  // ---- the embeddings: the mask of site 0, LN backward, row 0 of d position / d type
  LnBwdArgs be{w.gA, gB, w.xh0, w.inv0, a->emb_ln_w, w.dy, w.term, w.gX, nullptr, B, iH, d, 0, -1};
  hipLaunchKernelGGL(k_bt_ln_bwd, dim3(rows4), dim3(256), 0, s, be);
  colsum(4, iH, w.term, ta->d_emb_ln_w, w.dy, ta->d_emb_ln_b, w.gX, ta->d_pos_emb, w.gX, ta->d_type_emb);
  ZeroArgs ze{{ta->d_pos_emb + H, ta->d_type_emb + H, nullptr, nullptr}, {(a->max_pos - 1) * H / 4, H / 4, 0, 0}};
  hipLaunchKernelGGL(k_bt_zero, dim3(unsigned(std::min<int64_t>((a->max_pos * H / 4 + 255) / 256, 1024)), 2), dim3(256),
                     0, s, ze);
  if (ta->dx) {
    hipLaunchKernelGGL(k_bt_dx_zero, ew_grid(N * H / 4), dim3(256), 0, s, ta->dx, a->ldx, N, int(H / 4));
    hipLaunchKernelGGL(k_bt_dx_roots, dim3(unsigned(B)), dim3(256), 0, s, w.gX, w.sq, iH, ta->dx, a->ldx);
  }
  BGCN_CHECK_LAUNCH();
  return BGCN_OK;
}

}  // namespace
}  // namespace bgcn

extern "C" size_t bgcn_bert_train_workspace_size(int64_t num_nodes, int64_t num_seqs, int64_t hidden,
                                                 int64_t intermediate, int64_t num_layers) {
  if (!bgcn::bert_shape_ok(num_nodes, num_seqs, hidden, intermediate, num_layers)) return 0;
  bgcn::BertTrainWs w;
  bgcn::Carve c(nullptr, 0);
  return bgcn::carve_bert_train<bgcn::TiledGemms>(c, num_seqs, hidden, intermediate, num_layers, &w);
}

extern "C" int bgcn_bert_train_grad(const bgcn_bert_train_args* args, void* workspace, size_t workspace_bytes,
                                    bgcn_stream_t stream) {
  return bgcn::bert_train_grad_impl<bgcn::TiledGemms>(args, workspace, workspace_bytes,
                                                      reinterpret_cast<hipStream_t>(stream));
}

extern "C" size_t bgcn_bert_train_skinny_workspace_size(int64_t num_nodes, int64_t num_seqs, int64_t hidden,
                                                        int64_t intermediate, int64_t num_layers) {
  if (!bgcn::bert_shape_ok(num_nodes, num_seqs, hidden, intermediate, num_layers)) return 0;
  bgcn::BertTrainWs w;
  bgcn::Carve c(nullptr, 0);
  return bgcn::carve_bert_train<bgcn::SkinnyGemms>(c, num_seqs, hidden, intermediate, num_layers, &w);
}

extern "C" int bgcn_bert_train_grad_skinny(const bgcn_bert_train_args* args, void* workspace, size_t workspace_bytes,
                                           bgcn_stream_t stream) {
  return bgcn::bert_train_grad_impl<bgcn::SkinnyGemms>(args, workspace, workspace_bytes,
                                                       reinterpret_cast<hipStream_t>(stream));
}
