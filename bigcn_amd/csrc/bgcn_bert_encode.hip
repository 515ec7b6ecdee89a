// bgcn_bert_encode: the PHEME feature extraction (Process/getPHEMEgraph.py:104-118) - a plain
// BertModel in eval mode over token ids, no attention mask: model.embeddings(ids) and
// model(ids).pooler_output - for num_seqs sequences of seq_len tokens as one launch sequence on the
// caller's stream, everything in the caller's workspace.  Row b T + t of every [M, .] matrix
// (M = num_seqs T) is token t of sequence b.
//
//   k_bert_embed_ids   h = LN(word[id] + type[0] + pos[t]), one wave per (sequence, position); a token
//                      id outside [0, vocab) sets BGCN_STATUS_TOKEN and is clamped before any read
//   per layer          the GEMMs of bgcn_bert_eval through gemm_xwt_impl (q | k as one product, v,
//                      attention-output dense, intermediate, output) and its two row kernels
//                      (bert_bias_act, bert_add_ln: bgcn_bert.hip)
//     k_bert_attn_all  attention over all T keys: a workgroup is four query tiles of one (sequence,
//                      head) and stages every K / V tile in LDS once for its four waves
//   last layer         CLS-only by default: k | v as one product over all rows, then q, attention
//     k_bert_attn_cls  (one wave per (sequence, head), query 0 only), attention-output, intermediate,
//                      output and both LayerNorms on the [num_seqs, hidden] first rows, read with the
//                      row stride T hidden.  last_layer_full: as every other layer.
//   k_bert_pooler      cls = tanh(pooler GEMM + bias)
//
// Stream order is the only dependency between the launches.  No float atomics; every sum has a
// fixed order.
#include "bgcn_bert.h"

namespace bgcn {
namespace {

constexpr int kHeadDim = 64;
constexpr int kQTile = BGCN_BERT_QUERY_TILE;
constexpr int kMaxPos = 512;
constexpr int kAttnWaves = 4;              // query tiles per workgroup of k_bert_attn_all
constexpr int kKvLd = kHeadDim + 4;        // row stride of the staged tiles: 16-byte rows, 4 banks apart
static_assert(kQTile == 32, "one 32x32 MFMA tile of scores per key tile");

// ---- embeddings.  Wave (b, pos): row b T + pos of dst (and of emb, when given).
struct EmbedIdsArgs {
  const int64_t* ids;   // [B, T]
  const float *word, *pos_emb, *type_emb, *g, *be;
  float* dst;           // [M, ld_dst]
  float* emb;           // [M, ld_emb] or null
  int64_t ld_dst, ld_emb, vocab;
  int T, H;
  float eps;
  int32_t* status;
};
__global__ __launch_bounds__(256) void k_bert_embed_ids(EmbedIdsArgs a) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int64_t b = blockIdx.x;
  const int pos = blockIdx.y * 4 + w, H = a.H, per = H >> 6;
  if (pos >= a.T) return;
  const int64_t row = b * a.T + pos;
  int64_t id = a.ids[row];
  if (id < 0 || id >= a.vocab) {
    if (l == 0) atomicOr(a.status, BGCN_STATUS_TOKEN);
    id = id < 0 ? 0 : a.vocab - 1;
  }
  const float* wr = a.word + id * H;
  const float* pe = a.pos_emb + int64_t(pos) * H;
  float v[kMaxPer];
#pragma unroll
  for (int i = 0; i < kMaxPer; ++i)
    if (i < per) {
      const int c = l + kWave * i;
      v[i] = (wr[c] + a.type_emb[c]) + pe[c];
    }
  const float inv = ln_row(v, per, H, a.g, a.be, a.eps, l, a.dst + row * a.ld_dst, nullptr);
  if (a.emb) {   // ln_row's own expression: the same bits
    float* out = a.emb + row * a.ld_emb;
#pragma unroll
    for (int i = 0; i < kMaxPer; ++i)
      if (i < per) {
        const int c = l + kWave * i;
        out[c] = fmaf(v[i] * inv, a.g[c], a.be[c]);
      }
  }
}

// ---- attention of one head over all T keys.  Workgroup (qb, head, b): wave w holds the queries
// [32 (4 qb + w), + 32) of sequence b.  Both products run on v_mfma_f32_32x32x2_f32 with k_bert_attn's
// lane maps (bgcn_bert.hip):
//   scores  S^T[key][query]: lane (j = l & 31, h = l >> 5) holds 8 consecutive k of row j of K (A)
//           and of Q (B) per 16-k block (16 i + 8 h ..); register 4 g + u of lane (j, h) is key
//           8 g + 4 h + u of the tile against query j.  A key past T scores -inf: its p is exactly 0.
//   one pass over the key tiles with a running maximum m and sum lsum per query (both in the two
//           lanes j, j + 32): mn = max(m, the tile's maximum), alpha = exp(m - mn), p = exp(s - mn),
//           lsum = lsum alpha + sum p, acc = acc alpha + V^T p.  Every tile holds key 32 kt < T, so mn
//           is finite; before the first tile m = -inf and alpha = 0 on acc = 0.
//   ctx^T[d][query] += V^T[d][key] P^T[key][query] takes register 4 g + u as the B operand of MFMA
//           (g, u) with no lane movement (lane (d, h) reads V[key 8 g + 4 h + u][d]).
// STAGE: the 256 threads copy the tile's K (+ bias) and V rows into LDS, the next tile's loads in
// flight while this one is computed; rows past T are read as row T - 1 (in bounds, finite; p = 0).
// !STAGE: every wave reads its operands from global memory, as k_bert_attn does.  Same bits.
struct AttnAllArgs {
  const float* qkv;   // [M, 3H]: q | k | v, without their biases
  const float *bq, *bk, *bv;
  float* ctx;         // [M, H]
  int T, H;
};
__device__ __forceinline__ void ld8(const float* p, float* dst) {
  const float4 x0 = ld4(p), x1 = ld4(p + 4);
  dst[0] = x0.x; dst[1] = x0.y; dst[2] = x0.z; dst[3] = x0.w;
  dst[4] = x1.x; dst[5] = x1.y; dst[6] = x1.z; dst[7] = x1.w;
}
__device__ __forceinline__ void ld8_bias(const float* p, const float* b, float* dst) {
  const float4 x0 = f4add(ld4(p), ld4(b)), x1 = f4add(ld4(p + 4), ld4(b + 4));
  dst[0] = x0.x; dst[1] = x0.y; dst[2] = x0.z; dst[3] = x0.w;
  dst[4] = x1.x; dst[5] = x1.y; dst[6] = x1.z; dst[7] = x1.w;
}
template <bool STAGE>
__global__ __launch_bounds__(64 * kAttnWaves) void k_bert_attn_all(AttnAllArgs a) {
  __shared__ __attribute__((aligned(16))) float Ks[STAGE ? kQTile * kKvLd : 4];
  __shared__ __attribute__((aligned(16))) float Vs[STAGE ? kQTile * kKvLd : 4];
  const int t = threadIdx.x, w = t >> 6, l = t & 63, j = l & 31, h = l >> 5;
  const int head = blockIdx.y, T = a.T;
  const int64_t row0 = int64_t(blockIdx.z) * T, ld = 3 * int64_t(a.H);
  const int q0 = (blockIdx.x * kAttnWaves + w) * kQTile;
  const bool wave_on = q0 < T;   // an idle wave of the last workgroup still stages and meets the barriers
  const bool qvalid = q0 + j < T;
  const int nkt = (T + kQTile - 1) / kQTile;
  const float* kbase = a.qkv + a.H + head * kHeadDim;
  const float* vbase = a.qkv + 2 * a.H + head * kHeadDim;
  float q[32];
  {
    const float* qp = a.qkv + (row0 + min(q0 + j, T - 1)) * ld + head * kHeadDim + 8 * h;
    const float* bp = a.bq + head * kHeadDim + 8 * h;
#pragma unroll
    for (int i = 0; i < 4; ++i) ld8_bias(qp + 16 * i, bp + 16 * i, &q[8 * i]);
  }
  // staging: thread t copies the float4 (row sr + 16 u, column sc) of both tiles, u < 2
  const int sr = t >> 4, sc = (t & 15) * 4;
  float4 kreg[2], vreg[2];
  const auto fetch = [&](int kt) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int64_t r = row0 + min(kt * kQTile + sr + 16 * u, T - 1);
      kreg[u] = f4add(ld4(kbase + r * ld + sc), ld4(a.bk + head * kHeadDim + sc));
      vreg[u] = ld4(vbase + r * ld + sc);
    }
  };
  if constexpr (STAGE) fetch(0);

  float m = -INFINITY, lsum = 0.f;
  f32x16 acc[2];
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[0][r] = acc[1][r] = 0.f;
  for (int kt = 0; kt < nkt; ++kt) {
    if constexpr (STAGE) {
      __syncthreads();   // the previous tile has been read by every wave
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        st4(&Ks[(sr + 16 * u) * kKvLd + sc], kreg[u]);
        st4(&Vs[(sr + 16 * u) * kKvLd + sc], vreg[u]);
      }
      __syncthreads();
      if (kt + 1 < nkt) fetch(kt + 1);
    }
    if (!wave_on) continue;
    float k[32];
    if constexpr (STAGE) {
#pragma unroll
      for (int i = 0; i < 4; ++i) ld8(&Ks[j * kKvLd + 16 * i + 8 * h], &k[8 * i]);
    } else {
      const float* kp = kbase + (row0 + min(kt * kQTile + j, T - 1)) * ld + 8 * h;
      const float* bp = a.bk + head * kHeadDim + 8 * h;
#pragma unroll
      for (int i = 0; i < 4; ++i) ld8_bias(kp + 16 * i, bp + 16 * i, &k[8 * i]);
    }
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i) s = mfma32x32x2(k[i], q[i], s);
    float tm = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = kt * kQTile + 8 * (r >> 2) + 4 * h + (r & 3);
      s[r] = key < T ? s[r] * 0.125f : -INFINITY;
      tm = fmaxf(tm, s[r]);
    }
    tm = fmaxf(tm, __shfl_xor(tm, 32));
    const float mn = fmaxf(m, tm), alpha = expf(m - mn);
    float e = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s[r] = expf(s[r] - mn);
      e += s[r];
    }
    lsum = lsum * alpha + e;
    m = mn;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      acc[0][r] *= alpha;
      acc[1][r] *= alpha;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int krow = 8 * (r >> 2) + 4 * h + (r & 3);
      float v0, v1;
      if constexpr (STAGE) {
        v0 = Vs[krow * kKvLd + j];
        v1 = Vs[krow * kKvLd + 32 + j];
      } else {
        const float* vp = vbase + (row0 + min(kt * kQTile + krow, T - 1)) * ld + j;
        v0 = vp[0];
        v1 = vp[32];
      }
      acc[0] = mfma32x32x2(v0, s[r], acc[0]);
      acc[1] = mfma32x32x2(v1, s[r], acc[1]);
    }
  }
  if (!qvalid) return;
  lsum += __shfl_xor(lsum, 32);   // lanes j and j + 32 are both active: qvalid depends on j alone
  float* out = a.ctx + (row0 + q0 + j) * a.H + head * kHeadDim;
  const float* bv = a.bv + head * kHeadDim;
#pragma unroll
  for (int dh = 0; dh < 2; ++dh)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int d = 32 * dh + 8 * g + 4 * h;
      st4(out + d, f4add(make_float4(acc[dh][4 * g] / lsum, acc[dh][4 * g + 1] / lsum, acc[dh][4 * g + 2] / lsum,
                                     acc[dh][4 * g + 3] / lsum),
                         ld4(bv + d)));
    }
}

// ---- the last layer's attention of query 0.  Wave (b, head), lane l: the scores of the keys
// l + 64 u (u < 8: T <= 512) as 64-term fmaf chains, the softmax by wave reductions, then as column l
// of the head ctx[l] = sum over the keys in ascending order of p[key] v[key][l].  Writes row b of
// ctx [B, H].
struct AttnClsArgs {
  const float* qkv;   // [M, 3H]; q only in the rows b T
  const float *bq, *bk, *bv;
  float* ctx;         // [B, H]
  int T, H, heads;
};
__global__ __launch_bounds__(256) void k_bert_attn_cls(AttnClsArgs a) {
  constexpr int kPer = kMaxPos / kWave;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int head = blockIdx.y * 4 + w, T = a.T;
  if (head >= a.heads) return;
  const int64_t b = blockIdx.x, row0 = b * T, ld = 3 * int64_t(a.H);
  float q[kHeadDim];
  {
    const float* qp = a.qkv + row0 * ld + head * kHeadDim;
    const float* bp = a.bq + head * kHeadDim;
#pragma unroll
    for (int i = 0; i < kHeadDim / 8; ++i) ld8_bias(qp + 8 * i, bp + 8 * i, &q[8 * i]);
  }
  const float* kbase = a.qkv + a.H + head * kHeadDim;
  const float* bk = a.bk + head * kHeadDim;
  float s[kPer], mx = -INFINITY;
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const int key = l + kWave * u;
    s[u] = -INFINITY;
    if (key < T) {
      const float* kp = kbase + (row0 + key) * ld;
      float d = 0.f;
#pragma unroll
      for (int i = 0; i < kHeadDim / 8; ++i) {
        float k[8];
        ld8_bias(kp + 8 * i, bk + 8 * i, k);
#pragma unroll
        for (int c = 0; c < 8; ++c) d = fmaf(k[c], q[8 * i + c], d);
      }
      s[u] = d * 0.125f;
    }
    mx = fmaxf(mx, s[u]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));   // key 0 < T: finite
  float e = 0.f;
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    s[u] = expf(s[u] - mx);   // a key past T: exactly 0
    e += s[u];
  }
  const float lsum = wave_sum(e);
  const float* vbase = a.qkv + 2 * a.H + head * kHeadDim + l;
  float acc = 0.f;
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    if (kWave * u >= T) break;   // wave-uniform
    const int n = min(kWave, T - kWave * u);
    for (int kk = 0; kk < n; ++kk)
      acc = fmaf(__shfl(s[u], kk), vbase[(row0 + kWave * u + kk) * ld], acc);
  }
  a.ctx[b * a.H + head * kHeadDim + l] = acc / lsum + a.bv[head * kHeadDim + l];
}

// ---- cls[b][c] = tanh(P[b][c] + bias[c]) (P: the pooler's GEMM)
__global__ __launch_bounds__(256) void k_bert_pooler(const float* __restrict__ P, const float* __restrict__ bias,
                                                     float* __restrict__ cls, int64_t total, int H) {
  for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < total; i += int64_t(gridDim.x) * 256)
    cls[i] = tanhf(P[i] + bias[i % H]);
}

// ---- host
struct EncWs {
  float *h, *a, *t, *ctx, *qkv, *inter, *P;
};

void carve_encode(Carve& c, int64_t M, int64_t B, int64_t H, int64_t I, EncWs* w) {
  const size_t m = size_t(M), h = size_t(H);
  w->h = c.take<float>(m * h);
  w->a = c.take<float>(m * h);
  w->t = c.take<float>(m * h);
  w->ctx = c.take<float>(m * h);
  w->qkv = c.take<float>(m * 3 * h);
  w->inter = c.take<float>(m * size_t(I));
  w->P = c.take<float>(size_t(B) * h);
}

bool encode_shape_ok(int64_t B, int64_t T, int64_t H, int64_t I, int64_t L) {
  return B > 0 && T > 0 && T <= kMaxPos && bert_shape_ok(B * T, B, H, I, L);
}

int encode_impl(const bgcn_bert_encode_args* a, void* ws, size_t ws_bytes, hipStream_t s) {
  BGCN_CHECK_ARG(a, "null args");
  const int64_t B = a->num_seqs, T = a->seq_len, H = a->hidden, I = a->intermediate, L = a->num_layers;
  BGCN_CHECK_ARG(encode_shape_ok(B, T, H, I, L) && a->heads * kHeadDim == H && a->max_pos >= 1 && a->max_pos <= kMaxPos,
                 "unsupported shape (hidden = 64 heads in [64, 1024], intermediate % 64 in [64, 4096], layers in "
                 "[1, 24], max_pos in [1, 512], num_seqs in [1, 65535])");
  BGCN_CHECK_ARG(T <= a->max_pos, "seq_len must be in [1, max_pos]");
  BGCN_CHECK_ARG(a->vocab >= 1, "vocab must be at least 1");
  BGCN_CHECK_ARG(a->input_ids && a->status, "null pointer");
  const float* emb[] = {a->word_emb, a->pos_emb, a->type_emb, a->emb_ln_w, a->emb_ln_b};
  for (const float* p : emb) BGCN_CHECK_ARG(p && a16(p), "null or unaligned BERT weight");
  const bool embed_only = a->embed_only != 0, full_last = a->last_layer_full != 0;
  if (!embed_only) {
    BGCN_CHECK_ARG(a->pooler_w && a16(a->pooler_w) && a->pooler_b && a16(a->pooler_b), "null or unaligned BERT weight");
    for (int l = 0; l < L; ++l) {
      const bgcn_bert_layer& y = a->layer[l];
      const float* lw[] = {y.q_w, y.q_b, y.k_w, y.k_b, y.v_w, y.v_b, y.ao_w, y.ao_b, y.ao_ln_w, y.ao_ln_b,
                           y.i_w, y.i_b, y.o_w, y.o_b, y.o_ln_w, y.o_ln_b};
      for (const float* p : lw) BGCN_CHECK_ARG(p && a16(p), "null or unaligned BERT weight");
    }
  }
  BGCN_CHECK_ARG(embed_only ? a->embeddings != nullptr : a->cls != nullptr,
                 "null output (cls is required; embeddings with embed_only)");
  BGCN_CHECK_ARG(a16(a->embeddings) && a16(a->cls) && a16(a->hidden_out) && a16(ws) &&
                     (!a->embeddings || (a->ld_embeddings >= H && a->ld_embeddings % 4 == 0)),
                 "embeddings (ld_embeddings % 4, at least hidden), cls, hidden_out and the workspace must be 16-byte "
                 "aligned");
  BGCN_CHECK_ARG(!a->hidden_out || (full_last && !embed_only), "hidden_out needs last_layer_full");
  const int64_t M = B * T;
  const int heads = int(a->heads);
  EncWs w{};
  if (!embed_only) {
    Carve c(ws, ws_bytes);
    carve_encode(c, M, B, H, I, &w);
    BGCN_CHECK_ARG(ws && align_up(c.off, 256) <= ws_bytes, "workspace too small");   // bgcn_bert_encode_workspace_size's figure
  }

  BGCN_CHECK_HIP(hipMemsetAsync(a->status, 0, sizeof(int32_t), s));
  // embed_only: the rows go to embeddings alone
  EmbedIdsArgs em{a->input_ids, a->word_emb, a->pos_emb, a->type_emb, a->emb_ln_w, a->emb_ln_b,
                  embed_only ? a->embeddings : w.h, embed_only ? nullptr : a->embeddings,
                  embed_only ? a->ld_embeddings : H, a->ld_embeddings, a->vocab, int(T), int(H), a->ln_eps, a->status};
  hipLaunchKernelGGL(k_bert_embed_ids, dim3(unsigned(B), grid_for(T, 4)), dim3(256), 0, s, em);
  BGCN_CHECK_LAUNCH();
  if (embed_only) return BGCN_OK;

  const bool stage = knob("BGCN_BERT_ATTN_STAGE", 1) != 0;
  const float* roots = nullptr;   // the last layer's first rows
  int64_t ld_roots = 0;
  for (int l = 0; l < L; ++l) {
    const bgcn_bert_layer& y = a->layer[l];
    if (l < L - 1 || full_last) {
      BGCN_TRY(gemm_xwt_impl(w.h, H, y.q_w, y.k_w, H, H, w.qkv, 3 * H, M, 2 * H, H, s, nullptr));
      BGCN_TRY(gemm_xwt_impl(w.h, H, y.v_w, nullptr, H, H, w.qkv + 2 * H, 3 * H, M, H, H, s, nullptr));
      AttnAllArgs at{w.qkv, y.q_b, y.k_b, y.v_b, w.ctx, int(T), int(H)};
      const dim3 grid(grid_for(T, kAttnWaves * kQTile), unsigned(heads), unsigned(B));
      if (stage)
        hipLaunchKernelGGL(k_bert_attn_all<true>, grid, dim3(64 * kAttnWaves), 0, s, at);
      else
        hipLaunchKernelGGL(k_bert_attn_all<false>, grid, dim3(64 * kAttnWaves), 0, s, at);
      BGCN_CHECK_LAUNCH();
      BGCN_TRY(gemm_xwt_impl(w.ctx, H, y.ao_w, nullptr, H, H, w.t, H, M, H, H, s, nullptr));
      bert_add_ln(w.t, y.ao_b, w.h, H, y.ao_ln_w, y.ao_ln_b, w.a, nullptr, nullptr, M, int(H), a->ln_eps, s);
      BGCN_TRY(gemm_xwt_impl(w.a, H, y.i_w, nullptr, H, I, w.inter, I, M, I, H, s, nullptr));
      bert_bias_act(w.inter, y.i_b, M, I, true, s);
      BGCN_TRY(gemm_xwt_impl(w.inter, I, y.o_w, nullptr, I, H, w.t, H, M, H, I, s, nullptr));
      float* out = l == L - 1 && a->hidden_out ? a->hidden_out : w.h;
      bert_add_ln(w.t, y.o_b, w.a, H, y.o_ln_w, y.o_ln_b, out, nullptr, nullptr, M, int(H), a->ln_eps, s);
      BGCN_CHECK_LAUNCH();
      roots = out;
      ld_roots = T * H;
    } else {
      // CLS-only: k | v of every row, q of the first rows (rows T apart in h and in qkv); from the
      // attention on, [B, H] matrices in the first B rows of ctx, t, a and inter
      BGCN_TRY(gemm_xwt_impl(w.h, H, y.k_w, y.v_w, H, H, w.qkv + H, 3 * H, M, 2 * H, H, s, nullptr));
      BGCN_TRY(gemm_xwt_impl(w.h, T * H, y.q_w, nullptr, H, H, w.qkv, T * 3 * H, B, H, H, s, nullptr));
      AttnClsArgs at{w.qkv, y.q_b, y.k_b, y.v_b, w.ctx, int(T), int(H), heads};
      hipLaunchKernelGGL(k_bert_attn_cls, dim3(unsigned(B), grid_for(heads, 4)), dim3(256), 0, s, at);
      BGCN_CHECK_LAUNCH();
      BGCN_TRY(gemm_xwt_impl(w.ctx, H, y.ao_w, nullptr, H, H, w.t, H, B, H, H, s, nullptr));
      bert_add_ln(w.t, y.ao_b, w.h, T * H, y.ao_ln_w, y.ao_ln_b, w.a, nullptr, nullptr, B, int(H), a->ln_eps, s);
      BGCN_TRY(gemm_xwt_impl(w.a, H, y.i_w, nullptr, H, I, w.inter, I, B, I, H, s, nullptr));
      bert_bias_act(w.inter, y.i_b, B, I, true, s);
      BGCN_TRY(gemm_xwt_impl(w.inter, I, y.o_w, nullptr, I, H, w.t, H, B, H, I, s, nullptr));
      bert_add_ln(w.t, y.o_b, w.a, H, y.o_ln_w, y.o_ln_b, w.ctx, nullptr, nullptr, B, int(H), a->ln_eps, s);
      BGCN_CHECK_LAUNCH();
      roots = w.ctx;
      ld_roots = H;
    }
  }
  BGCN_TRY(gemm_xwt_impl(roots, ld_roots, a->pooler_w, nullptr, H, H, w.P, H, B, H, H, s, nullptr));
  hipLaunchKernelGGL(k_bert_pooler, dim3(unsigned(std::min<int64_t>((B * H + 255) / 256, 4096))), dim3(256), 0, s, w.P,
                     a->pooler_b, a->cls, B * H, int(H));
  BGCN_CHECK_LAUNCH();
  return BGCN_OK;
}

}  // namespace
}  // namespace bgcn

extern "C" size_t bgcn_bert_encode_workspace_size(int64_t num_seqs, int64_t seq_len, int64_t hidden,
                                                  int64_t intermediate, int64_t num_layers, int last_layer_full) {
  (void)last_layer_full;   // both forms of the last layer use the same buffers
  if (!bgcn::encode_shape_ok(num_seqs, seq_len, hidden, intermediate, num_layers)) return 0;
  bgcn::EncWs w;
  bgcn::Carve c(nullptr, 0);
  bgcn::carve_encode(c, num_seqs * seq_len, num_seqs, hidden, intermediate, &w);
  return bgcn::align_up(c.off, 256);
}

extern "C" int bgcn_bert_encode(const bgcn_bert_encode_args* args, void* workspace, size_t workspace_bytes,
                                bgcn_stream_t stream) {
  return bgcn::encode_impl(args, workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream));
}
