// bgcn_bert_eval: the TreeBERT baseline (model/Twitter/BERT_Twitter.py:20-42) in eval mode for a
// whole batch of trees as one launch sequence on the caller's stream, everything in the caller's
// workspace.  The model is BertModel(is_decoder = True) fed inputs_embeds, no attention mask: each
// tree is one sequence, the rows [seq_start[b], seq_start[b + 1]) of x (the last one runs to N), n
// of them, row t at position t:
//   embeddings  h = LN(x[t] + position_embeddings[t] + token_type_embeddings[0])   (biased variance,
//               eps = ln_eps; word_embeddings is never read)
//   per layer   q, k, v = Linear(h); per head (d = 64) P = softmax(q k^T / 8) over keys j <= t,
//               ctx = P v;  a = LN(dense(ctx) + h);  o = LN(dense2(gelu(dense1(a))) + a),
//               gelu(x) = x 0.5 (1 + erf(x / sqrt 2))
//   head        pooled = tanh(pooler.dense(o_last[0])), logp = log_softmax(fc(pooled))
//
// Root-only form (no hidden / hidden_sum / attn_sum asked for): position 0 attends to itself only
// and a softmax over one key is exactly 1, so ctx[0] = v[0] and the class is a function of the
// tree's first row.  The chain runs on [B, hidden]: no q, k or score, no row of x but the roots.
// Full form: all N rows through every layer.  logp then comes from the full pass's own root rows.
//
//   k_bert_setup       the sequences' (start, len), their validity (the status word), the first row
//                      that belongs to a sequence, attn_sum zeroed
//   k_bert_embed       x + position + type, LN: one wave per (sequence, position), early exit
//   per layer          GEMMs through gemm_xwt_impl (q | k as one product, v, attention-output
//                      dense, intermediate, output), bias in the row kernel that follows
//     k_bert_attn      full form: causal attention, one wave per (sequence, head, 32 queries)
//     k_bert_attn_sum  full form: this layer's column sums of P, added into attn_sum in a fixed order
//     k_bert_bias_act  root-only: v + bias;  both: intermediate + bias, gelu
//     k_bert_add_ln    LN(y + bias + residual); on the last layer also the row sums and the zero
//                      rows above the first sequence
//   k_bert_roots       full form: the root rows of last_hidden_state
//   k_bert_head        pooler bias + tanh, fc, log_softmax, NLL term, argmax (seq_head_tail)
//   seq_finish         mean loss and correct count
//
// Stream order is the only dependency between the launches.  No float atomics; every sum has a
// fixed order.
//
// bgcn_bert_eval_w16 is the root-only form on bf16 weight images: every GEMM a split-K product of
// bgcn_gemm_w16.hip, its partials added by k_bert_bias_act_part / k_bert_add_ln_part (the pooler's by
// k_w16_reduce); setup, embeddings, head and finish are the launches above.
#include "bgcn_bert.h"

namespace bgcn {
namespace {

constexpr int kHeadDim = 64;
constexpr int kQTile = BGCN_BERT_QUERY_TILE;
constexpr int kMaxPos = 512;
constexpr int kMaxHidden = 1024;
static_assert(kMaxHidden == kMaxPer * kWave, "ln_row holds a row in kMaxPer values per lane");
static_assert(kQTile == 32, "one 32x32 MFMA tile of scores per key tile");

// ---- setup (after k_lstm_setup).  Block 0: validity of seq_start over all sequences; one fault
// empties every sequence and makes every row one outside any sequence (first = N).  Every block:
// attn_sum = 0.
struct SetupArgs {
  const int64_t* seq_start;
  int64_t B, N, max_pos;
  SeqInfo sq;
  int64_t* first;     // [1] rows [0, first) belong to no sequence
  float* attn_sum;    // [N] or null
  int32_t* status;
};
__global__ __launch_bounds__(256) void k_bert_setup(SetupArgs a) {
  const int t = threadIdx.x;
  if (blockIdx.x == 0) {
    int bad = 0;
    for (int64_t b = t; b < a.B; b += 256) {
      const int64_t st = a.seq_start[b], en = b + 1 < a.B ? a.seq_start[b + 1] : a.N;
      bad |= (st < 0 || st >= a.N || en <= st || en > a.N || en - st > a.max_pos) ? 1 : 0;
    }
    bad = __syncthreads_or(bad);
    for (int64_t b = t; b < a.B; b += 256) {
      const int64_t st = a.seq_start[b], en = b + 1 < a.B ? a.seq_start[b + 1] : a.N;
      a.sq.start[b] = bad ? 0 : int32_t(st);
      a.sq.len[b] = bad ? 0 : int32_t(en - st);
    }
    if (t == 0) {
      *a.status = bad ? BGCN_STATUS_SEQUENCE : 0;   // the call's first launch
      *a.first = bad ? a.N : lstm_first_start(a.seq_start, a.N);
    }
  }
  if (a.attn_sum)
    for (int64_t i = int64_t(blockIdx.x) * 256 + t; i < a.N; i += int64_t(gridDim.x) * 256) a.attn_sum[i] = 0.f;
}

// ---- embeddings.  Wave (b, pos): dst row = LN(x[start + pos] + pos_emb[pos] + type_emb).  Full
// form: grid.y covers max_pos, the row lands at start + pos.  Root-only: pos = 0 only, the row
// lands at b (an emptied sequence gets a zero row, so the chain stays finite).
struct EmbedArgs {
  const float* x;
  int64_t ldx;
  const float *pos_emb, *type_emb, *g, *be;
  SeqInfo sq;
  float* dst;   // [M, H]
  int H;
  float eps;
  int root_only;
};
__global__ __launch_bounds__(256) void k_bert_embed(EmbedArgs a) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int64_t b = blockIdx.x;
  const int pos = blockIdx.y * 4 + w, len = a.sq.len[b], H = a.H, per = H >> 6;
  if (a.root_only ? pos != 0 : pos >= len) return;
  float* dst = a.dst + (a.root_only ? b : int64_t(a.sq.start[b]) + pos) * H;
  if (len == 0) {   // root-only, emptied
    for (int c = l; c < H; c += kWave) dst[c] = 0.f;
    return;
  }
  const float* xr = a.x + (int64_t(a.sq.start[b]) + pos) * a.ldx;
  const float* pe = a.pos_emb + int64_t(pos) * H;
  float v[kMaxPer];
#pragma unroll
  for (int i = 0; i < kMaxPer; ++i)
    if (i < per) {
      const int c = l + kWave * i;
      v[i] = (xr[c] + pe[c]) + a.type_emb[c];
    }
  ln_row(v, per, H, a.g, a.be, a.eps, l, dst, nullptr);
}

// ---- out[r] = LN(y[r] + bias + res[r]), one wave per row (res: rows ldres floats apart).  The last
// layer of the full form also writes the row's sum and zero rows above the first sequence (first,
// rowsum: null elsewhere).
struct AddLnArgs {
  const float *y, *bias, *res, *g, *be;
  float* out;
  float* rowsum;
  const int64_t* first;
  int64_t M, ldres;
  int H;
  float eps;
};
__global__ __launch_bounds__(256) void k_bert_add_ln(AddLnArgs a) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, H = a.H, per = H >> 6;
  const int64_t r = int64_t(blockIdx.x) * 4 + w;
  if (r >= a.M) return;
  float* out = a.out + r * H;
  if (a.first && r < *a.first) {
    for (int c = l; c < H; c += kWave) out[c] = 0.f;
    if (a.rowsum && l == 0) a.rowsum[r] = 0.f;
    return;
  }
  const float *y = a.y + r * H, *res = a.res + r * a.ldres;
  float v[kMaxPer];
#pragma unroll
  for (int i = 0; i < kMaxPer; ++i)
    if (i < per) {
      const int c = l + kWave * i;
      v[i] = (y[c] + a.bias[c]) + res[c];
    }
  ln_row(v, per, H, a.g, a.be, a.eps, l, out, a.rowsum ? a.rowsum + r : nullptr);
}

// ---- y[r][c] = act(y[r][c] + bias[c]) in place over [M, C], C % 4 == 0; GELU: the erf form (gelu_erf)
template <bool GELU>
__global__ __launch_bounds__(256) void k_bert_bias_act(float* __restrict__ y, const float* __restrict__ bias,
                                                       int64_t total4, int C4) {
  for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < total4; i += int64_t(gridDim.x) * 256) {
    const int c = int(i % C4) * 4;
    float4 v = f4add(ld4(y + i * 4), ld4(bias + c));
    if constexpr (GELU) v = make_float4(gelu_erf(v.x), gelu_erf(v.y), gelu_erf(v.z), gelu_erf(v.w));
    st4(y + i * 4, v);
  }
}

// ---- the two row kernels above for bgcn_bert_eval_w16: y is not a finished product but the S
// partials part[s][r][c] (stride floats apart) of the split-K GEMM (bgcn_gemm_w16.hip), added here in
// the order of s before the bias
__device__ __forceinline__ float4 part_sum4(const float* __restrict__ part, int S, int64_t stride, int64_t i) {
  // four loads in flight per step (one after the other, S memory latencies end to end); the order of
  // the additions is that of s
  float4 v = ld4(part + i);
  int s = 1;
  for (; s + 4 <= S; s += 4) {
    const float4 t0 = ld4(part + s * stride + i), t1 = ld4(part + (s + 1) * stride + i);
    const float4 t2 = ld4(part + (s + 2) * stride + i), t3 = ld4(part + (s + 3) * stride + i);
    v = f4add(f4add(f4add(f4add(v, t0), t1), t2), t3);
  }
  for (; s < S; ++s) v = f4add(v, ld4(part + s * stride + i));
  return v;
}
struct AddLnPartArgs {
  const float *part, *bias, *res, *g, *be;
  float* out;
  int64_t M, stride;
  int S, H;
  float eps;
};
__global__ __launch_bounds__(256) void k_bert_add_ln_part(AddLnPartArgs a) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, H = a.H, per = H >> 6;
  const int64_t r = int64_t(blockIdx.x) * 4 + w;
  if (r >= a.M) return;
  const float *y = a.part + r * H, *res = a.res + r * H;
  float v[kMaxPer];
#pragma unroll
  for (int i = 0; i < kMaxPer; ++i)
    if (i < per) v[i] = y[l + kWave * i];
  int s = 1;
  for (; s + 4 <= a.S; s += 4) {   // 4 per loads in flight; added in the order of s
    float t[4][kMaxPer];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int i = 0; i < kMaxPer; ++i)
        if (i < per) t[u][i] = y[(s + u) * a.stride + l + kWave * i];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int i = 0; i < kMaxPer; ++i)
        if (i < per) v[i] += t[u][i];
  }
  for (; s < a.S; ++s)
#pragma unroll
    for (int i = 0; i < kMaxPer; ++i)
      if (i < per) v[i] += y[s * a.stride + l + kWave * i];
#pragma unroll
  for (int i = 0; i < kMaxPer; ++i)
    if (i < per) {
      const int c = l + kWave * i;
      v[i] = (v[i] + a.bias[c]) + res[c];
    }
  ln_row(v, per, H, a.g, a.be, a.eps, l, a.out + r * H, nullptr);
}
template <bool GELU>
__global__ __launch_bounds__(256) void k_bert_bias_act_part(const float* __restrict__ part, int S, int64_t stride,
                                                            const float* __restrict__ bias, float* __restrict__ out,
                                                            int64_t total4, int C4) {
  for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < total4; i += int64_t(gridDim.x) * 256) {
    const int c = int(i % C4) * 4;
    float4 v = f4add(part_sum4(part, S, stride, i * 4), ld4(bias + c));
    if constexpr (GELU) v = make_float4(gelu_erf(v.x), gelu_erf(v.y), gelu_erf(v.z), gelu_erf(v.w));
    st4(out + i * 4, v);
  }
}

// ---- causal attention of one head, one wave per (query tile qt, head, sequence b): the queries
// [32 qt, 32 qt + 32) against the key tiles 0 .. qt.  Both products run on v_mfma_f32_32x32x2_f32.
//   scores  S^T[key][query] = sum_k K[key][k] Q[query][k]: lane (j = l & 31, h = l >> 5) holds
//           8 consecutive k of row j of K (A operand) and of Q (B operand) per 16-k block
//           (16 i + 8 h ..); MFMA (i, t) pairs k = 16 i + t with 16 i + 8 + t on both.  Register
//           4 g + u of lane (j, h) is key 8 g + 4 h + u of the tile against query j: a query's
//           scores of one tile sit in the two lanes j and j + 32, so its maximum and its
//           normaliser are 16 in-lane steps and one exchange.
//   pass 1  over the key tiles: the running maximum m and sum l of exp(s - m) per query
//   pass 2  the same scores again, p = exp(s - m) / l (0 above the diagonal and for the rows of
//           the tile past the sequence's end); ctx^T[d][query] += V^T[d][key] P^T[key][query]
//           takes register 4 g + u as the B operand of MFMA (g, u) with no lane movement (lane
//           (d, h) loads V[key 8 g + 4 h + u][d]); the column sums of P (over the tile's queries:
//           the 32 lanes of one half) go to part[qt][head][row of the key], one writer each.
// Rows past the end of the sequence are read as the sequence's last row (in bounds, finite).
struct AttnArgs {
  const float* qkv;   // [N, 3H]: q | k | v
  const float *bq, *bk, *bv;
  float* ctx;         // [N, H]
  float* part;        // [max_pos / 32][heads][N] or null
  SeqInfo sq;
  int64_t N;
  int H, heads;
};
__device__ __forceinline__ void ld8_bias(const float* p, const float* b, float* dst) {
  const float4 x0 = f4add(ld4(p), ld4(b)), x1 = f4add(ld4(p + 4), ld4(b + 4));
  dst[0] = x0.x; dst[1] = x0.y; dst[2] = x0.z; dst[3] = x0.w;
  dst[4] = x1.x; dst[5] = x1.y; dst[6] = x1.z; dst[7] = x1.w;
}
__device__ __forceinline__ f32x16 attn_scores(const AttnArgs& a, const float (&q)[32], int64_t start, int len, int kt,
                                              int head, int j, int h, int qi) {
  const int krow = min(kt * kQTile + j, len - 1);
  const float* kp = a.qkv + (start + krow) * (3 * int64_t(a.H)) + a.H + head * kHeadDim + 8 * h;
  const float* bp = a.bk + head * kHeadDim + 8 * h;
  float k[32];
#pragma unroll
  for (int i = 0; i < 4; ++i) ld8_bias(kp + 16 * i, bp + 16 * i, &k[8 * i]);
  f32x16 s;
#pragma unroll
  for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
  for (int i = 0; i < 32; ++i) s = mfma32x32x2(k[i], q[i], s);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int key = kt * kQTile + 8 * (r >> 2) + 4 * h + (r & 3);
    s[r] = key <= qi ? s[r] * 0.125f : -INFINITY;
  }
  return s;
}
__global__ __launch_bounds__(64) void k_bert_attn(AttnArgs a) {
  const int l = threadIdx.x, j = l & 31, h = l >> 5;
  const int qt = blockIdx.x, head = blockIdx.y;
  const int64_t b = blockIdx.z;
  const int len = a.sq.len[b], q0 = qt * kQTile;
  if (q0 >= len) return;
  const int64_t start = a.sq.start[b], ld = 3 * int64_t(a.H);
  const bool qvalid = q0 + j < len;
  const int qi = min(q0 + j, len - 1);
  float q[32];
  {
    const float* qp = a.qkv + (start + qi) * ld + head * kHeadDim + 8 * h;
    const float* bp = a.bq + head * kHeadDim + 8 * h;
#pragma unroll
    for (int i = 0; i < 4; ++i) ld8_bias(qp + 16 * i, bp + 16 * i, &q[8 * i]);
  }
  // pass 1: every tile holds a key <= qi for one of the lanes j, j + 32 (key 32 kt <= q0), so m is
  // finite after the exchange
  float m = -INFINITY, lsum = 0.f;
  for (int kt = 0; kt <= qt; ++kt) {
    const f32x16 s = attn_scores(a, q, start, len, kt, head, j, h, qi);
    float tm = s[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) tm = fmaxf(tm, s[r]);
    tm = fmaxf(tm, __shfl_xor(tm, 32));
    const float mn = fmaxf(m, tm);
    float e = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) e += expf(s[r] - mn);
    lsum = lsum * expf(m - mn) + e;
    m = mn;
  }
  lsum += __shfl_xor(lsum, 32);

  f32x16 acc[2];
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[0][r] = acc[1][r] = 0.f;
  for (int kt = 0; kt <= qt; ++kt) {
    f32x16 p = attn_scores(a, q, start, len, kt, head, j, h, qi);
#pragma unroll
    for (int r = 0; r < 16; ++r) p[r] = qvalid ? expf(p[r] - m) / lsum : 0.f;
    if (a.part) {
      float* part = a.part + (int64_t(qt) * a.heads + head) * a.N + start;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float c = p[r];
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) c += __shfl_xor(c, o);
        const int key = kt * kQTile + 8 * (r >> 2) + 4 * h + (r & 3);
        if (j == 0 && key < len) part[key] = c;
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int vrow = min(kt * kQTile + 8 * (r >> 2) + 4 * h + (r & 3), len - 1);
      const float* vp = a.qkv + (start + vrow) * ld + 2 * a.H + head * kHeadDim + j;
      acc[0] = mfma32x32x2(vp[0], p[r], acc[0]);
      acc[1] = mfma32x32x2(vp[32], p[r], acc[1]);
    }
  }
  if (!qvalid) return;
  float* out = a.ctx + (start + q0 + j) * a.H + head * kHeadDim;
  const float* bv = a.bv + head * kHeadDim;
#pragma unroll
  for (int dh = 0; dh < 2; ++dh)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int d = 32 * dh + 8 * g + 4 * h;
      st4(out + d, f4add(make_float4(acc[dh][4 * g], acc[dh][4 * g + 1], acc[dh][4 * g + 2], acc[dh][4 * g + 3]),
                         ld4(bv + d)));
    }
}

// ---- attn_sum[row of key i] += sum over the query tiles that reach key i (i / 32 .. (len - 1) / 32)
// and, inside each, the heads in order, of this layer's partial column sums
__global__ __launch_bounds__(256) void k_bert_attn_sum(const float* __restrict__ part, SeqInfo sq, int64_t N,
                                                       int heads, float* __restrict__ attn_sum) {
  const int64_t b = blockIdx.x;
  const int i = blockIdx.y * 256 + threadIdx.x, len = sq.len[b];
  if (i >= len) return;
  const int64_t row = int64_t(sq.start[b]) + i;
  float s = 0.f;
  for (int qt = i / kQTile; qt <= (len - 1) / kQTile; ++qt)
    for (int hd = 0; hd < heads; ++hd) s += part[(int64_t(qt) * heads + hd) * N + row];
  attn_sum[row] += s;
}

// ---- the root rows of last_hidden_state [N, H] into R [B, H] (zeros for an emptied sequence)
__global__ __launch_bounds__(256) void k_bert_roots(const float* __restrict__ hid, SeqInfo sq, int H,
                                                    float* __restrict__ R) {
  const int64_t b = blockIdx.x;
  const bool ok = sq.len[b] > 0;
  const float* src = hid + int64_t(sq.start[b]) * H;
  for (int c = threadIdx.x; c < H; c += 256) R[b * H + c] = ok ? src[c] : 0.f;
}

// ---- head, workgroup b = sequence b: pooled = tanh(P[b] + pooler bias) (P = the pooler's GEMM),
// fc by the four waves (class c by wave c % 4), then wave 0: seq_head_tail
struct BertHeadArgs {
  const float *P, *pb, *W, *bias;   // [B, H], [H], [C, H], [C]
  int H, C;
  const int64_t* y;
  float *logp, *loss_row;
  int32_t* predw;
  int64_t* pred;
  int32_t* status;
};
__global__ __launch_bounds__(256) void k_bert_head(BertHeadArgs a) {
  __shared__ __attribute__((aligned(16))) float pooled[kMaxHidden];
  __shared__ float z[kMaxOut];
  const int t = threadIdx.x, w = t >> 6, l = t & 63, H = a.H;
  const int64_t b = blockIdx.x;
  for (int c = t; c < H; c += 256) pooled[c] = tanhf(a.P[b * H + c] + a.pb[c]);
  __syncthreads();
  for (int c = w; c < a.C; c += 4) {
    const float* wr = a.W + int64_t(c) * H;
    float p = 0.f;
    for (int k = 4 * l; k < H; k += 256) {
      const float4 x = ld4(&pooled[k]), v = ld4(wr + k);
      p = fmaf(x.x, v.x, fmaf(x.y, v.y, fmaf(x.z, v.z, fmaf(x.w, v.w, p))));
    }
    p = wave_sum(p);
    if (l == 0) z[c] = p + a.bias[c];
  }
  __syncthreads();
  if (w != 0) return;
  seq_head_tail(z, a.C, b, l, a.y, a.logp, a.loss_row, a.predw, a.pred, a.status);
}

// ---- host
struct BertWs {
  float *h, *a, *t, *ctx, *qkv, *inter, *part, *R, *P;
  SeqInfo sq;
  float* loss_row;
  int32_t* predw;
  int64_t* first;
};

}  // namespace

void bert_add_ln(const float* y, const float* bias, const float* res, int64_t ldres, const float* g, const float* be,
                 float* out, float* rowsum, const int64_t* first, int64_t M, int H, float eps, hipStream_t s) {
  AddLnArgs a{y, bias, res, g, be, out, rowsum, first, M, ldres, H, eps};
  hipLaunchKernelGGL(k_bert_add_ln, dim3(grid_for(M, 4)), dim3(256), 0, s, a);
}

void bert_bias_act(float* y, const float* bias, int64_t M, int64_t C, bool gelu, hipStream_t s) {
  const int64_t total4 = M * C / 4;
  const dim3 grid(unsigned(std::min<int64_t>((total4 + 255) / 256, 4096)));
  if (gelu)
    hipLaunchKernelGGL(k_bert_bias_act<true>, grid, dim3(256), 0, s, y, bias, total4, int(C / 4));
  else
    hipLaunchKernelGGL(k_bert_bias_act<false>, grid, dim3(256), 0, s, y, bias, total4, int(C / 4));
}

bool bert_shape_ok(int64_t N, int64_t B, int64_t H, int64_t I, int64_t L) {
  return N > 0 && B > 0 && N < (int64_t(1) << 31) - 1 && B <= 65535 && H % kHeadDim == 0 && H >= 64 &&
         H <= kMaxHidden && I % 64 == 0 && I >= 64 && I <= 4096 && L >= 1 && L <= BGCN_BERT_MAX_LAYERS;
}

static void carve_bert(Carve& c, int64_t N, int64_t B, int64_t H, int64_t I, bool full, BertWs* w) {
  const size_t m = size_t(full ? N : B), nb = size_t(B), h = size_t(H);
  w->h = c.take<float>(m * h);
  w->a = c.take<float>(m * h);
  w->t = c.take<float>(m * h);
  w->ctx = c.take<float>(m * h);
  w->inter = c.take<float>(m * size_t(I));
  w->qkv = full ? c.take<float>(m * 3 * h) : nullptr;
  w->part = full ? c.take<float>(size_t(kMaxPos / kQTile) * size_t(H / kHeadDim) * m) : nullptr;
  w->R = full ? c.take<float>(nb * h) : nullptr;
  w->P = c.take<float>(nb * h);
  w->sq.start = c.take<int32_t>(nb);
  w->sq.len = c.take<int32_t>(nb);
  w->loss_row = c.take<float>(nb);
  w->predw = c.take<int32_t>(nb);
  w->first = c.take<int64_t>(1);
}

int bert_check_args(const bgcn_bert_args* a, const void* ws) {
  BGCN_CHECK_ARG(a, "null args");
  BGCN_CHECK_ARG(bert_shape_ok(a->num_nodes, a->num_seqs, a->hidden, a->intermediate, a->num_layers) &&
                     a->heads * kHeadDim == a->hidden && a->max_pos >= 1 && a->max_pos <= kMaxPos &&
                     a->out_feats >= 1 && a->out_feats <= kMaxOut,
                 "unsupported shape (hidden = 64 heads in [64, 1024], intermediate % 64 in [64, 4096], layers in "
                 "[1, 24], max_pos in [1, 512], out_feats in [1, 64])");
  BGCN_CHECK_ARG(a->x && a->seq_start && a->logp && a->status, "null pointer");
  BGCN_CHECK_ARG(a->ldx >= a->hidden && a->ldx % 4 == 0 && a16(a->x), "x rows must be 16-byte aligned (ldx % 4)");
  const float* emb[] = {a->pos_emb, a->type_emb, a->emb_ln_w, a->emb_ln_b, a->pooler_w, a->pooler_b, a->fc_w, a->fc_b};
  for (const float* p : emb) BGCN_CHECK_ARG(p && a16(p), "null or unaligned BERT weight");
  for (int l = 0; l < a->num_layers; ++l) {
    const bgcn_bert_layer& y = a->layer[l];
    const float* lw[] = {y.q_w, y.q_b, y.k_w, y.k_b, y.v_w, y.v_b, y.ao_w, y.ao_b, y.ao_ln_w, y.ao_ln_b,
                         y.i_w, y.i_b, y.o_w, y.o_b, y.o_ln_w, y.o_ln_b};
    for (const float* p : lw) BGCN_CHECK_ARG(p && a16(p), "null or unaligned BERT weight");
  }
  BGCN_CHECK_ARG(a16(a->logp) && a16(a->hidden_out) && a16(a->hidden_sum) && a16(a->attn_sum) && a16(ws),
                 "logp, hidden, hidden_sum, attn_sum and the workspace must be 16-byte aligned");
  return BGCN_OK;
}

void bert_setup(const bgcn_bert_args* a, SeqInfo sq, int64_t* first, hipStream_t s) {
  SetupArgs su{a->seq_start, a->num_seqs, a->num_nodes, a->max_pos, sq, first, a->attn_sum, a->status};
  hipLaunchKernelGGL(k_bert_setup, dim3(64), dim3(256), 0, s, su);
}

int bert_head(const bgcn_bert_args* a, const float* P, float* loss_row, int32_t* predw, hipStream_t s) {
  BertHeadArgs hd{P, a->pooler_b, a->fc_w, a->fc_b, int(a->hidden), int(a->out_feats), a->y, a->logp, loss_row,
                  predw, a->pred, a->status};
  hipLaunchKernelGGL(k_bert_head, dim3(unsigned(a->num_seqs)), dim3(256), 0, s, hd);
  BGCN_CHECK_LAUNCH();
  return seq_finish(loss_row, predw, a->y, a->num_seqs, a->loss, a->correct, s);
}

static int bert_eval_impl(const bgcn_bert_args* a, void* ws, size_t ws_bytes, hipStream_t s) {
  BGCN_TRY(bert_check_args(a, ws));
  const int64_t N = a->num_nodes, B = a->num_seqs, H = a->hidden, I = a->intermediate, L = a->num_layers;
  const bool full = a->hidden_out || a->hidden_sum || a->attn_sum;
  BertWs w;
  Carve c(ws, ws_bytes);
  carve_bert(c, N, B, H, I, full, &w);
  BGCN_CHECK_ARG(ws && align_up(c.off, 256) <= ws_bytes, "workspace too small");   // bgcn_bert_workspace_size's figure
  const int64_t M = full ? N : B;
  const int heads = int(a->heads);

  bert_setup(a, w.sq, w.first, s);
  EmbedArgs em{a->x, a->ldx, a->pos_emb, a->type_emb, a->emb_ln_w, a->emb_ln_b, w.sq, w.h, int(H), a->ln_eps, full ? 0 : 1};
  hipLaunchKernelGGL(k_bert_embed, dim3(unsigned(B), full ? grid_for(a->max_pos, 4) : 1), dim3(256), 0, s, em);
  BGCN_CHECK_LAUNCH();

  for (int l = 0; l < L; ++l) {
    const bgcn_bert_layer& y = a->layer[l];
    const bool last = l == L - 1;
    if (full) {
      BGCN_TRY(gemm_xwt_impl(w.h, H, y.q_w, y.k_w, H, H, w.qkv, 3 * H, M, 2 * H, H, s, nullptr));
      BGCN_TRY(gemm_xwt_impl(w.h, H, y.v_w, nullptr, H, H, w.qkv + 2 * H, 3 * H, M, H, H, s, nullptr));
      AttnArgs at{w.qkv, y.q_b, y.k_b, y.v_b, w.ctx, a->attn_sum ? w.part : nullptr, w.sq, N, int(H), heads};
      hipLaunchKernelGGL(k_bert_attn, dim3(grid_for(a->max_pos, kQTile), unsigned(heads), unsigned(B)), dim3(64), 0, s,
                         at);
      if (a->attn_sum)
        hipLaunchKernelGGL(k_bert_attn_sum, dim3(unsigned(B), grid_for(a->max_pos, 256)), dim3(256), 0, s, w.part, w.sq,
                           N, heads, a->attn_sum);
    } else {   // P = 1 at position 0: ctx = v
      BGCN_TRY(gemm_xwt_impl(w.h, H, y.v_w, nullptr, H, H, w.ctx, H, M, H, H, s, nullptr));
      bert_bias_act(w.ctx, y.v_b, M, H, false, s);
    }
    BGCN_CHECK_LAUNCH();
    BGCN_TRY(gemm_xwt_impl(w.ctx, H, y.ao_w, nullptr, H, H, w.t, H, M, H, H, s, nullptr));
    bert_add_ln(w.t, y.ao_b, w.h, H, y.ao_ln_w, y.ao_ln_b, w.a, nullptr, nullptr, M, int(H), a->ln_eps, s);
    BGCN_TRY(gemm_xwt_impl(w.a, H, y.i_w, nullptr, H, I, w.inter, I, M, I, H, s, nullptr));
    bert_bias_act(w.inter, y.i_b, M, I, true, s);
    BGCN_TRY(gemm_xwt_impl(w.inter, I, y.o_w, nullptr, I, H, w.t, H, M, H, I, s, nullptr));
    const bool fin = full && last;
    bert_add_ln(w.t, y.o_b, w.a, H, y.o_ln_w, y.o_ln_b, fin && a->hidden_out ? a->hidden_out : w.h,
                fin ? a->hidden_sum : nullptr, fin ? w.first : nullptr, M, int(H), a->ln_eps, s);
    BGCN_CHECK_LAUNCH();
  }

  const float* roots = w.h;
  if (full) {
    hipLaunchKernelGGL(k_bert_roots, dim3(unsigned(B)), dim3(256), 0, s, a->hidden_out ? a->hidden_out : w.h, w.sq,
                       int(H), w.R);
    roots = w.R;
  }
  BGCN_TRY(gemm_xwt_impl(roots, H, a->pooler_w, nullptr, H, H, w.P, H, B, H, H, s, nullptr));
  return bert_head(a, w.P, w.loss_row, w.predw, s);
}

// ---- the root-only form on bf16 weight images: bert_eval_impl's root-only branch with every GEMM
// a split-K product on an image (gemm_w16_partials) whose partials the next row kernel adds
static size_t bert_w16_part_floats(int64_t B, int64_t H, int64_t I) {
  return std::max({w16_part_floats(B, H, H), w16_part_floats(B, I, H), w16_part_floats(B, H, I)});
}

static int bert_eval_w16_impl(const bgcn_bert_w16_args* wa, void* ws, size_t ws_bytes, hipStream_t s) {
  BGCN_CHECK_ARG(wa, "null args");
  const bgcn_bert_args* a = &wa->base;
  BGCN_TRY(bert_check_args(a, ws));
  BGCN_CHECK_ARG(!a->hidden_out && !a->hidden_sum && !a->attn_sum,
                 "bgcn_bert_eval_w16 is the root-only form: hidden_out, hidden_sum and attn_sum must be NULL");
  const int64_t N = a->num_nodes, B = a->num_seqs, H = a->hidden, I = a->intermediate, L = a->num_layers;
  for (int l = 0; l < L; ++l)
    for (const void* p : {wa->v_w16[l], wa->ao_w16[l], wa->i_w16[l], wa->o_w16[l]})
      BGCN_CHECK_ARG(p && a16(p), "null or unaligned weight image");
  BGCN_CHECK_ARG(wa->pooler_w16 && a16(wa->pooler_w16), "null or unaligned weight image");
  BertWs w;
  Carve c(ws, ws_bytes);
  carve_bert(c, N, B, H, I, false, &w);
  float* part = c.take<float>(bert_w16_part_floats(B, H, I));
  BGCN_CHECK_ARG(ws && align_up(c.off, 256) <= ws_bytes, "workspace too small");   // bgcn_bert_w16_workspace_size's figure
  const unsigned rows4 = grid_for(B, 4);
  const int Shh = w16_splits(H, H), Sih = w16_splits(I, H), Shi = w16_splits(H, I);

  bert_setup(a, w.sq, w.first, s);
  EmbedArgs em{a->x, a->ldx, a->pos_emb, a->type_emb, a->emb_ln_w, a->emb_ln_b, w.sq, w.h, int(H), a->ln_eps, 1};
  hipLaunchKernelGGL(k_bert_embed, dim3(unsigned(B), 1), dim3(256), 0, s, em);
  BGCN_CHECK_LAUNCH();

  const auto bias_grid = [](int64_t total4) { return dim3(unsigned(std::min<int64_t>((total4 + 255) / 256, 4096))); };
  for (int l = 0; l < L; ++l) {
    const bgcn_bert_layer& y = a->layer[l];
    BGCN_TRY(gemm_w16_partials(w.h, H, wa->v_w16[l], part, B, H, H, s));   // P = 1 at position 0: ctx = v
    hipLaunchKernelGGL(k_bert_bias_act_part<false>, bias_grid(B * H / 4), dim3(256), 0, s, part, Shh, B * H, y.v_b,
                       w.ctx, B * H / 4, int(H / 4));
    BGCN_TRY(gemm_w16_partials(w.ctx, H, wa->ao_w16[l], part, B, H, H, s));
    AddLnPartArgs l1{part, y.ao_b, w.h, y.ao_ln_w, y.ao_ln_b, w.a, B, B * H, Shh, int(H), a->ln_eps};
    hipLaunchKernelGGL(k_bert_add_ln_part, dim3(rows4), dim3(256), 0, s, l1);
    BGCN_TRY(gemm_w16_partials(w.a, H, wa->i_w16[l], part, B, I, H, s));
    hipLaunchKernelGGL(k_bert_bias_act_part<true>, bias_grid(B * I / 4), dim3(256), 0, s, part, Sih, B * I, y.i_b,
                       w.inter, B * I / 4, int(I / 4));
    BGCN_TRY(gemm_w16_partials(w.inter, I, wa->o_w16[l], part, B, H, I, s));
    AddLnPartArgs l2{part, y.o_b, w.a, y.o_ln_w, y.o_ln_b, w.h, B, B * H, Shi, int(H), a->ln_eps};
    hipLaunchKernelGGL(k_bert_add_ln_part, dim3(rows4), dim3(256), 0, s, l2);
    BGCN_CHECK_LAUNCH();
  }
  BGCN_TRY(gemm_w16_partials(w.h, H, wa->pooler_w16, part, B, H, H, s));
  BGCN_TRY(w16_reduce(part, Shh, B, H, nullptr, w.P, H, s));
  return bert_head(a, w.P, w.loss_row, w.predw, s);
}

}  // namespace bgcn

extern "C" size_t bgcn_bert_w16_workspace_size(int64_t num_seqs, int64_t hidden, int64_t intermediate,
                                               int64_t num_layers) {
  if (!bgcn::bert_shape_ok(num_seqs, num_seqs, hidden, intermediate, num_layers)) return 0;
  bgcn::BertWs w;
  bgcn::Carve c(nullptr, 0);
  bgcn::carve_bert(c, num_seqs, num_seqs, hidden, intermediate, false, &w);
  c.take<float>(bgcn::bert_w16_part_floats(num_seqs, hidden, intermediate));
  return bgcn::align_up(c.off, 256);
}

extern "C" int bgcn_bert_eval_w16(const bgcn_bert_w16_args* args, void* workspace, size_t workspace_bytes,
                                  bgcn_stream_t stream) {
  return bgcn::bert_eval_w16_impl(args, workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream));
}

extern "C" size_t bgcn_bert_workspace_size(int64_t num_nodes, int64_t num_seqs, int64_t hidden, int64_t intermediate,
                                           int64_t num_layers, int want_full) {
  if (!bgcn::bert_shape_ok(num_nodes, num_seqs, hidden, intermediate, num_layers)) return 0;
  bgcn::BertWs w;
  bgcn::Carve c(nullptr, 0);
  bgcn::carve_bert(c, num_nodes, num_seqs, hidden, intermediate, want_full != 0, &w);
  return bgcn::align_up(c.off, 256);
}

extern "C" int bgcn_bert_eval(const bgcn_bert_args* args, void* workspace, size_t workspace_bytes,
                              bgcn_stream_t stream) {
  return bgcn::bert_eval_impl(args, workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream));
}
