// What the TreeBERT baseline's two translation units share.  bgcn_bert.hip owns the evaluation
// (both forms) and the kernels that open and close every call (k_bert_setup, k_bert_head, compiled
// once) and the shape limits; bgcn_bert_train.hip holds the training forward's row kernels and the
// backward.  Here: the LayerNorm of a row held by a wave, the GELU, and the host functions both use.
#pragma once
#include "bgcn_lstm.h"

namespace bgcn {

constexpr int kMaxPer = 16;   // values of one row per lane: hidden <= 64 kMaxPer (bgcn_bert.hip's kMaxHidden)

// ---- LayerNorm of one row held by one wave: lane l holds the columns l + 64 i, i < per.  Two
// passes over the registers (mean, then the centred squares), biased variance.  v is left centred
// (v - mean) and 1 / sqrt(var + eps) is returned: v[i] * inv is the normalised row.
__device__ __forceinline__ float ln_row(float (&v)[kMaxPer], int per, int H, const float* __restrict__ g,
                                        const float* __restrict__ be, float eps, int l, float* __restrict__ out,
                                        float* rowsum) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < kMaxPer; ++i)
    if (i < per) s += v[i];
  const float mean = wave_sum(s) / float(H);
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < kMaxPer; ++i)
    if (i < per) {
      v[i] -= mean;
      q = fmaf(v[i], v[i], q);
    }
  const float inv = 1.0f / sqrtf(wave_sum(q) / float(H) + eps);
  float rs = 0.f;
#pragma unroll
  for (int i = 0; i < kMaxPer; ++i)
    if (i < per) {
      const int c = l + kWave * i;
      const float y = fmaf(v[i] * inv, g[c], be[c]);
      out[c] = y;
      rs += y;
    }
  if (rowsum) {
    rs = wave_sum(rs);
    if (l == 0) *rowsum = rs;
  }
  return inv;
}

// GELU, the erf form
__device__ __forceinline__ float gelu_erf(float x) { return x * 0.5f * (1.0f + erff(x * 0.70710678118654752440f)); }

bool bert_shape_ok(int64_t N, int64_t B, int64_t H, int64_t I, int64_t L);
// everything bgcn_bert_args must satisfy but the workspace's size (the caller's last check)
int bert_check_args(const bgcn_bert_args* a, const void* ws);
// the call's first launch (k_bert_setup): the sequences' (start, len), *first, attn_sum zeroed, *status
void bert_setup(const bgcn_bert_args* a, SeqInfo sq, int64_t* first, hipStream_t s);
// the call's last launches: k_bert_head on P [B, hidden] (the pooler's GEMM without its bias), then
// seq_finish
int bert_head(const bgcn_bert_args* a, const float* P, float* loss_row, int32_t* predw, hipStream_t s);

// The two row kernels between the GEMMs (bgcn_bert.hip), also launched by the encoder over token ids
// (bgcn_bert_encode.hip).
// k_bert_add_ln: out[r] = LN(y[r] + bias + res[r]) over M rows of H columns, one wave per row; y and
// out have the row stride H, res the row stride ldres.  rowsum [M] and first [1] (rows below *first
// become zeros) may be null.
void bert_add_ln(const float* y, const float* bias, const float* res, int64_t ldres, const float* g, const float* be,
                 float* out, float* rowsum, const int64_t* first, int64_t M, int H, float eps, hipStream_t s);
// k_bert_bias_act: y[r][c] = act(y[r][c] + bias[c]) in place over [M, C], C % 4 == 0; gelu: the erf form
void bert_bias_act(float* y, const float* bias, int64_t M, int64_t C, bool gelu, hipStream_t s);

}  // namespace bgcn
