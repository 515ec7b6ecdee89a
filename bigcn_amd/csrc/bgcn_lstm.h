// What the LSTM baseline's two translation units share.  bgcn_lstm.hip owns the forward (its four
// kernels, compiled once, and lstm_forward, which both entry points call); bgcn_lstm_train.hip
// holds the backward.  Here: the constants, the forward's share of the workspace, the forward's
// host functions and the clamp of seq_start[0] that both setup kernels use.
#pragma once
#include "bgcn_internal.h"

namespace bgcn {

constexpr int kSeqTile = BGCN_LSTM_SEQ_TILE;   // sequences per workgroup of a step: the MFMA's 32 columns
constexpr int kMaxLayers = 4;
constexpr int kMaxOut = 64;
static_assert(kSeqTile == 32, "one 32x32 MFMA tile per workgroup");

struct SeqInfo {
  int32_t* start;   // [B]
  int32_t* len;     // [B] 0: the sequence is not evaluated
};

// The forward's share of the workspace.  save (the training forward): per layer the gates G[l],
// activated in place, and the cell states C[l]; else every layer goes through G[0] and C is null.
struct LstmFwdWs {
  float* G[kMaxLayers];   // [N, 8H]
  float* Y[kMaxLayers];   // [N, 2H]
  float* C[kMaxLayers];   // [N, 2H]
  float* c;               // [2, B, H]
  SeqInfo sq;
  float* loss_row;
  int32_t* predw;
};

bool lstm_shape_ok(int64_t N, int64_t B, int64_t F, int64_t H, int64_t L);
// everything bgcn_lstm_args must satisfy but the workspace's size (the caller's last check)
int lstm_check_args(const bgcn_lstm_args* a, const void* ws);
// out (may be null): the caller's [N, 2H] takes the place of the last layer's Y
void carve_lstm_fwd(Carve& c, int64_t N, int64_t B, int64_t H, int64_t L, bool save, float* out, LstmFwdWs* w);
// setup, per layer the input GEMM and the steps, head, finish; h_n may be null
int lstm_forward(const bgcn_lstm_args* a, const LstmFwdWs& w, bool save, float* h_n, hipStream_t s);

// the mean NLL and the correct count over B sequences from their loss terms and predictions (one
// workgroup, fixed order); nothing is launched when loss and correct are both null.  Shared with the
// TreeBERT entry point (bgcn_bert.hip), whose head ends the same way.
int seq_finish(const float* loss_row, const int32_t* predw, const int64_t* y, int64_t B, float* loss,
               int32_t* correct, hipStream_t s);

// The end of a sequence's head, one wave (lane l): log_softmax of the C <= 64 logits z, the NLL
// term, the first maximal class (torch's max); a label outside [0, C) adds no loss and sets
// BGCN_STATUS_SEQUENCE.
__device__ __forceinline__ void seq_head_tail(const float* z, int C, int64_t b, int l, const int64_t* y, float* logp,
                                              float* loss_row, int32_t* predw, int64_t* pred, int32_t* status) {
  const bool in = l < C;
  const float zc = in ? z[l] : -INFINITY;
  float mx = zc;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  const float lse = mx + logf(wave_sum(in ? expf(zc - mx) : 0.f));
  const float lp = zc - lse;
  if (in && logp) logp[b * C + l] = lp;
  float bv = lp;
  int bi = l;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {   // the first maximal class, as torch's max
    const float ov = __shfl_xor(bv, o);
    const int oi = __shfl_xor(bi, o);
    if (ov > bv || (ov == bv && oi < bi)) {
      bv = ov;
      bi = oi;
    }
  }
  const int64_t yb = y ? y[b] : 0;
  const bool yok = y && yb >= 0 && yb < C;
  const float ly = __shfl(lp, yok ? int(yb) : 0);
  if (l == 0) {
    loss_row[b] = yok ? -ly : 0.f;
    predw[b] = bi;
    if (pred) pred[b] = bi;
    if (y && !yok) atomicOr(status, BGCN_STATUS_SEQUENCE);
  }
}

// seq_start[0] as a row count in [0, N]: the rows above it belong to no sequence
__device__ __forceinline__ int64_t lstm_first_start(const int64_t* seq_start, int64_t N) {
  const int64_t s0 = seq_start[0];
  return s0 < 0 ? 0 : (s0 > N ? N : s0);
}

}  // namespace bgcn
