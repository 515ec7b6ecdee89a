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

// seq_start[0] as a row count in [0, N]: the rows above it belong to no sequence
__device__ __forceinline__ int64_t lstm_first_start(const int64_t* seq_start, int64_t N) {
  const int64_t s0 = seq_start[0];
  return s0 < 0 ? 0 : (s0 > N ? N : s0);
}

}  // namespace bgcn
