// The loss of EBGCN's training loop (EBGCN.py:301-306: nll_loss + edge_loss_td * TD_edge_loss +
// edge_loss_bu * BU_edge_loss), its accuracy (:311-312), the gradient the backward starts from
// and the step's skip decision, in one single-workgroup launch (a batch has ~128 trees of at most
// 16 classes: the launch, not the work, is what the dozen small torch kernels it replaces cost).
#include "bgcn_common.h"
#include "bgcn_internal.h"

namespace bgcn {
namespace {

struct TrainLossArgs {
  const float* logp;
  const int64_t* y;
  int64_t B;
  int C;
  const float* td_loss;
  const float* bu_loss;
  float w_td, w_bu;
  float* loss;
  int32_t* correct;
  int64_t* pred;
  float* dlogp;
  int32_t* status;
  float* skip_flag;
  int32_t* status_seen;
};

__global__ __launch_bounds__(256) void k_ebgcn_train_loss(TrainLossArgs a) {
  __shared__ float ls[4];
  __shared__ int32_t cs[4], bs[4];
  const int t = threadIdx.x;
  const int C = a.C;
  const float g = -1.0f / float(a.B);
  float sum = 0.f;
  int32_t n = 0, bad = 0;
  for (int64_t b = t; b < a.B; b += 256) {   // tree b on lane b % 256, in order
    const float* row = a.logp + b * C;
    const int64_t yb = a.y[b];
    const bool yok = yb >= 0 && yb < C;
    int best = 0;
    float bv = row[0];
    for (int c = 1; c < C; ++c) {
      const float v = row[c];
      if (v > bv) { bv = v; best = c; }   // the first maximum, as torch.max
    }
    for (int c = 0; c < C; ++c) a.dlogp[b * C + c] = (yok && c == yb) ? g : 0.f;
    if (a.pred) a.pred[b] = best;
    if (yok) sum += row[yb];
    n += (yb == int64_t(best)) ? 1 : 0;
    bad |= yok ? 0 : 1;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {   // a fixed butterfly
    sum += __shfl_xor(sum, m);
    n += __shfl_xor(n, m);
    bad |= __shfl_xor(bad, m);
  }
  if ((t & 63) == 0) {
    ls[t >> 6] = sum;
    cs[t >> 6] = n;
    bs[t >> 6] = bad;
  }
  __syncthreads();
  if (t == 0) {
    const float s = ((ls[0] + ls[1]) + ls[2]) + ls[3];   // the waves in order
    float loss = -s / float(a.B);
    if (a.td_loss) loss = fmaf(a.w_td, *a.td_loss, loss);
    if (a.bu_loss) loss = fmaf(a.w_bu, *a.bu_loss, loss);
    *a.loss = loss;
    *a.correct = cs[0] + cs[1] + cs[2] + cs[3];
    int32_t st = *a.status;
    if (bs[0] | bs[1] | bs[2] | bs[3]) st |= 2;
    *a.status = st;
    *a.skip_flag = st != 0 ? 1.0f : 0.0f;
    if (a.status_seen && st) atomicOr(a.status_seen, st);
  }
}

}  // namespace
}  // namespace bgcn

extern "C" int bgcn_ebgcn_train_loss(const float* logp, const int64_t* y, int64_t num_graphs, int32_t num_classes,
                                     const float* td_loss, const float* bu_loss, float edge_loss_td,
                                     float edge_loss_bu, float* loss, int32_t* correct, int64_t* pred, float* dlogp,
                                     int32_t* status, float* skip_flag, int32_t* status_seen, bgcn_stream_t stream) {
  using namespace bgcn;
  BGCN_CHECK_ARG(num_graphs >= 1, "train_loss: need at least one tree");
  BGCN_CHECK_ARG(num_classes >= 1 && num_classes <= kMaxClasses, "train_loss: num_classes must be in [1, 16]");
  BGCN_CHECK_ARG(logp && y && loss && correct && dlogp && status && skip_flag, "train_loss: null pointer");
  const TrainLossArgs a{logp, y, num_graphs, int(num_classes), td_loss, bu_loss, edge_loss_td, edge_loss_bu,
                        loss, correct, pred, dlogp, status, skip_flag, status_seen};
  hipLaunchKernelGGL(k_ebgcn_train_loss, dim3(1), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
  BGCN_CHECK_LAUNCH();
  return BGCN_OK;
}
