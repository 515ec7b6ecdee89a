// The metric side of the reference's validation loop (tools/evaluate.py:3-139 called from
// BiGCN_Twitter.py:223) and of its explain run's bookkeeping (explain_PHEME.py:480, 609): every
// number they report derives from how often label a met prediction p.
//
// bgcn_confusion - counts[a * C + p] = #{i : y[i] = a, pred[i] = p}, int32, in ONE launch of ONE
// workgroup of four waves:
//   - every wave counts into its own C * C bins in LDS (at most 256 int32 each, 4 KiB in all) with
//     integer LDS atomics: the 64 lanes of a wave that meet in one bin (with C = 4 there are 16)
//     serialise there, the four waves do not disturb each other;
//   - the four copies are summed and bin q is written by thread q: a plain store when the call
//     overwrites (no zeroing launch, no memset: all C * C bins are written whatever B is), a plain
//     read-add-store when it accumulates (the single workgroup owns the buffer for the launch, and
//     launches on one stream are ordered, so no atomic is needed in global memory);
//   - integer adds only: exact, and the same on every run whatever order the atomics land in.
// The entries are read grid-stride by the 256 threads, so B is any size; a validation batch is a
// few hundred trees, far below what a second workgroup would pay for (it would need the zeroing
// pass this launch saves).  An entry outside [0, C) is not counted: its bin index is never formed,
// and bit 0 of *status is set (the library's convention for a data-dependent index error).
#include "bgcn_internal.h"

namespace bgcn {
namespace {

constexpr int kBins = kMaxClasses * kMaxClasses;   // 256 (the head's class limit): one bin per thread at the write-out
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
static_assert(kBins == kThreads, "thread q writes bin q");

__global__ __launch_bounds__(kThreads) void k_confusion(const int64_t* __restrict__ pred,
                                                        const int64_t* __restrict__ y, int64_t B, int C,
                                                        int32_t* __restrict__ counts, int accumulate,
                                                        int32_t* __restrict__ status) {
  __shared__ int32_t bins[kWaves][kBins];
  const int tid = threadIdx.x;
  for (int w = 0; w < kWaves; ++w) bins[w][tid] = 0;
  __syncthreads();
  int32_t* mine = bins[tid / 64];
  int bad = 0;
  for (int64_t i = tid; i < B; i += kThreads) {
    const int64_t a = y[i], p = pred[i];
    if (a >= 0 && a < C && p >= 0 && p < C) {
      atomicAdd(&mine[int(a) * C + int(p)], 1);
    } else {
      bad = 1;
    }
  }
  bad = __syncthreads_or(bad);   // (also orders the LDS atomics before the reads below)
  if (tid < C * C) {
    int32_t n = 0;
    for (int w = 0; w < kWaves; ++w) n += bins[w][tid];
    counts[tid] = accumulate ? counts[tid] + n : n;
  }
  if (bad && tid == 0) atomicOr(status, 1);
}

}  // namespace

int confusion_impl(const int64_t* pred, const int64_t* y, int64_t B, int C, int32_t* counts, int accumulate,
                   int32_t* status, hipStream_t s) {
  BGCN_CHECK_ARG(C >= 1 && C <= kMaxClasses, "confusion: num_classes must be in [1, 16]");
  BGCN_CHECK_ARG(B >= 0, "confusion: negative size");
  BGCN_CHECK_ARG(pred && y && counts && status, "confusion: null pointer");
  if (B == 0 && accumulate) return BGCN_OK;   // nothing to add
  hipLaunchKernelGGL(k_confusion, dim3(1), dim3(kThreads), 0, s, pred, y, B, C, counts, accumulate, status);
  BGCN_CHECK_LAUNCH();
  return BGCN_OK;
}

}  // namespace bgcn

extern "C" int bgcn_confusion(const int64_t* pred, const int64_t* y, int64_t B, int num_classes, int32_t* counts,
                              int accumulate, int32_t* status, bgcn_stream_t stream) {
  return bgcn::confusion_impl(pred, y, B, num_classes, counts, accumulate, status,
                              reinterpret_cast<hipStream_t>(stream));
}
