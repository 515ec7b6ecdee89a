// Many-tensor Adam: one launch for up to 128 tensors in up to 8 learning-rate groups.
//
// bgcn_adam_step (bgcn_optim.hip) carries its tensors by value in the kernel arguments, 16 at the
// most.  An EBGCN has 68 parameter tensors in five groups (EBGCN.py:249-260), sixty of them of
// 4096 elements or fewer.  Here what is fixed between steps - param, exp_avg, exp_avg_sq, numel,
// group, first workgroup - lives in a table in device memory that the caller uploads once, and
// what changes every step - the gradient pointers autograd hands out afresh, the groups' learning
// rates, the bias corrections, the skip flag - travels in the kernel arguments (about 1.1 KB), so
// a step makes no host-to-device copy.  The update is bgcn_internal.h's adam_chunk, the one
// k_adam's tensors without a weight image take.
#include "bgcn_common.h"
#include "bgcn_internal.h"

namespace bgcn {
namespace {

constexpr int kChunk = BGCN_ADAM_MULTI_CHUNK;   // elements per workgroup (256 threads x one float4)
static_assert(kChunk == 256 * 4, "one float4 per thread");

__global__ __launch_bounds__(256) void k_adam_multi(bgcn_adam_multi_args a) {
  if (a.skip_flag && *a.skip_flag != 0.0f) {   // invalid step: no update
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.skip_count) atomicAdd(a.skip_count, 1);
    return;
  }
  // the last tensor whose first workgroup is not after this one (uniform: scalar loads).  An
  // empty tensor shares its first_block with the next one and is never the last such.
  const int64_t b = blockIdx.x;
  int lo = 0, hi = a.count - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (a.table[mid].first_block <= b) lo = mid; else hi = mid - 1;
  }
  const float* __restrict__ grad = a.grad[lo];
  if (!grad) return;   // `grad is None`: parameter and moments untouched
  const bgcn_adam_multi_tensor T = a.table[lo];
  const AdamConst c{a.beta1, a.beta2, a.weight_decay, a.eps, a.lr[T.group] / a.bias_correction1,
                    1.0f / a.bias_correction2_sqrt, a.grad_scale};
  adam_chunk(T.param, grad, T.exp_avg, T.exp_avg_sq, T.numel, (b - T.first_block) * kChunk + threadIdx.x * 4, c);
}

bool count_ok(int count) { return count >= 1 && count <= BGCN_ADAM_MULTI_MAX_TENSORS; }

}  // namespace
}  // namespace bgcn

extern "C" size_t bgcn_adam_multi_table_size(int count) {
  return bgcn::count_ok(count) ? size_t(count) * sizeof(bgcn_adam_multi_tensor) : 0;
}

extern "C" int bgcn_adam_multi_plan(const bgcn_adam_multi_tensor* tensors, int count, void* table_host,
                                    size_t table_bytes, int64_t* blocks) {
  using namespace bgcn;
  BGCN_CHECK_ARG(count_ok(count), "adam_multi: 1..BGCN_ADAM_MULTI_MAX_TENSORS tensors");
  BGCN_CHECK_ARG(tensors && blocks, "adam_multi: null tensors / blocks");
  BGCN_CHECK_ARG(table_host, "adam_multi: null table");
  BGCN_CHECK_ARG(table_bytes >= bgcn_adam_multi_table_size(count), "adam_multi: table buffer too small");
  int64_t total = 0;
  for (int k = 0; k < count; ++k) {
    const bgcn_adam_multi_tensor& T = tensors[k];
    BGCN_CHECK_ARG(T.group >= 0 && T.group < BGCN_ADAM_MULTI_MAX_GROUPS, "adam_multi: group outside [0, 8)");
    BGCN_CHECK_ARG(T.numel >= 0, "adam_multi: numel < 0");
    BGCN_CHECK_ARG(T.numel == 0 || (T.param && T.exp_avg && T.exp_avg_sq),
                   "adam_multi: null param / exp_avg / exp_avg_sq");
    total += (T.numel + kChunk - 1) / kChunk;
    BGCN_CHECK_ARG(total <= int64_t(0x7fffffff), "adam_multi: too many elements for one launch");
  }
  bgcn_adam_multi_tensor* out = static_cast<bgcn_adam_multi_tensor*>(table_host);
  total = 0;
  for (int k = 0; k < count; ++k) {
    out[k] = tensors[k];
    out[k].first_block = total;
    out[k].reserved = 0;
    total += (tensors[k].numel + kChunk - 1) / kChunk;
  }
  *blocks = total;
  return BGCN_OK;
}

extern "C" int bgcn_adam_multi_step(const bgcn_adam_multi_args* args, bgcn_stream_t stream) {
  using namespace bgcn;
  BGCN_CHECK_ARG(args, "adam_multi: null args");
  BGCN_CHECK_ARG(count_ok(args->count), "adam_multi: 1..BGCN_ADAM_MULTI_MAX_TENSORS tensors");
  BGCN_CHECK_ARG(args->table, "adam_multi: null table");
  BGCN_CHECK_ARG(args->blocks >= 0 && args->blocks <= int64_t(0x7fffffff), "adam_multi: bad block count");
  if (args->blocks == 0) return BGCN_OK;
  hipLaunchKernelGGL(k_adam_multi, dim3(unsigned(args->blocks)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), *args);
  BGCN_CHECK_LAUNCH();
  return BGCN_OK;
}
