// EBGCN in TRAINING mode: bn1 (batch statistics) + relu + conv2's lin over the [64 + F] concat
// (model/Twitter/EBGCN.py:72-84) and their backward, without the dense [N, 64 + F] concat.
//
// The concat row of node i is c_i = [h1_i | x[rootindex[batch_i]]]: its F root columns hold only
// B distinct rows.  With n_b the node count of tree b and N the valid node count:
//   h columns: mean / biased variance over the N rows of h1
//   x columns: mean_x = (1/N) sum_b n_b x[r_b],  var_x = (1/N) sum_b n_b (x[r_b] - mean_x)^2
//   g = gamma / sqrt(var + eps), t = beta - mean g                       (the fold)
//   z2_i = relu(g_h h1_i + t_h) W2[:, :64]^T + r[batch_i],  r[b] = relu(g_x x[r_b] + t_x) W2[:, 64:]^T
// which is conv2_lin_impl on the folded batch statistics.  Backward, with dR[b] = sum_{i in b} dz2_i,
// a_h = relu(y_h), a_x[b] = relu(y_x[b]):
//   dW2[:, :64] = dz2^T a_h                 dW2[:, 64:] = dR^T a_x        (B rows, not N)
//   dY_h = (dz2 W2[:, :64]) . [y_h > 0]     dY_x[b] = (dR[b] W2[:, 64:]) . [y_x[b] > 0]
//   dbeta = column sums of dY (N rows / B rows), dgamma = sums of dY . chat, chat = (c - mean) rstd
//   dh1_i = g_h . (dY_h,i - dbeta_h / N - chat_h,i . dgamma_h / N)
// Nothing of size N x F is read or written: the largest arrays are [B, F] and [N, 64].
//
// Reductions: every float sum has a fixed order - block partials in the workspace (256 rows of h1,
// 32 trees of the root table per block; inside a block 16 / 4 row lanes that are combined in lane
// order), then one ordered pass.  Variances are of centred values: each block centres on its own
// mean and the ordered pass merges (n, mean, M2) triples (Chan et al.).  The only atomics are on
// integers (tree sizes, status bits).  The batch vector need not be sorted: when it is, dR's block
// of tree b finds its node range by bisection, else it picks its nodes out of the whole vector in
// node order.
//
// A node is valid when its tree id is in [0, B) and that tree's rootindex in [0, N); a tree with a
// bad rootindex has its size set to 0, so "tree_count[batch_i] > 0" is the validity test everywhere.
#include "bgcn_internal.h"

namespace bgcn {

int conv2_lin_impl(const float* h1, int64_t ldh, const float* x, int64_t ldx, const int64_t* batch,
                   const int64_t* rootindex, int64_t N, int64_t B, int64_t F, int64_t hid, const float* w2,
                   const float* g, const float* t, float* z2, int64_t ldz, int32_t* status, void* ws, size_t ws_bytes,
                   hipStream_t s);
int gemm_xw_impl(const float* X, int64_t ldx, const float* W, int64_t ldw, float* Y, int64_t ldy, int64_t M,
                 int64_t Nc, int64_t K, hipStream_t stream);

namespace {

constexpr int kH = 64;           // hidden size
constexpr int kRows = 256;       // rows of h1 per block of the N-row reductions
constexpr int kRowLanes = 16;    // ... as 16 row lanes x 16 float4 column groups
constexpr int kTrees = 32;       // trees per block of the root-table reductions
constexpr int kTreeLanes = 4;    // ... as 4 tree lanes (one wave each) x 64 float4 column groups

__device__ __forceinline__ float4 f4sub(float4 a, float4 b) {
  return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w);
}
__device__ __forceinline__ float4 f4scale(float a, float4 x) { return make_float4(a * x.x, a * x.y, a * x.z, a * x.w); }
// a true division: a column of equal values keeps its value as its mean (n v / n)
__device__ __forceinline__ float4 f4div(float4 x, float a) { return make_float4(x.x / a, x.y / a, x.z / a, x.w / a); }
__device__ __forceinline__ float4 f4rstd(float4 var, float eps) {
  return make_float4(1.0f / sqrtf(var.x + eps), 1.0f / sqrtf(var.y + eps), 1.0f / sqrtf(var.z + eps),
                     1.0f / sqrtf(var.w + eps));
}
// v where m > 0, else 0
__device__ __forceinline__ float4 f4mask(float4 m, float4 v) {
  return make_float4(m.x > 0.f ? v.x : 0.f, m.y > 0.f ? v.y : 0.f, m.z > 0.f ? v.z : 0.f, m.w > 0.f ? v.w : 0.f);
}
// the tree of node i, or -1 for an invalid node (never read through)
__device__ __forceinline__ int64_t valid_tree(const int64_t* __restrict__ batch, const int32_t* __restrict__ cnt,
                                              int64_t i, int64_t B) {
  const int64_t b = batch[i];
  return (b >= 0 && b < B && cnt[b] > 0) ? b : -1;
}
// sum of the lanes' float4 partials sm[lane][col] in lane order
template <int LANES, int COLS>
__device__ __forceinline__ float4 lane_sum(const float4 (*sm)[COLS], int col) {
  float4 s = sm[0][col];
#pragma unroll
  for (int r = 1; r < LANES; ++r) s = f4add(s, sm[r][col]);
  return s;
}

// ------------------------------------------------------------------ tree sizes
__global__ __launch_bounds__(256) void k_tree_count(const int64_t* __restrict__ batch, int64_t N, int64_t B,
                                                    int32_t* __restrict__ cnt, int32_t* __restrict__ status) {
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (i >= N) return;
  const int64_t b = batch[i];
  if (b < 0 || b >= B)
    atomicOr(status, 1);
  else
    atomicAdd(&cnt[b], 1);
}

// one block: a tree whose rootindex is outside [0, N) loses its nodes (size 0, status bit 0);
// num_valid = the nodes that are left
__global__ __launch_bounds__(256) void k_tree_finalize(const int64_t* __restrict__ rootindex, int64_t N, int64_t B,
                                                       int32_t* __restrict__ cnt, int32_t* __restrict__ num_valid,
                                                       int32_t* __restrict__ status) {
  __shared__ int32_t red[256];
  const int t = threadIdx.x;
  int32_t s = 0;
  bool bad = false;
  for (int64_t b = t; b < B; b += 256) {
    const int64_t r = rootindex[b];
    int32_t c = cnt[b];
    if (r < 0 || r >= N) {
      bad |= c > 0;
      cnt[b] = 0;
      c = 0;
    }
    s += c;
  }
  if (bad) atomicOr(status, 1);
  red[t] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  if (t == 0) *num_valid = red[0];
}

// ------------------------------------------------------------------ batch statistics
// Block p: (n, mean, M2) of its kRows rows of h1, per column; invalid rows are left out.
__global__ __launch_bounds__(256) void k_stat_h(const float* __restrict__ h1, int64_t ldh,
                                                const int64_t* __restrict__ batch, const int32_t* __restrict__ cnt,
                                                int64_t N, int64_t B, int32_t* __restrict__ pn,
                                                float* __restrict__ pmean, float* __restrict__ pm2) {
  __shared__ float4 sm[kRowLanes][16];
  __shared__ int32_t sn[kRowLanes];
  const int q = threadIdx.x & 15, r = threadIdx.x >> 4;
  const int64_t i0 = int64_t(blockIdx.x) * kRows + r;
  float4 v[kRows / kRowLanes];
  int32_t n = 0;
  float4 acc = f4zero();
#pragma unroll
  for (int j = 0; j < kRows / kRowLanes; ++j) {
    const int64_t i = i0 + kRowLanes * j;
    const bool ok = i < N && valid_tree(batch, cnt, i, B) >= 0;
    v[j] = ok ? ld4(h1 + i * ldh + 4 * q) : f4zero();
    n += ok ? 1 : 0;
    acc = f4add(acc, v[j]);
  }
  sm[r][q] = acc;
  if (q == 0) sn[r] = n;
  __syncthreads();
  int32_t nb = 0;
#pragma unroll
  for (int k = 0; k < kRowLanes; ++k) nb += sn[k];
  const float4 mean = nb > 0 ? f4div(lane_sum<kRowLanes, 16>(sm, q), float(nb)) : f4zero();
  __syncthreads();
  float4 m2 = f4zero();
#pragma unroll
  for (int j = 0; j < kRows / kRowLanes; ++j) {
    const int64_t i = i0 + kRowLanes * j;
    const bool ok = i < N && valid_tree(batch, cnt, i, B) >= 0;
    if (ok) {
      const float4 d = f4sub(v[j], mean);
      m2 = f4add(m2, f4mul(d, d));
    }
  }
  sm[r][q] = m2;
  __syncthreads();
  if (r == 0) {
    st4(pmean + int64_t(blockIdx.x) * kH + 4 * q, mean);
    st4(pm2 + int64_t(blockIdx.x) * kH + 4 * q, lane_sum<kRowLanes, 16>(sm, q));
    if (q == 0) pn[blockIdx.x] = nb;
  }
}

// Block (column group, chunk p): (n, mean, M2) of the chunk's kTrees root rows weighted by tree size.
// A wave is one tree lane: the tree's size and root are wave-uniform, the rows stream as float4 columns.
__global__ __launch_bounds__(256) void k_stat_x(const float* __restrict__ x, int64_t ldx,
                                                const int64_t* __restrict__ rootindex,
                                                const int32_t* __restrict__ cnt, int64_t B, int64_t F4,
                                                int32_t* __restrict__ pn, float* __restrict__ pmean,
                                                float* __restrict__ pm2) {
  __shared__ float4 sm[kTreeLanes][64];
  __shared__ int32_t sn[kTreeLanes];
  const int cq = threadIdx.x & 63, r = threadIdx.x >> 6;
  const int64_t q = int64_t(blockIdx.x) * 64 + cq;
  const bool col = q < F4;
  const int64_t b0 = int64_t(blockIdx.y) * kTrees + r;
  float4 v[kTrees / kTreeLanes];
  float w[kTrees / kTreeLanes];
  int32_t n = 0;
  float4 acc = f4zero();
#pragma unroll
  for (int j = 0; j < kTrees / kTreeLanes; ++j) {
    const int64_t b = b0 + kTreeLanes * j;
    const int32_t c = b < B ? cnt[b] : 0;
    w[j] = float(c);
    v[j] = (c > 0 && col) ? ld4(x + rootindex[b] * ldx + 4 * q) : f4zero();
    n += c;
    acc = f4fma(w[j], v[j], acc);
  }
  sm[r][cq] = acc;
  if (cq == 0) sn[r] = n;
  __syncthreads();
  int32_t nb = 0;
#pragma unroll
  for (int k = 0; k < kTreeLanes; ++k) nb += sn[k];
  const float4 mean = nb > 0 ? f4div(lane_sum<kTreeLanes, 64>(sm, cq), float(nb)) : f4zero();
  __syncthreads();
  float4 m2 = f4zero();
#pragma unroll
  for (int j = 0; j < kTrees / kTreeLanes; ++j) {
    const float4 d = f4sub(v[j], mean);
    m2 = f4fma(w[j], f4mul(d, d), m2);   // w = 0 for a tree that is left out
  }
  sm[r][cq] = m2;
  __syncthreads();
  if (r == 0) {
    const int64_t F = 4 * F4;
    if (col) {
      st4(pmean + int64_t(blockIdx.y) * F + 4 * q, mean);
      st4(pm2 + int64_t(blockIdx.y) * F + 4 * q, lane_sum<kTreeLanes, 64>(sm, cq));
    }
    if (blockIdx.x == 0 && cq == 0) pn[blockIdx.y] = nb;
  }
}

// One thread per column of the concat: the ordered merge of the partial (n, mean, M2) triples, then
// the fold (bn_fold, as in eval mode).  Fewer than two valid nodes: no statistics, everything 0.
__global__ __launch_bounds__(256) void k_stats_fold(const int32_t* __restrict__ hn, const float* __restrict__ hmean,
                                                    const float* __restrict__ hm2, int Ph,
                                                    const int32_t* __restrict__ xn, const float* __restrict__ xmean,
                                                    const float* __restrict__ xm2, int Px, int64_t F,
                                                    const float* __restrict__ gamma, const float* __restrict__ beta,
                                                    float eps, const int32_t* __restrict__ num_valid,
                                                    float* __restrict__ mean_out, float* __restrict__ var_out,
                                                    float* __restrict__ g, float* __restrict__ t) {
  const int64_t c = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (c >= kH + F) return;
  const bool hs = c < kH;
  const int32_t* pn = hs ? hn : xn;
  const float* pm = hs ? hmean + c : xmean + (c - kH);
  const float* p2 = hs ? hm2 + c : xm2 + (c - kH);
  const int64_t ld = hs ? kH : F;
  const int P = hs ? Ph : Px;
  float n = 0.f, mean = 0.f, m2 = 0.f;
  for (int p = 0; p < P; ++p) {
    const int32_t nbi = pn[p];
    if (nbi == 0) continue;
    const float nb = float(nbi), mb = pm[int64_t(p) * ld], m2b = p2[int64_t(p) * ld];
    if (n == 0.f) {
      n = nb;
      mean = mb;
      m2 = m2b;
    } else {
      const float nn = n + nb, d = mb - mean;
      mean = fmaf(d, nb / nn, mean);
      m2 = m2 + m2b + d * d * (n * nb / nn);
      n = nn;
    }
  }
  float var = n > 0.f ? m2 / n : 0.f, gg = 0.f, tt = 0.f;
  if (*num_valid >= 2) {
    bn_fold(gamma[c], beta[c], mean, var, eps, gg, tt);
  } else {
    mean = 0.f;
    var = 0.f;
  }
  mean_out[c] = mean;
  var_out[c] = var;
  g[c] = gg;
  t[c] = tt;
}

// a_x[b] = relu(g_x x[r_b] + t_x) (f4affine, as k_affine_relu_rows: the forward's own root table has
// these bits); zeros for a tree without valid nodes
__global__ __launch_bounds__(256) void k_root_act(const float* __restrict__ x, int64_t ldx,
                                                  const int64_t* __restrict__ rootindex,
                                                  const int32_t* __restrict__ cnt, int64_t B, int64_t F4,
                                                  const float* __restrict__ g, const float* __restrict__ t,
                                                  float* __restrict__ ax) {
  const int64_t idx = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (idx >= B * F4) return;
  const int64_t b = idx / F4, q = idx - b * F4;
  float4 v = f4zero();
  if (cnt[b] > 0) v = f4relu(f4affine(ld4(g + 4 * q), ld4(x + rootindex[b] * ldx + 4 * q), ld4(t + 4 * q)));
  st4(ax + idx * 4, v);
}

// rows[i][:64] = 0 for an invalid node (every node when fewer than two are valid)
__global__ __launch_bounds__(256) void k_zero_invalid(float* __restrict__ rows, int64_t ld,
                                                      const int64_t* __restrict__ batch,
                                                      const int32_t* __restrict__ cnt, int64_t N, int64_t B,
                                                      const int32_t* __restrict__ num_valid) {
  const int64_t idx = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (idx >= N * (kH / 4)) return;
  const int64_t i = idx >> 4;
  if (*num_valid >= 2 && valid_tree(batch, cnt, i, B) >= 0) return;
  st4(rows + i * ld + 4 * int(idx & 15), f4zero());
}

// ------------------------------------------------------------------ backward
// a_h[i] = relu(g_h h1_i + t_h), zeros for an invalid node; *unsorted |= 1 when batch decreases
__global__ __launch_bounds__(256) void k_act_h(const float* __restrict__ h1, int64_t ldh,
                                               const int64_t* __restrict__ batch, const int32_t* __restrict__ cnt,
                                               int64_t N, int64_t B, const float* __restrict__ g,
                                               const float* __restrict__ t, float* __restrict__ act,
                                               int32_t* __restrict__ unsorted) {
  const int64_t idx = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (idx >= N * (kH / 4)) return;
  const int64_t i = idx >> 4;
  const int q = int(idx & 15);
  if (q == 0 && i > 0 && batch[i] < batch[i - 1]) atomicOr(unsorted, 1);
  float4 v = f4zero();
  if (valid_tree(batch, cnt, i, B) >= 0) v = f4relu(f4affine(ld4(g + 4 * q), ld4(h1 + i * ldh + 4 * q), ld4(t + 4 * q)));
  st4(act + i * kH + 4 * q, v);
}

// dR[b] = sum of dz2 over tree b's valid nodes, one block per tree: row lane r takes the rows
// lo + r, lo + r + 16, ... of the range [lo, hi) in order (a sorted batch vector: the tree's own
// range, found by bisection; else the whole vector), the 16 lanes are combined in lane order
__global__ __launch_bounds__(256) void k_tree_sum(const float* __restrict__ dz, int64_t ldd,
                                                  const int64_t* __restrict__ batch, const int32_t* __restrict__ cnt,
                                                  int64_t N, const int32_t* __restrict__ unsorted,
                                                  float* __restrict__ dR) {
  __shared__ float4 sm[kRowLanes][16];
  const int q = threadIdx.x & 15, r = threadIdx.x >> 4;
  const int64_t b = blockIdx.x;
  if (cnt[b] == 0) {   // block-uniform
    if (r == 0) st4(dR + b * kH + 4 * q, f4zero());
    return;
  }
  int64_t lo = 0, hi = N;
  if (*unsorted == 0) {
    int64_t a = 0, e = N;   // first i with batch[i] >= b
    while (a < e) {
      const int64_t m = (a + e) >> 1;
      if (batch[m] < b) a = m + 1; else e = m;
    }
    lo = a;
    e = N;                  // first i with batch[i] > b
    while (a < e) {
      const int64_t m = (a + e) >> 1;
      if (batch[m] <= b) a = m + 1; else e = m;
    }
    hi = a;
  }
  float4 acc = f4zero();
  for (int64_t i = lo + r; i < hi; i += kRowLanes)
    if (batch[i] == b) acc = f4add(acc, ld4(dz + i * ldd + 4 * q));
  sm[r][q] = acc;
  __syncthreads();
  if (r == 0) st4(dR + b * kH + 4 * q, lane_sum<kRowLanes, 16>(sm, q));
}

// h side of bn1's backward, block p over its kRows rows: G (= dz2 W2[:, :64], in gy) becomes
// dY = G . [y > 0] in place (zeros for an invalid node); part[p][0] = sum dY, part[p][1] = sum dY . chat
__global__ __launch_bounds__(256) void k_bn_bwd_h(const float* __restrict__ h1, int64_t ldh,
                                                  const int64_t* __restrict__ batch,
                                                  const int32_t* __restrict__ cnt, int64_t N, int64_t B,
                                                  const float* __restrict__ g, const float* __restrict__ t,
                                                  const float* __restrict__ mean, const float* __restrict__ var,
                                                  float eps, float* __restrict__ gy, float* __restrict__ part) {
  __shared__ float4 sb[kRowLanes][16];
  __shared__ float4 sg[kRowLanes][16];
  const int q = threadIdx.x & 15, r = threadIdx.x >> 4;
  const float4 gg = ld4(g + 4 * q), tt = ld4(t + 4 * q), mu = ld4(mean + 4 * q);
  const float4 rs = f4rstd(ld4(var + 4 * q), eps);
  float4 db = f4zero(), dg = f4zero();
  for (int j = 0; j < kRows / kRowLanes; ++j) {
    const int64_t i = int64_t(blockIdx.x) * kRows + r + kRowLanes * j;
    if (i >= N) break;
    float4 dy = f4zero();
    if (valid_tree(batch, cnt, i, B) >= 0) {
      const float4 h = ld4(h1 + i * ldh + 4 * q);
      dy = f4mask(f4affine(gg, h, tt), ld4(gy + i * kH + 4 * q));
      db = f4add(db, dy);
      dg = f4add(dg, f4mul(dy, f4mul(f4sub(h, mu), rs)));
    }
    st4(gy + i * kH + 4 * q, dy);
  }
  sb[r][q] = db;
  sg[r][q] = dg;
  __syncthreads();
  if (r == 0) {
    st4(part + int64_t(blockIdx.x) * 2 * kH + 4 * q, lane_sum<kRowLanes, 16>(sb, q));
    st4(part + int64_t(blockIdx.x) * 2 * kH + kH + 4 * q, lane_sum<kRowLanes, 16>(sg, q));
  }
}

// x side, block (column group, chunk p) over its kTrees trees: dY_x[b] = G_x[b] . [a_x[b] > 0]
// (G_x = dR W2[:, 64:]; a_x > 0 exactly where y_x > 0), part[p][0] = sum dY_x, part[p][1] = sum dY_x . chat_x
__global__ __launch_bounds__(256) void k_bn_bwd_x(const float* __restrict__ x, int64_t ldx,
                                                  const int64_t* __restrict__ rootindex,
                                                  const int32_t* __restrict__ cnt, int64_t B, int64_t F4,
                                                  const float* __restrict__ ax, const float* __restrict__ gx,
                                                  const float* __restrict__ mean, const float* __restrict__ var,
                                                  float eps, float* __restrict__ part) {
  __shared__ float4 sb[kTreeLanes][64];
  __shared__ float4 sg[kTreeLanes][64];
  const int cq = threadIdx.x & 63, r = threadIdx.x >> 6;
  const int64_t q = int64_t(blockIdx.x) * 64 + cq, F = 4 * F4;
  const bool col = q < F4;
  float4 db = f4zero(), dg = f4zero();
  if (col) {
    const float4 mu = ld4(mean + 4 * q), rs = f4rstd(ld4(var + 4 * q), eps);
#pragma unroll
    for (int j = 0; j < kTrees / kTreeLanes; ++j) {
      const int64_t b = int64_t(blockIdx.y) * kTrees + r + kTreeLanes * j;
      if (b < B && cnt[b] > 0) {
        const float4 dy = f4mask(ld4(ax + b * F + 4 * q), ld4(gx + b * F + 4 * q));
        db = f4add(db, dy);
        dg = f4add(dg, f4mul(dy, f4mul(f4sub(ld4(x + rootindex[b] * ldx + 4 * q), mu), rs)));
      }
    }
  }
  sb[r][cq] = db;
  sg[r][cq] = dg;
  __syncthreads();
  if (r == 0 && col) {
    st4(part + int64_t(blockIdx.y) * 2 * F + 4 * q, lane_sum<kTreeLanes, 64>(sb, cq));
    st4(part + int64_t(blockIdx.y) * 2 * F + F + 4 * q, lane_sum<kTreeLanes, 64>(sg, cq));
  }
}

// dbeta[c] / dgamma[c] = the partials of column c summed in block order
__global__ __launch_bounds__(256) void k_bn_bwd_final(const float* __restrict__ part_h, int Ph,
                                                      const float* __restrict__ part_x, int Px, int64_t F,
                                                      float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int64_t c = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (c >= kH + F) return;
  const bool hs = c < kH;
  const int64_t ld = hs ? kH : F;
  const float* p = hs ? part_h + c : part_x + (c - kH);
  const int P = hs ? Ph : Px;
  float db = 0.f, dg = 0.f;
  for (int k = 0; k < P; ++k) {
    db += p[int64_t(k) * 2 * ld];
    dg += p[int64_t(k) * 2 * ld + ld];
  }
  dbeta[c] = db;
  dgamma[c] = dg;
}

// dh1_i = g_h . (dY_i - dbeta_h / N - chat_i . dgamma_h / N); zeros for an invalid node
__global__ __launch_bounds__(256) void k_dh1(const float* __restrict__ h1, int64_t ldh,
                                             const int64_t* __restrict__ batch, const int32_t* __restrict__ cnt,
                                             int64_t N, int64_t B, const float* __restrict__ g,
                                             const float* __restrict__ mean, const float* __restrict__ var, float eps,
                                             const float* __restrict__ dy, const float* __restrict__ dgamma,
                                             const float* __restrict__ dbeta, const int32_t* __restrict__ num_valid,
                                             float* __restrict__ dh1, int64_t ldd) {
  const int64_t idx = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (idx >= N * (kH / 4)) return;
  const int64_t i = idx >> 4;
  const int q = int(idx & 15);
  const int32_t nv = *num_valid;
  float4 out = f4zero();
  if (nv >= 2 && valid_tree(batch, cnt, i, B) >= 0) {
    const float inv = 1.0f / float(nv);
    const float4 ch = f4mul(f4sub(ld4(h1 + i * ldh + 4 * q), ld4(mean + 4 * q)), f4rstd(ld4(var + 4 * q), eps));
    const float4 d = f4sub(f4sub(ld4(dy + i * kH + 4 * q), f4scale(inv, ld4(dbeta + 4 * q))),
                           f4mul(ch, f4scale(inv, ld4(dgamma + 4 * q))));
    out = f4mul(ld4(g + 4 * q), d);
  }
  st4(dh1 + i * ldd + 4 * q, out);
}

struct Bn1TrainWs {
  void* conv2;        // conv2_lin_impl's workspace
  size_t conv2_bytes;
  int32_t *hn, *xn;   // [Ph], [Px] valid rows / nodes per block
  float *hmean, *hm2; // [Ph, 64]
  float *xmean, *xm2; // [Px, F]
  float* act;         // [N, 64] a_h
  float* gy;          // [N, 64] dz2 W2[:, :64], then dY_h
  float* dR;          // [B, 64]
  float* gx;          // [B, F]  dR W2[:, 64:]
  float* part_h;      // [Ph, 2, 64]
  float* part_x;      // [Px, 2, F]
  int32_t* unsorted;  // [1]
  void* tn;           // gemm_tn_impl's split partials
  size_t tn_bytes;
};
int64_t blocks_h(int64_t N) { return (N + kRows - 1) / kRows; }
int64_t blocks_x(int64_t B) { return (B + kTrees - 1) / kTrees; }
size_t carve_bn1_train(Carve& c, int64_t N, int64_t B, int64_t F, Bn1TrainWs* w) {
  const size_t Ph = size_t(blocks_h(N)), Px = size_t(blocks_x(B));
  w->conv2_bytes = bgcn_ebgcn_conv2_lin_workspace_size(N, B, F);
  w->conv2 = c.take<char>(w->conv2_bytes);
  w->hn = c.take<int32_t>(Ph);
  w->xn = c.take<int32_t>(Px);
  w->hmean = c.take<float>(Ph * kH);
  w->hm2 = c.take<float>(Ph * kH);
  w->xmean = c.take<float>(Px * size_t(F));
  w->xm2 = c.take<float>(Px * size_t(F));
  w->act = c.take<float>(size_t(N) * kH);
  w->gy = c.take<float>(size_t(N) * kH);
  w->dR = c.take<float>(size_t(B) * kH);
  w->gx = c.take<float>(size_t(B) * size_t(F));
  w->part_h = c.take<float>(Ph * 2 * kH);
  w->part_x = c.take<float>(Px * 2 * size_t(F));
  w->unsorted = c.take<int32_t>(1);
  w->tn_bytes = std::max(tn_ws_size(kH, kH, N), tn_ws_size(kH, F, B));
  w->tn = c.take<char>(w->tn_bytes);
  return align_up(c.off, 256);
}

int check_shape(int64_t N, int64_t B, int64_t F, int64_t hid, int64_t ldh, int64_t ldx) {
  BGCN_CHECK_ARG(hid == kH, "conv2_lin_train: the hidden size must be 64");
  BGCN_CHECK_ARG(F > 0 && F % 4 == 0, "conv2_lin_train: in_feats must be a positive multiple of 4");
  BGCN_CHECK_ARG(N > 0 && B > 0, "conv2_lin_train: need N > 0 and B > 0");
  BGCN_CHECK_ARG(N < (int64_t(1) << 31) && B <= (int64_t(1) << 20) && B * (F / 4) < (int64_t(1) << 38),
                 "conv2_lin_train: batch too large");
  BGCN_CHECK_ARG(ldh >= kH && ldh % 4 == 0 && ldx >= F && ldx % 4 == 0,
                 "conv2_lin_train: leading dimensions must be multiples of 4 and cover the rows");
  return BGCN_OK;
}

}  // namespace

int conv2_lin_train_fwd_impl(const bgcn_conv2_lin_train_fwd_args* a, void* ws, size_t ws_bytes, hipStream_t s) {
  BGCN_CHECK_ARG(a, "conv2_lin_train: null argument struct");
  const int64_t N = a->num_nodes, B = a->num_graphs, F = a->in_feats;
  BGCN_TRY(check_shape(N, B, F, a->hid, a->ldh, a->ldx));
  BGCN_CHECK_ARG(a->ldz >= kH && a->ldz % 4 == 0,
                 "conv2_lin_train: leading dimensions must be multiples of 4 and cover the rows");
  BGCN_CHECK_ARG(a->eps >= 0.f, "conv2_lin_train: eps must not be negative");
  BGCN_CHECK_ARG(a->h1 && a->x && a->batch && a->rootindex && a->w2 && a->gamma && a->beta && a->z2 &&
                     a->batch_mean && a->batch_var && a->bn_g && a->bn_t && a->a_x && a->tree_count &&
                     a->num_valid && a->status,
                 "conv2_lin_train: null pointer");
  BGCN_CHECK_ARG(a16(a->h1) && a16(a->x) && a16(a->w2) && a16(a->z2) && a16(a->bn_g) && a16(a->bn_t) && a16(a->a_x),
                 "conv2_lin_train: pointers must be 16-byte aligned");
  Bn1TrainWs w;
  Carve c(ws, ws_bytes);
  carve_bn1_train(c, N, B, F, &w);
  BGCN_CHECK_ARG(ws && c.ok(), "conv2_lin_train: workspace too small");
  const int Ph = int(blocks_h(N)), Px = int(blocks_x(B));
  const int64_t F4 = F / 4;
  BGCN_CHECK_HIP(hipMemsetAsync(a->tree_count, 0, size_t(B) * sizeof(int32_t), s));
  hipLaunchKernelGGL(k_tree_count, dim3(grid_for(N, 256)), dim3(256), 0, s, a->batch, N, B, a->tree_count, a->status);
  BGCN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_tree_finalize, dim3(1), dim3(256), 0, s, a->rootindex, N, B, a->tree_count, a->num_valid,
                     a->status);
  BGCN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_stat_h, dim3(Ph), dim3(256), 0, s, a->h1, a->ldh, a->batch, a->tree_count, N, B, w.hn, w.hmean,
                     w.hm2);
  BGCN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_stat_x, dim3(grid_for(F4, 64), Px), dim3(256), 0, s, a->x, a->ldx, a->rootindex, a->tree_count,
                     B, F4, w.xn, w.xmean, w.xm2);
  BGCN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_stats_fold, dim3(grid_for(kH + F, 256)), dim3(256), 0, s, w.hn, w.hmean, w.hm2, Ph, w.xn,
                     w.xmean, w.xm2, Px, F, a->gamma, a->beta, a->eps, a->num_valid, a->batch_mean, a->batch_var,
                     a->bn_g, a->bn_t);
  BGCN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_root_act, dim3(grid_for(B * F4, 256)), dim3(256), 0, s, a->x, a->ldx, a->rootindex,
                     a->tree_count, B, F4, a->bn_g + kH, a->bn_t + kH, a->a_x);
  BGCN_CHECK_LAUNCH();
  BGCN_TRY(conv2_lin_impl(a->h1, a->ldh, a->x, a->ldx, a->batch, a->rootindex, N, B, F, kH, a->w2, a->bn_g, a->bn_t,
                          a->z2, a->ldz, a->status, w.conv2, w.conv2_bytes, s));
  hipLaunchKernelGGL(k_zero_invalid, dim3(grid_for(N * (kH / 4), 256)), dim3(256), 0, s, a->z2, a->ldz, a->batch,
                     a->tree_count, N, B, a->num_valid);
  BGCN_CHECK_LAUNCH();
  return BGCN_OK;
}

int conv2_lin_train_bwd_impl(const bgcn_conv2_lin_train_bwd_args* a, void* ws, size_t ws_bytes, hipStream_t s) {
  BGCN_CHECK_ARG(a, "conv2_lin_train: null argument struct");
  const int64_t N = a->num_nodes, B = a->num_graphs, F = a->in_feats;
  BGCN_TRY(check_shape(N, B, F, a->hid, a->ldh, a->ldx));
  BGCN_CHECK_ARG(a->lddz >= kH && a->lddz % 4 == 0 && a->ldd >= kH && a->ldd % 4 == 0,
                 "conv2_lin_train: leading dimensions must be multiples of 4 and cover the rows");
  BGCN_CHECK_ARG(a->eps >= 0.f, "conv2_lin_train: eps must not be negative");
  BGCN_CHECK_ARG(a->dz2 && a->h1 && a->x && a->batch && a->rootindex && a->w2 && a->batch_mean && a->batch_var &&
                     a->bn_g && a->bn_t && a->a_x && a->tree_count && a->num_valid && a->dh1 && a->dw2 &&
                     a->dgamma && a->dbeta,
                 "conv2_lin_train: null pointer");
  BGCN_CHECK_ARG(a16(a->dz2) && a16(a->h1) && a16(a->x) && a16(a->w2) && a16(a->batch_mean) && a16(a->batch_var) &&
                     a16(a->bn_g) && a16(a->bn_t) && a16(a->a_x) && a16(a->dh1) && a16(a->dw2) && a16(a->dgamma) &&
                     a16(a->dbeta),
                 "conv2_lin_train: pointers must be 16-byte aligned");
  Bn1TrainWs w;
  Carve c(ws, ws_bytes);
  carve_bn1_train(c, N, B, F, &w);
  BGCN_CHECK_ARG(ws && c.ok(), "conv2_lin_train: workspace too small");
  const int Ph = int(blocks_h(N)), Px = int(blocks_x(B));
  const int64_t F4 = F / 4, ldw = kH + F;
  const unsigned rows16 = grid_for(N * (kH / 4), 256);
  BGCN_CHECK_HIP(hipMemsetAsync(w.unsorted, 0, sizeof(int32_t), s));
  hipLaunchKernelGGL(k_act_h, dim3(rows16), dim3(256), 0, s, a->h1, a->ldh, a->batch, a->tree_count, N, B, a->bn_g,
                     a->bn_t, w.act, w.unsorted);
  BGCN_CHECK_LAUNCH();
  // dW2[:, :64] = dz2^T a_h (an invalid node's a_h row is zero)
  BGCN_TRY(gemm_tn_impl(a->dz2, a->lddz, w.act, kH, a->dw2, nullptr, ldw, kH, kH, kH, N, w.tn, w.tn_bytes, s, -1,
                        nullptr));
  hipLaunchKernelGGL(k_tree_sum, dim3(unsigned(B)), dim3(256), 0, s, a->dz2, a->lddz, a->batch, a->tree_count, N,
                     w.unsorted, w.dR);
  BGCN_CHECK_LAUNCH();
  // dW2[:, 64:] = dR^T a_x: B rows
  BGCN_TRY(gemm_tn_impl(w.dR, kH, a->a_x, F, a->dw2 + kH, nullptr, ldw, kH, kH, F, B, w.tn, w.tn_bytes, s, -1,
                        nullptr));
  BGCN_TRY(gemm_xw_impl(a->dz2, a->lddz, a->w2, ldw, w.gy, kH, N, kH, kH, s));
  BGCN_TRY(gemm_xw_impl(w.dR, kH, a->w2 + kH, ldw, w.gx, F, B, F, kH, s));
  hipLaunchKernelGGL(k_bn_bwd_h, dim3(Ph), dim3(256), 0, s, a->h1, a->ldh, a->batch, a->tree_count, N, B, a->bn_g,
                     a->bn_t, a->batch_mean, a->batch_var, a->eps, w.gy, w.part_h);
  BGCN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_bn_bwd_x, dim3(grid_for(F4, 64), Px), dim3(256), 0, s, a->x, a->ldx, a->rootindex,
                     a->tree_count, B, F4, a->a_x, w.gx, a->batch_mean + kH, a->batch_var + kH, a->eps, w.part_x);
  BGCN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_bn_bwd_final, dim3(grid_for(kH + F, 256)), dim3(256), 0, s, w.part_h, Ph, w.part_x, Px, F,
                     a->dgamma, a->dbeta);
  BGCN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_dh1, dim3(rows16), dim3(256), 0, s, a->h1, a->ldh, a->batch, a->tree_count, N, B, a->bn_g,
                     a->batch_mean, a->batch_var, a->eps, w.gy, a->dgamma, a->dbeta, a->num_valid, a->dh1, a->ldd);
  BGCN_CHECK_LAUNCH();
  return BGCN_OK;
}

}  // namespace bgcn

extern "C" size_t bgcn_ebgcn_conv2_lin_train_workspace_size(int64_t num_nodes, int64_t num_graphs, int64_t in_feats) {
  if (num_nodes <= 0 || num_graphs <= 0 || in_feats <= 0) return 0;
  bgcn::Bn1TrainWs w;
  bgcn::Carve c(nullptr, 0);
  return bgcn::carve_bn1_train(c, num_nodes, num_graphs, in_feats, &w);
}

extern "C" int bgcn_ebgcn_conv2_lin_train_fwd(const bgcn_conv2_lin_train_fwd_args* args, void* workspace,
                                              size_t workspace_bytes, bgcn_stream_t stream) {
  return bgcn::conv2_lin_train_fwd_impl(args, workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int bgcn_ebgcn_conv2_lin_train_bwd(const bgcn_conv2_lin_train_bwd_args* args, void* workspace,
                                              size_t workspace_bytes, bgcn_stream_t stream) {
  return bgcn::conv2_lin_train_bwd_impl(args, workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream));
}
