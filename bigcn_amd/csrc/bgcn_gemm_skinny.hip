// Skinny-M GEMMs on fp32 weights as the parameter tensors store them, for the weight-bound
// [B, hidden] chain of TreeBERT's training call (a few dozen rows against 2 - 9 MB of weights that
// change at every optimiser step: no image, no rounding).  bgcn_gemm_w16.hip is the template: the
// reduction is split over waves and workgroups until a 768 x 768 product is 288 workgroups, weight
// loads are issued first and kept in registers across the row tiles of a block, the four waves'
// accumulators are added through LDS in wave order, and the partials are added in slice order by
// k_w16_reduce (w16_reduce, which is fp32 in and out and is used as it is).
//
// Arithmetic: v_mfma_f32_32x32x2_f32, fp32 operands and accumulator - an fmaf chain per element, so
// integer operands give exact results and a row's bits depend on nothing but that row and W.  Lane
// (h, r) of a wave feeds A[r][h] and B[h][r]; which two reduction indices share one instruction is
// free as long as A and B agree, so every lane loads runs of consecutive elements.
//
//   xwt  Y[M, Nc] = X[M, K] . W[Nc, K]^T (+ bias).  Workgroup (nt, s, rb): columns [32 nt, 32 nt + 32),
//        k-slice s, rows [128 rb, 128 rb + 128).  Wave w takes the k-tiles (4 s + w) KW .. of 16; lane
//        (h, r) holds W[32 nt + r][16 kt + 8 h + j] and X[m0 + r][the same k], j < 8.
//        S = K / (64 KW) partials part[s][m][n].
//   xw   Y[M, K] = G[M, Nc] . W[Nc, K].  Workgroup (kt, s, rb): output columns [32 kt, 32 kt + 32),
//        slice s of the rows of W.  Wave w takes the 16 KW rows from 16 KW (4 s + w); lane (h, r) holds
//        W[n0 + 8 KW h + j][32 kt + r] (a wave load is two rows of 128 contiguous bytes) and
//        G[m0 + r][n0 + 8 KW h + j], j < 8 KW.  S = Nc / (64 KW) partials part[s][m][k].
//   tn   dW[Nc, K] = G[M, Nc]^T . X[M, K].  One wave per 32 x 64 tile of dW (288 workgroups at 768 x 768),
//        the rows of G and X taken two per instruction in ascending order, no split, no partials.
//
// The split (skinny_kw): KW the largest of 8, 4, 2 that divides the reduction's 64-blocks and still
// leaves (output width / 32) S >= 256 workgroups, else 1 - bgcn_gemm_w16.hip's rule, a function of
// the weight's shape alone.  No float atomics; rows past M are read as row M - 1 and not written.
#include "bgcn_internal.h"

namespace bgcn {
namespace {

constexpr int kTile = 32;               // one MFMA tile: 32 x 32 outputs
constexpr int kRowBlock = 128;          // rows per workgroup: four row tiles on one set of weight registers
constexpr int kFillGroups = 256;        // workgroups the split aims for (one per CU)
constexpr int64_t kMaxRows = int64_t(kRowBlock) * 65535;

// the four waves' tiles added in wave order; D register q of lane ln is row (q & 3) + 8 (q >> 2) +
// 4 (ln >> 5), column ln & 31
__device__ __forceinline__ void reduce_tile(float (&red)[4][kTile * 32], const f32x16& acc, int tid, int64_t m0,
                                            int64_t M, float* __restrict__ out, int64_t ld) {
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int q = 0; q < 16; ++q) red[wave][q * 64 + lane] = acc[q];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = tid + 256 * i, q = e >> 6, ln = e & 63;
    const float v = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
    const int64_t m = m0 + (q & 3) + 8 * (q >> 2) + 4 * (ln >> 5);
    if (m < M) out[m * ld + (ln & 31)] = v;
  }
  __syncthreads();
}

template <int KW>
__global__ __launch_bounds__(256) void k_skinny_xwt(const float* __restrict__ X, int64_t ldx,
                                                     const float* __restrict__ W, int64_t ldw,
                                                     float* __restrict__ part, int64_t M, int Nc) {
  __shared__ float red[4][kTile * 32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, r = lane & 31;
  const int nt = blockIdx.x, s = blockIdx.y;
  const int k0 = (s * 4 + wave) * KW * 16 + 8 * h;
  const float* wp = W + (int64_t(nt) * kTile + r) * ldw + k0;
  float4 w[KW][2];
#pragma unroll
  for (int i = 0; i < KW; ++i) {
    w[i][0] = ld4(wp + i * 16);
    w[i][1] = ld4(wp + i * 16 + 4);
  }
  const int64_t mb = int64_t(blockIdx.z) * kRowBlock, me = min<int64_t>(M, mb + kRowBlock);
  float* out = part + int64_t(s) * M * Nc + nt * kTile;
  for (int64_t m0 = mb; m0 < me; m0 += 32) {
    const float* xp = X + min<int64_t>(m0 + r, M - 1) * ldx + k0;
    float4 xa[KW][2];
#pragma unroll
    for (int i = 0; i < KW; ++i) {
      xa[i][0] = ld4(xp + i * 16);
      xa[i][1] = ld4(xp + i * 16 + 4);
    }
    f32x16 acc = {0};
#pragma unroll
    for (int i = 0; i < KW; ++i) {
      acc = mfma32x32x2(xa[i][0].x, w[i][0].x, acc);
      acc = mfma32x32x2(xa[i][0].y, w[i][0].y, acc);
      acc = mfma32x32x2(xa[i][0].z, w[i][0].z, acc);
      acc = mfma32x32x2(xa[i][0].w, w[i][0].w, acc);
      acc = mfma32x32x2(xa[i][1].x, w[i][1].x, acc);
      acc = mfma32x32x2(xa[i][1].y, w[i][1].y, acc);
      acc = mfma32x32x2(xa[i][1].z, w[i][1].z, acc);
      acc = mfma32x32x2(xa[i][1].w, w[i][1].w, acc);
    }
    reduce_tile(red, acc, tid, m0, M, out, Nc);
  }
}

template <int KW>
__global__ __launch_bounds__(256) void k_skinny_xw(const float* __restrict__ G, int64_t ldg,
                                                    const float* __restrict__ W, int64_t ldw,
                                                    float* __restrict__ part, int64_t M, int K) {
  __shared__ float red[4][kTile * 32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, r = lane & 31;
  const int kt = blockIdx.x, s = blockIdx.y;
  const int n0 = (s * 4 + wave) * KW * 16 + 8 * KW * h;
  const float* wp = W + int64_t(n0) * ldw + kt * kTile + r;
  float w[8 * KW];
#pragma unroll
  for (int j = 0; j < 8 * KW; ++j) w[j] = wp[j * ldw];
  const int64_t mb = int64_t(blockIdx.z) * kRowBlock, me = min<int64_t>(M, mb + kRowBlock);
  float* out = part + int64_t(s) * M * K + kt * kTile;
  for (int64_t m0 = mb; m0 < me; m0 += 32) {
    const float* gp = G + min<int64_t>(m0 + r, M - 1) * ldg + n0;
    float4 g[2 * KW];
#pragma unroll
    for (int i = 0; i < 2 * KW; ++i) g[i] = ld4(gp + 4 * i);
    f32x16 acc = {0};
#pragma unroll
    for (int i = 0; i < 2 * KW; ++i) {
      acc = mfma32x32x2(g[i].x, w[4 * i], acc);
      acc = mfma32x32x2(g[i].y, w[4 * i + 1], acc);
      acc = mfma32x32x2(g[i].z, w[4 * i + 2], acc);
      acc = mfma32x32x2(g[i].w, w[4 * i + 3], acc);
    }
    reduce_tile(red, acc, tid, m0, M, out, K);
  }
}

// one wave: dW rows [32 by, 32 by + 32) x columns [64 bx, 64 bx + 64); lane (h, r) feeds G[m + h][n0 + r]
// against X[m + h][k0 + 2 r + c], c < 2 (two tiles, one 8-byte load and store per lane and row)
__global__ __launch_bounds__(64) void k_skinny_tn(const float* __restrict__ G, int64_t ldg,
                                                   const float* __restrict__ X, int64_t ldx,
                                                   float* __restrict__ dW, int64_t ldw, int64_t M) {
  const int lane = threadIdx.x, h = lane >> 5, r = lane & 31;
  const int n0 = blockIdx.y * kTile, k0 = blockIdx.x * 64;
  const float* gp = G + n0 + r;
  const float* xp = X + k0 + 2 * r;
  f32x16 acc0 = {0}, acc1 = {0};
  for (int64_t m0 = 0; m0 < M; m0 += 8) {   // four instructions' loads in flight
    float g[4];
    float2 x[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t m = m0 + 2 * u + h, mm = min<int64_t>(m, M - 1);
      g[u] = gp[mm * ldg];
      x[u] = *reinterpret_cast<const float2*>(xp + mm * ldx);
      if (m >= M) {   // the odd row past the end adds exact zeros
        g[u] = 0.f;
        x[u] = make_float2(0.f, 0.f);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (m0 + 2 * u < M) {
        acc0 = mfma32x32x2(g[u], x[u].x, acc0);
        acc1 = mfma32x32x2(g[u], x[u].y, acc1);
      }
  }
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int n = n0 + (q & 3) + 8 * (q >> 2) + 4 * h;
    *reinterpret_cast<float2*>(dW + int64_t(n) * ldw + k0 + 2 * r) = make_float2(acc0[q], acc1[q]);
  }
}

// `red`: the reduction's length, `width`: the output's columns
int skinny_kw(int64_t red, int64_t width) {
  const int64_t ct = width / kTile, r64 = red / 64;
  for (int kw : {8, 4, 2})
    if (r64 % kw == 0 && ct * (r64 / kw) >= kFillGroups) return kw;
  return 1;
}

template <template <int> class Launch, class... A>
void launch_kw(int kw, A... a) {
  switch (kw) {
    case 8: Launch<8>::go(a...); break;
    case 4: Launch<4>::go(a...); break;
    case 2: Launch<2>::go(a...); break;
    default: Launch<1>::go(a...); break;
  }
}
template <int KW>
struct LaunchXwt {
  static void go(dim3 grid, hipStream_t s, const float* X, int64_t ldx, const float* W, int64_t ldw, float* part,
                 int64_t M, int Nc) {
    hipLaunchKernelGGL(k_skinny_xwt<KW>, grid, dim3(256), 0, s, X, ldx, W, ldw, part, M, Nc);
  }
};
template <int KW>
struct LaunchXw {
  static void go(dim3 grid, hipStream_t s, const float* G, int64_t ldg, const float* W, int64_t ldw, float* part,
                 int64_t M, int K) {
    hipLaunchKernelGGL(k_skinny_xw<KW>, grid, dim3(256), 0, s, G, ldg, W, ldw, part, M, K);
  }
};

bool ld_ok(const void* p, int64_t ld, int64_t width) { return p && a16(p) && ld >= width && ld % 4 == 0; }

}  // namespace

int skinny_splits_xwt(int64_t Nc, int64_t K) { return int(K / 64 / skinny_kw(K, Nc)); }
int skinny_splits_xw(int64_t Nc, int64_t K) { return int(Nc / 64 / skinny_kw(Nc, K)); }

size_t skinny_part_floats(int64_t M, int64_t Nc, int64_t K) {
  return size_t(M) * std::max(size_t(skinny_splits_xwt(Nc, K)) * size_t(Nc), size_t(skinny_splits_xw(Nc, K)) * size_t(K));
}

int gemm_xwt_skinny_impl(const float* X, int64_t ldx, const float* W, int64_t ldw, const float* bias, float* Y,
                         int64_t ldy, int64_t M, int64_t Nc, int64_t K, float* part, hipStream_t s) {
  const int kw = skinny_kw(K, Nc), S = int(K / 64 / kw);
  launch_kw<LaunchXwt>(kw, dim3(unsigned(Nc / kTile), unsigned(S), grid_for(M, kRowBlock)), s, X, ldx, W, ldw, part, M,
                       int(Nc));
  BGCN_CHECK_LAUNCH();
  return w16_reduce(part, S, M, Nc, bias, Y, ldy, s);
}

int gemm_xw_skinny_impl(const float* G, int64_t ldg, const float* W, int64_t ldw, float* Y, int64_t ldy, int64_t M,
                        int64_t Nc, int64_t K, float* part, hipStream_t s) {
  const int kw = skinny_kw(Nc, K), S = int(Nc / 64 / kw);
  launch_kw<LaunchXw>(kw, dim3(unsigned(K / kTile), unsigned(S), grid_for(M, kRowBlock)), s, G, ldg, W, ldw, part, M,
                      int(K));
  BGCN_CHECK_LAUNCH();
  return w16_reduce(part, S, M, K, nullptr, Y, ldy, s);
}

int gemm_tn_skinny_impl(const float* G, int64_t ldg, const float* X, int64_t ldx, float* dW, int64_t ldw, int64_t M,
                        int64_t Nc, int64_t K, hipStream_t s) {
  hipLaunchKernelGGL(k_skinny_tn, dim3(unsigned(K / 64), unsigned(Nc / kTile)), dim3(64), 0, s, G, ldg, X, ldx, dW, ldw, M);
  BGCN_CHECK_LAUNCH();
  return BGCN_OK;
}

}  // namespace bgcn

extern "C" size_t bgcn_gemm_skinny_workspace_size(int64_t M, int64_t Nc, int64_t K) {
  if (!bgcn::w16_shape_ok(Nc, K) || M < 1 || M > bgcn::kMaxRows) return 0;
  return bgcn::align_up(bgcn::skinny_part_floats(M, Nc, K) * sizeof(float), 256);
}

#define BGCN_SKINNY_SHAPE(M, Nc, K)                                      \
  BGCN_CHECK_ARG(w16_shape_ok(Nc, K) && M >= 1 && M <= kMaxRows,         \
                 "unsupported shape (M >= 1, Nc and K multiples of 64 in [64, 4096])")
#define BGCN_SKINNY_WS(M, Nc, K)                                                                              \
  BGCN_CHECK_ARG(workspace && a16(workspace) && workspace_bytes >= bgcn_gemm_skinny_workspace_size(M, Nc, K), \
                 "workspace too small")

extern "C" int bgcn_gemm_xwt_skinny(const float* X, int64_t ldx, const float* W, int64_t ldw, const float* bias,
                                    float* Y, int64_t ldy, int64_t M, int64_t Nc, int64_t K, void* workspace,
                                    size_t workspace_bytes, bgcn_stream_t stream) {
  using namespace bgcn;
  BGCN_SKINNY_SHAPE(M, Nc, K);
  BGCN_CHECK_ARG(ld_ok(X, ldx, K) && ld_ok(W, ldw, K) && ld_ok(Y, ldy, Nc) && a16(bias),
                 "X, W and Y: non-null, 16-byte aligned rows (ld % 4) of at least the row width; bias 16-byte aligned");
  BGCN_SKINNY_WS(M, Nc, K);
  return gemm_xwt_skinny_impl(X, ldx, W, ldw, bias, Y, ldy, M, Nc, K, static_cast<float*>(workspace),
                              reinterpret_cast<hipStream_t>(stream));
}

extern "C" int bgcn_gemm_xw_skinny(const float* G, int64_t ldg, const float* W, int64_t ldw, float* Y, int64_t ldy,
                                   int64_t M, int64_t Nc, int64_t K, void* workspace, size_t workspace_bytes,
                                   bgcn_stream_t stream) {
  using namespace bgcn;
  BGCN_SKINNY_SHAPE(M, Nc, K);
  BGCN_CHECK_ARG(ld_ok(G, ldg, Nc) && ld_ok(W, ldw, K) && ld_ok(Y, ldy, K),
                 "G, W and Y: non-null, 16-byte aligned rows (ld % 4) of at least the row width");
  BGCN_SKINNY_WS(M, Nc, K);
  return gemm_xw_skinny_impl(G, ldg, W, ldw, Y, ldy, M, Nc, K, static_cast<float*>(workspace),
                             reinterpret_cast<hipStream_t>(stream));
}

extern "C" int bgcn_gemm_tn_skinny(const float* G, int64_t ldg, const float* X, int64_t ldx, float* dW, int64_t ldw,
                                   int64_t M, int64_t Nc, int64_t K, bgcn_stream_t stream) {
  using namespace bgcn;
  BGCN_SKINNY_SHAPE(M, Nc, K);
  BGCN_CHECK_ARG(ld_ok(G, ldg, Nc) && ld_ok(X, ldx, K) && ld_ok(dW, ldw, K),
                 "G, X and dW: non-null, 16-byte aligned rows (ld % 4) of at least the row width");
  return gemm_tn_skinny_impl(G, ldg, X, ldx, dW, ldw, M, Nc, K, reinterpret_cast<hipStream_t>(stream));
}
