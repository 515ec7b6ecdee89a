// Skinny-M GEMM on bf16 weight images: Y[M, Nc] = X[M, K] (fp32) . W16[Nc, K]^T, for the weight-bound
// [B, hidden] chain of the TreeBERT root-only form (a few dozen rows against 1 - 5 MB of weights).
// A 128-column block tile leaves 6 - 24 workgroups for such a product; here K is split over waves
// and workgroups so that a 768 x 768 product is 288 workgroups, and the weights are read as bf16.
//
// Image (k_w16_pack).  W[Nc, K] rounded to bf16 (nearest even, torch's .to(bfloat16) bit for bit)
// and tiled in the B-operand order of v_mfma_f32_32x32x16_bf16: tile (nt, kt) = columns [32 nt,
// 32 nt + 32) x k [16 kt, 16 kt + 16) is 1 KB, lane l = 32 h + r holds W[32 nt + r][16 kt + 8 h + j],
// j < 8, as 16 bytes at byte 16 l.  Tiles are ordered [nt][kt]: the k-tiles a wave takes for its
// column tile are consecutive, and one wave load is one contiguous, fully coalesced 1 KB block.
// The image is 2 Nc K bytes.
//
// Product (k_gemm_w16<KW>).  Workgroup (nt, s, rb): column tile nt, k-slice s, rows [128 rb, 128 rb
// + 128).  Its four waves take KW consecutive k-tiles each (wave w: k-tiles (4 s + w) KW ..), load
// all of them before anything else, and keep them in registers across the row tiles of the block:
// per row tile of 32 rows, lane (h, r) loads X[m0 + r][k + 8 h ..+ 8] as fp32, splits it into three
// bf16 planes (split3_bf16) and runs three products per k-tile against the exact bf16 weight
// (mfma_planes<3, 1>: lo, mid, hi), fp32 accumulate.  The four accumulators are added through LDS in
// wave order and the sum is the workgroup's partial part[s][m][n].  The partials are summed in the
// order of s by k_w16_reduce (+ bias), or by the consuming row kernel (bgcn_bert.hip).
//
// The split: S = K / (64 KW) partials, KW the largest of 8, 4, 2 that divides K / 64 and still leaves
// (Nc / 32) S >= 256 workgroups, else 1.  A function of (Nc, K) alone: a row's bits do not depend on
// the other rows of the call.  No float atomics; rows past M are read as row M - 1 and not written.
#include "bgcn_internal.h"

namespace bgcn {
namespace {

constexpr int kTn = 32, kTk = 16;       // one MFMA B tile: columns x k
constexpr int kRowBlock = 128;          // rows per workgroup: four row tiles on one set of weight registers
constexpr int64_t kMinDim = 64, kMaxDim = 4096;
constexpr int kFillGroups = 256;        // workgroups the split aims for (one per CU)

// fp32 -> bf16 bits, round to nearest even (c10::detail::round_to_nearest_even)
__device__ __forceinline__ uint32_t bf16_rne(float x) {
  const uint32_t u = __float_as_uint(x);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

__global__ __launch_bounds__(256) void k_w16_pack(const float* __restrict__ W, int64_t ldw, int ktiles,
                                                   int64_t chunks, uint4* __restrict__ image, int vec) {
  const int64_t g = int64_t(blockIdx.x) * 256 + threadIdx.x;   // 16-byte chunk = tile * 64 + lane
  if (g >= chunks) return;
  const int lane = int(g & 63), r = lane & 31, h = lane >> 5;
  const int64_t tile = g >> 6, nt = tile / ktiles, kt = tile % ktiles;
  const float* src = W + (nt * kTn + r) * ldw + kt * kTk + 8 * h;
  float v[8];
  if (vec) {
    const float4 a = ld4(src), b = ld4(src + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = src[j];
  }
  uint4 o;
  o.x = bf16_rne(v[0]) | (bf16_rne(v[1]) << 16);
  o.y = bf16_rne(v[2]) | (bf16_rne(v[3]) << 16);
  o.z = bf16_rne(v[4]) | (bf16_rne(v[5]) << 16);
  o.w = bf16_rne(v[6]) | (bf16_rne(v[7]) << 16);
  image[g] = o;
}

template <int KW>
__global__ __launch_bounds__(256) void k_gemm_w16(const float* __restrict__ X, int64_t ldx,
                                                   const bf16x8* __restrict__ image, float* __restrict__ part,
                                                   int64_t M, int Nc, int ktiles) {
  __shared__ float red[4][kTn * 32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, r = lane & 31;
  const int nt = blockIdx.x, s = blockIdx.y;
  const int kt0 = (s * 4 + wave) * KW;
  const bf16x8* wp = image + (int64_t(nt) * ktiles + kt0) * 64 + lane;
  bf16x8 w[KW];
#pragma unroll
  for (int i = 0; i < KW; ++i) w[i] = wp[i * 64];
  const int64_t mb = int64_t(blockIdx.z) * kRowBlock, me = min<int64_t>(M, mb + kRowBlock);
  const int k0 = kt0 * kTk + 8 * h;
  float* out = part + int64_t(s) * M * Nc + nt * kTn;
  for (int64_t m0 = mb; m0 < me; m0 += 32) {
    const float* xp = X + min<int64_t>(m0 + r, M - 1) * ldx + k0;
    float4 xa[KW][2];
#pragma unroll
    for (int i = 0; i < KW; ++i) {
      xa[i][0] = ld4(xp + i * kTk);
      xa[i][1] = ld4(xp + i * kTk + 4);
    }
    f32x16 acc = {0};
#pragma unroll
    for (int i = 0; i < KW; ++i) {
      const float e[8] = {xa[i][0].x, xa[i][0].y, xa[i][0].z, xa[i][0].w, xa[i][1].x, xa[i][1].y, xa[i][1].z, xa[i][1].w};
      bf16x8 a[3];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        __bf16 x, y, z;
        split3_bf16(e[j], x, y, z);
        a[0][j] = x; a[1][j] = y; a[2][j] = z;
      }
      const bf16x8 b[1] = {w[i]};
      acc = mfma_planes<3, 1>(a, b, acc);
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) red[wave][q * 64 + lane] = acc[q];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = tid + 256 * i, q = e >> 6, ln = e & 63;
      const float v = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
      const int64_t m = m0 + (q & 3) + 8 * (q >> 2) + 4 * (ln >> 5);   // D register q of lane ln
      if (m < M) out[m * Nc + (ln & 31)] = v;
    }
    __syncthreads();
  }
}

// Y[m][c] = ((part[0] + part[1]) + ...)[m][c] (+ bias[c]), four columns per thread
__global__ __launch_bounds__(256) void k_w16_reduce(const float* __restrict__ part, int S, int64_t stride, int C4,
                                                     int64_t total4, const float* __restrict__ bias,
                                                     float* __restrict__ Y, int64_t ldy) {
  for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < total4; i += int64_t(gridDim.x) * 256) {
    const int64_t m = i / C4;
    const int c = int(i % C4) * 4;
    const float* p = part + i * 4;
    float4 v = ld4(p);
    int s = 1;
    for (; s + 4 <= S; s += 4) {   // four loads in flight; added in the order of s
      const float4 t0 = ld4(p + s * stride), t1 = ld4(p + (s + 1) * stride);
      const float4 t2 = ld4(p + (s + 2) * stride), t3 = ld4(p + (s + 3) * stride);
      v = f4add(f4add(f4add(f4add(v, t0), t1), t2), t3);
    }
    for (; s < S; ++s) v = f4add(v, ld4(p + s * stride));
    if (bias) v = f4add(v, ld4(bias + c));
    st4(Y + m * ldy + c, v);
  }
}

int w16_kw(int64_t Nc, int64_t K) {
  const int64_t ct = Nc / kTn, k64 = K / 64;
  for (int kw : {8, 4, 2})
    if (k64 % kw == 0 && ct * (k64 / kw) >= kFillGroups) return kw;
  return 1;
}

}  // namespace

bool w16_shape_ok(int64_t Nc, int64_t K) {
  return Nc >= kMinDim && Nc <= kMaxDim && Nc % 64 == 0 && K >= kMinDim && K <= kMaxDim && K % 64 == 0;
}

size_t w16_image_bytes(int64_t Nc, int64_t K) { return w16_shape_ok(Nc, K) ? size_t(2) * size_t(Nc) * size_t(K) : 0; }

int w16_splits(int64_t Nc, int64_t K) { return int(K / 64 / w16_kw(Nc, K)); }

size_t w16_part_floats(int64_t M, int64_t Nc, int64_t K) { return size_t(w16_splits(Nc, K)) * size_t(M) * size_t(Nc); }

int gemm_w16_partials(const float* X, int64_t ldx, const void* image, float* part, int64_t M, int64_t Nc, int64_t K,
                      hipStream_t s) {
  const int kw = w16_kw(Nc, K);
  const dim3 grid(unsigned(Nc / kTn), unsigned(K / 64 / kw), grid_for(M, kRowBlock));
  const bf16x8* img = static_cast<const bf16x8*>(image);
  const int ktiles = int(K / kTk);
  switch (kw) {
    case 8: hipLaunchKernelGGL(k_gemm_w16<8>, grid, dim3(256), 0, s, X, ldx, img, part, M, int(Nc), ktiles); break;
    case 4: hipLaunchKernelGGL(k_gemm_w16<4>, grid, dim3(256), 0, s, X, ldx, img, part, M, int(Nc), ktiles); break;
    case 2: hipLaunchKernelGGL(k_gemm_w16<2>, grid, dim3(256), 0, s, X, ldx, img, part, M, int(Nc), ktiles); break;
    default: hipLaunchKernelGGL(k_gemm_w16<1>, grid, dim3(256), 0, s, X, ldx, img, part, M, int(Nc), ktiles); break;
  }
  BGCN_CHECK_LAUNCH();
  return BGCN_OK;
}

int w16_reduce(const float* part, int S, int64_t M, int64_t Nc, const float* bias, float* Y, int64_t ldy, hipStream_t s) {
  const int64_t total4 = M * Nc / 4;
  hipLaunchKernelGGL(k_w16_reduce, dim3(unsigned(std::min<int64_t>((total4 + 255) / 256, 4096))), dim3(256), 0, s, part,
                     S, M * Nc, int(Nc / 4), total4, bias, Y, ldy);
  BGCN_CHECK_LAUNCH();
  return BGCN_OK;
}

}  // namespace bgcn

extern "C" size_t bgcn_w16_image_size(int64_t Nc, int64_t K) { return bgcn::w16_image_bytes(Nc, K); }

extern "C" int bgcn_w16_pack(const float* W, int64_t ldw, int64_t Nc, int64_t K, void* image, bgcn_stream_t stream) {
  using namespace bgcn;
  BGCN_CHECK_ARG(w16_shape_ok(Nc, K), "unsupported shape (Nc and K multiples of 64 in [64, 4096])");
  BGCN_CHECK_ARG(W && ldw >= K, "null W or ldw < K");
  BGCN_CHECK_ARG(image && a16(image), "null or unaligned weight image");
  const int64_t chunks = Nc * K / 8;
  const int vec = a16(W) && ldw % 4 == 0;
  hipLaunchKernelGGL(k_w16_pack, dim3(grid_for(chunks, 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), W, ldw,
                     int(K / kTk), chunks, static_cast<uint4*>(image), vec);
  BGCN_CHECK_LAUNCH();
  return BGCN_OK;
}

extern "C" size_t bgcn_gemm_xwt_w16_workspace_size(int64_t M, int64_t Nc, int64_t K) {
  if (!bgcn::w16_shape_ok(Nc, K) || M < 1 || M > int64_t(bgcn::kRowBlock) * 65535) return 0;
  return bgcn::align_up(bgcn::w16_part_floats(M, Nc, K) * sizeof(float), 256);
}

extern "C" int bgcn_gemm_xwt_w16(const float* X, int64_t ldx, const void* image, const float* bias, float* Y,
                                 int64_t ldy, int64_t M, int64_t Nc, int64_t K, void* workspace,
                                 size_t workspace_bytes, bgcn_stream_t stream) {
  using namespace bgcn;
  BGCN_CHECK_ARG(w16_shape_ok(Nc, K) && M >= 1 && M <= int64_t(kRowBlock) * 65535,
                 "unsupported shape (M >= 1, Nc and K multiples of 64 in [64, 4096])");
  BGCN_CHECK_ARG(X && Y, "null pointer");
  BGCN_CHECK_ARG(ldx >= K && ldx % 4 == 0 && a16(X) && ldy >= Nc && ldy % 4 == 0 && a16(Y) && a16(bias),
                 "X and Y rows and the bias must be 16-byte aligned (ldx % 4, ldy % 4)");
  BGCN_CHECK_ARG(image && a16(image), "null or unaligned weight image");
  BGCN_CHECK_ARG(workspace && a16(workspace) && workspace_bytes >= bgcn_gemm_xwt_w16_workspace_size(M, Nc, K),
                 "workspace too small");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  float* part = static_cast<float*>(workspace);
  BGCN_TRY(gemm_w16_partials(X, ldx, image, part, M, Nc, K, s));
  return w16_reduce(part, w16_splits(Nc, K), M, Nc, bias, Y, ldy, s);
}
