// bgcn_lstm_train_grad: one iteration of the LSTM baseline's training loop up to the optimiser
// (model/Twitter/LSTM_Twitter.py:96-126: forward, mean NLL, accuracy, backward) for a whole batch
// of trees as one launch sequence on the caller's stream, everything in the caller's workspace.
//
//   forward         lstm_forward (bgcn_lstm.hip) with save = true: bgcn_lstm_eval's launches, the
//                   step as k_lstm_step<true>: per layer the activated gates A_l [N, 8H] go over G
//                   in place and the cell states into C_l [N, 2H]
//   k_lstm_bwd_setup   zero dY_{L-1}; zero the rows above seq_start[0] of every A_l and of Hprev
//   k_lstm_head_bwd    per tree: dz = (softmax - onehot(y)) / B, d h_n = dz fc.weight
//   k_lstm_fc_grad     d fc.weight = dz^T h_n, d fc.bias = column sums of dz (over b in order),
//                      skip_flag
//   per layer l = L-1 .. 0
//     k_lstm_seed      dY_l += d h_n: the forward half at a tree's last row, the reverse half at
//                      its first
//     k_lstm_whh_t     W_hh^T of both directions [2][H][4H]: the forward step's operand pattern
//     k_lstm_bwd_step x max_len, s downwards: dh = dY_l[row] + W_hh^T dpre(step s + 1), the gate
//                      derivatives over A_l's row in place, the dc carry
//     dW_ih = dG_l^T X_l (gemm_tn), k_lstm_shift + dW_hh[d] = dG_l[:, d]^T Hprev[:, d] (gemm_tn),
//     dX_l = dG_l [W_ih_fwd ; W_ih_rev] (gemm_xw2) = dY_{l-1}, or the caller's dx
//
// Stream order is the only dependency between workgroups; no float atomics, every sum in a
// fixed order.  This file holds the backward's kernels and launches only.
#include "bgcn_lstm.h"

namespace bgcn {
namespace {

constexpr int kBwdUnits = 32;    // hidden units per workgroup of a backward step: the MFMA's 32 rows
constexpr int kShiftRows = 8;    // rows of a tree per workgroup of k_lstm_shift

// ---- zero what the GEMMs read but no tree owns or no launch writes
struct BwdSetupArgs {
  const int64_t* seq_start;
  int64_t N;
  float* A[kMaxLayers];   // [N, 8H]
  int L;
  int64_t H;
  float* Hprev;           // [N, 2H]
  float* dYtop;           // [N, 2H]
};
__global__ __launch_bounds__(256) void k_lstm_bwd_setup(BwdSetupArgs a) {
  const int64_t i0 = int64_t(blockIdx.x) * 256 + threadIdx.x, stride = int64_t(gridDim.x) * 256;
  const int64_t ny = a.N * 2 * a.H;
  for (int64_t i = i0; i < ny; i += stride) a.dYtop[i] = 0.f;
  const int64_t s0 = lstm_first_start(a.seq_start, a.N);
  const int64_t na = s0 * 8 * a.H, nh = s0 * 2 * a.H;
  for (int l = 0; l < a.L; ++l)
    for (int64_t i = i0; i < na; i += stride) a.A[l][i] = 0.f;
  for (int64_t i = i0; i < nh; i += stride) a.Hprev[i] = 0.f;
}

// ---- head backward, workgroup b = sequence b
struct HeadBwdArgs {
  const float* logp;   // [B, C]
  const int64_t* y;
  const float* W;      // [C, D]
  int64_t B;
  int C, D;
  float* dz;           // [B, C]
  float* dhn;          // [B, D], D ordered (l0 fwd, l0 rev, l1 fwd, ...)
};
__global__ __launch_bounds__(256) void k_lstm_head_bwd(HeadBwdArgs a) {
  __shared__ float dzs[kMaxOut];
  const int t = threadIdx.x;
  const int64_t b = blockIdx.x;
  if (t < a.C) {
    const int64_t yb = a.y[b];
    const bool yok = yb >= 0 && yb < a.C;
    const float g = yok ? (expf(a.logp[b * a.C + t]) - (t == yb ? 1.f : 0.f)) / float(a.B) : 0.f;
    dzs[t] = g;
    a.dz[b * a.C + t] = g;
  }
  __syncthreads();
  for (int k = t; k < a.D; k += 256) {
    float acc = 0.f;
    for (int c = 0; c < a.C; ++c) acc = fmaf(dzs[c], a.W[int64_t(c) * a.D + k], acc);
    a.dhn[b * a.D + k] = acc;
  }
}

// ---- d fc.weight [C, D], d fc.bias [C], skip_flag.  Block (x, c < C): columns 256 x .. of row c,
// the trees in order; block (0, C): the bias and the flag.
struct FcGradArgs {
  const float* dz;    // [B, C]
  const float* h_n;   // [2L, B, H]
  int64_t B;
  int C, D, H;
  float *dW, *db;
  const int32_t* status;
  float* skip_flag;
};
__global__ __launch_bounds__(256) void k_lstm_fc_grad(FcGradArgs a) {
  const int t = threadIdx.x, c = blockIdx.y;
  if (c == a.C) {
    if (blockIdx.x != 0) return;
    if (t < a.C) {
      float s = 0.f;
      for (int64_t b = 0; b < a.B; ++b) s += a.dz[b * a.C + t];
      a.db[t] = s;
    }
    if (t == 0) *a.skip_flag = *a.status != 0 ? 1.0f : 0.0f;   // every status bit is known after the head
    return;
  }
  const int k = blockIdx.x * 256 + t;
  if (k >= a.D) return;
  const int ld = k / a.H, kk = k - ld * a.H;   // ld = 2 layer + direction
  const float* hp = a.h_n + int64_t(ld) * a.B * a.H + kk;
  float acc = 0.f;
  for (int64_t b = 0; b < a.B; ++b) acc = fmaf(a.dz[b * a.C + c], hp[b * a.H], acc);
  a.dW[int64_t(c) * a.D + k] = acc;
}

// ---- dY_l += d h_n of layer l, workgroup b = sequence b: one thread per element, no order to fix
struct SeedArgs {
  float* dY;          // [N, 2H]
  const float* dhn;   // [B, D]
  SeqInfo sq;
  int H, D, layer;
};
__global__ __launch_bounds__(256) void k_lstm_seed(SeedArgs a) {
  const int64_t b = blockIdx.x;
  const int64_t start = a.sq.start[b], len = a.sq.len[b];
  if (len <= 0) return;
  for (int col = threadIdx.x; col < 2 * a.H; col += 256) {
    const int64_t row = col < a.H ? start + len - 1 : start;
    a.dY[row * (2 * int64_t(a.H)) + col] += a.dhn[b * a.D + a.layer * 2 * a.H + col];
  }
}

// ---- WT[d][u][k] = W_hh[d][k][u]: 32 x 32 tiles through LDS, grid (H / 32, 4H / 32, 2)
struct WhhTArgs {
  const float* W[2];   // [4H, H]
  float* WT;           // [2][H][4H]
  int H;
};
__global__ __launch_bounds__(256) void k_lstm_whh_t(WhhTArgs a) {
  __shared__ float tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5, d = blockIdx.z;
  const int u0 = blockIdx.x * 32, k0 = blockIdx.y * 32;
  const int64_t H = a.H;
  for (int i = ty; i < 32; i += 8) tile[i][tx] = a.W[d][(k0 + i) * H + u0 + tx];
  __syncthreads();
  for (int i = ty; i < 32; i += 8) a.WT[(d * H + u0 + i) * 4 * H + k0 + tx] = tile[tx][i];
}

// ---- one backward step.  Workgroup (slice, dir, tile): hidden units [32 slice, 32 slice + 32) of
// direction dir for the sequences [32 tile, 32 tile + 32).  D[i][j] = sum_k WT[32 slice + i][k]
// dpre[j][k] over the 4H gate pre-activation gradients of step s + 1 (A_l at the row of that
// step), on v_mfma_f32_32x32x2_f32 with k split over the four waves (wave w: [w H, (w + 1) H)),
// the forward step's operand pattern.  D's register 4q + w of lane (j, h) is unit w + 8q + 4h of
// sequence j: thread (wave w, lane (j, h)) adds the four waves' partial tiles in wave order and
// owns four units of its sequence.  At s = len - 1 the sequence has no later step: its lanes feed
// zeros to the product, and neither the product nor the dc carry enters dh / dc.
struct BwdStepArgs {
  float* A;           // [N, 8H] the activated gates; a row becomes its dpre
  const float* C;     // [N, 2H]
  const float* dY;    // [N, 2H]
  const float* WT;    // [2][H][4H]
  float* dc;          // [2, B, H] the carry dc f of the step above
  SeqInfo sq;
  int64_t B;
  int H;
  int s;
};
__global__ __launch_bounds__(256) void k_lstm_bwd_step(BwdStepArgs a) {
  __shared__ float part[4][16][64];
  const int t = threadIdx.x, w = t >> 6, l = t & 63, r = l & 31, h = l >> 5;
  const int H = a.H, s = a.s, dir = blockIdx.y;
  const int64_t sj = int64_t(blockIdx.z) * kSeqTile + r;
  int32_t start = 0, len = 0;
  if (sj < a.B) {
    start = a.sq.start[sj];
    len = a.sq.len[sj];
  }
  const bool active = s < len;
  if (__ballot(active) == 0) return;   // every wave sees the tile's 32 sequences: uniform
  const int64_t row = dir == 0 ? int64_t(start) + s : int64_t(start) + len - 1 - s;
  const int64_t nrow = dir == 0 ? row + 1 : row - 1;   // the row of step s + 1
  const int64_t prow = dir == 0 ? row - 1 : row + 1;   // the row of step s - 1
  const bool rec = active && s < len - 1;
  const int64_t ldy = 2 * int64_t(H), lda = 8 * int64_t(H);

  // the epilogue's operands, requested before the product: units w + 4h + 8q of sequence r
  const int hid0 = blockIdx.x * kBwdUnits + w + 4 * h;
  float gate[4][4], cc[4], cprev[4], dcar[4], dy[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    cc[q] = cprev[q] = dcar[q] = dy[q] = 0.f;
#pragma unroll
    for (int g = 0; g < 4; ++g) gate[q][g] = 0.f;
  }
  float* ap = a.A + (active ? row : 0) * lda + int64_t(dir) * 4 * H + hid0;
  float* dcp = a.dc + (int64_t(dir) * a.B + (sj < a.B ? sj : 0)) * H + hid0;
  if (active) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int g = 0; g < 4; ++g) gate[q][g] = ap[g * H + 8 * q];
      cc[q] = a.C[row * ldy + int64_t(dir) * H + hid0 + 8 * q];
      dy[q] = a.dY[row * ldy + int64_t(dir) * H + hid0 + 8 * q];
      if (s > 0) cprev[q] = a.C[prow * ldy + int64_t(dir) * H + hid0 + 8 * q];
      if (rec) dcar[q] = dcp[8 * q];
    }
  }

  f32x16 acc;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = 0.f;
  if (__ballot(rec) != 0) {   // the same 32 sequences in every wave: uniform over the workgroup
    const float* wr = a.WT + (int64_t(dir) * H + blockIdx.x * kBwdUnits + r) * 4 * H;
    const float* dp = a.A + (rec ? nrow : 0) * lda + int64_t(dir) * 4 * H;
    const int k1 = (w + 1) * H;
    for (int k = w * H + 8 * h; k < k1; k += 16) {
      const float4 a0 = ld4(wr + k), a1 = ld4(wr + k + 4);
      // (a lane without a later step loads row 0, in bounds, and drops it: no branch in the loop)
      float4 b0 = ld4(dp + k), b1 = ld4(dp + k + 4);
      if (!rec) b0 = b1 = f4zero();
      acc = mfma32x32x2(a0.x, b0.x, acc);
      acc = mfma32x32x2(a0.y, b0.y, acc);
      acc = mfma32x32x2(a0.z, b0.z, acc);
      acc = mfma32x32x2(a0.w, b0.w, acc);
      acc = mfma32x32x2(a1.x, b1.x, acc);
      acc = mfma32x32x2(a1.y, b1.y, acc);
      acc = mfma32x32x2(a1.z, b1.z, acc);
      acc = mfma32x32x2(a1.w, b1.w, acc);
    }
  }
#pragma unroll
  for (int q = 0; q < 16; ++q) part[w][q][l] = acc[q];
  __syncthreads();
  if (!active) return;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int reg = 4 * q + w;
    const float rsum = ((part[0][reg][l] + part[1][reg][l]) + part[2][reg][l]) + part[3][reg][l];
    const float dh = rec ? dy[q] + rsum : dy[q];
    const float ig = gate[q][0], fg = gate[q][1], gg = gate[q][2], og = gate[q][3];
    const float tc = tanhf(cc[q]);
    const float dc = dcar[q] + dh * og * (1.0f - tc * tc);
    ap[8 * q] = dc * gg * ig * (1.0f - ig);
    ap[H + 8 * q] = dc * cprev[q] * fg * (1.0f - fg);
    ap[2 * H + 8 * q] = dc * ig * (1.0f - gg * gg);
    ap[3 * H + 8 * q] = dh * tc * og * (1.0f - og);
    dcp[8 * q] = dc * fg;
  }
}

// ---- Hprev: Y_l shifted by one row inside each tree, zero where a tree has no such row.  Forward
// half: the previous row; reverse half: the next row.  Block (chunk, b) strides over the trees and
// the chunks of kShiftRows rows.
struct ShiftArgs {
  const float* Y;   // [N, 2H]
  float* Hprev;     // [N, 2H]
  SeqInfo sq;
  int64_t B;
  int H;
};
__global__ __launch_bounds__(256) void k_lstm_shift(ShiftArgs a) {
  const int H = a.H, W = 2 * H;
  for (int64_t b = blockIdx.y; b < a.B; b += gridDim.y) {
    const int64_t start = a.sq.start[b], len = a.sq.len[b];
    for (int64_t i0 = int64_t(blockIdx.x) * kShiftRows; i0 < len; i0 += int64_t(gridDim.x) * kShiftRows) {
      const int rows = int(len - i0 < kShiftRows ? len - i0 : kShiftRows);
      for (int idx = threadIdx.x; idx < rows * W; idx += 256) {
        const int rr = idx / W, col = idx - rr * W;
        const int64_t i = i0 + rr, row = start + i;
        float v = 0.f;
        if (col < H) {
          if (i > 0) v = a.Y[(row - 1) * W + col];
        } else if (i < len - 1) {
          v = a.Y[(row + 1) * W + col];
        }
        a.Hprev[row * W + col] = v;
      }
    }
  }
}

struct TrainWs {
  LstmFwdWs f;            // the forward's share: G[l] holds A_l
  float* dc;              // [2, B, H]
  float* dY[2];           // [N, 2H]: dY_l in dY[l & 1]
  float* Hprev;           // [N, 2H]
  float* WT;              // [2][H][4H]
  float *dz, *h_n, *dhn;  // [B, C <= 64], [2L, B, H], [B, 2LH]
  void* tn;
  size_t tn_bytes;
};

size_t carve_train(Carve& c, int64_t N, int64_t B, int64_t F, int64_t H, int64_t L, float* out, TrainWs* w) {
  const size_t n = size_t(N), nb = size_t(B), h = size_t(H);
  carve_lstm_fwd(c, N, B, H, L, true, out, &w->f);
  w->dc = c.take<float>(2 * nb * h);
  w->dY[0] = c.take<float>(n * 2 * h);
  w->dY[1] = c.take<float>(n * 2 * h);
  w->Hprev = c.take<float>(n * 2 * h);
  w->WT = c.take<float>(2 * h * 4 * h);
  w->dz = c.take<float>(nb * kMaxOut);
  w->h_n = c.take<float>(2 * size_t(L) * nb * h);
  w->dhn = c.take<float>(2 * size_t(L) * nb * h);
  size_t tn = std::max(tn_ws_size(8 * H, F, N), tn_ws_size(4 * H, H, N));
  if (L > 1) tn = std::max(tn, tn_ws_size(8 * H, 2 * H, N));
  w->tn_bytes = tn;
  w->tn = c.take<char>(tn);
  return align_up(c.off, 256);
}

}  // namespace

int lstm_train_grad_impl(const bgcn_lstm_train_args* ta, void* ws, size_t ws_bytes, hipStream_t s) {
  BGCN_CHECK_ARG(ta, "null args");
  const bgcn_lstm_args* a = &ta->fwd;
  BGCN_TRY(lstm_check_args(a, ws));
  const int64_t N = a->num_nodes, B = a->num_seqs, F = a->in_feats, H = a->hid, L = a->num_layers,
                C = a->out_feats;
  BGCN_CHECK_ARG(a->y && ta->d_fc_w && ta->d_fc_b && ta->skip_flag, "null pointer");
  BGCN_CHECK_ARG(a16(ta->dx), "x and dx rows must be 16-byte aligned (ldx % 4)");
  for (int l = 0; l < L; ++l)
    for (int d = 0; d < 2; ++d)
      BGCN_CHECK_ARG(ta->d_w_ih[l][d] && ta->d_w_hh[l][d] && a16(ta->d_w_ih[l][d]) && a16(ta->d_w_hh[l][d]),
                     "null or unaligned LSTM weight gradient");
  TrainWs w;
  Carve c(ws, ws_bytes);
  carve_train(c, N, B, F, H, L, a->out, &w);
  BGCN_CHECK_ARG(ws && c.ok(), "workspace too small");
  float* h_n = a->h_n ? a->h_n : w.h_n;
  const int D = int(2 * L * H);
  const int64_t steps = std::min<int64_t>(a->max_len, N);
  const LstmFwdWs& f = w.f;

  BGCN_TRY(lstm_forward(a, f, true, h_n, s));   // the gates and cell states kept

  // ---- backward: the head
  const int top = int(L - 1);
  BwdSetupArgs bs{a->seq_start, N, {f.G[0], f.G[1], f.G[2], f.G[3]}, int(L), H, w.Hprev, w.dY[top & 1]};
  hipLaunchKernelGGL(k_lstm_bwd_setup, dim3(std::min<unsigned>(grid_for(N * 2 * H, 1024), 1024)), dim3(256), 0, s, bs);
  BGCN_CHECK_LAUNCH();
  HeadBwdArgs hb{a->logp, a->y, a->fc_w, B, int(C), D, w.dz, w.dhn};
  hipLaunchKernelGGL(k_lstm_head_bwd, dim3(unsigned(B)), dim3(256), 0, s, hb);
  BGCN_CHECK_LAUNCH();
  FcGradArgs fg{w.dz, h_n, B, int(C), D, int(H), ta->d_fc_w, ta->d_fc_b, a->status, ta->skip_flag};
  hipLaunchKernelGGL(k_lstm_fc_grad, dim3(grid_for(D, 256), unsigned(C + 1)), dim3(256), 0, s, fg);
  BGCN_CHECK_LAUNCH();

  // ---- backward through the layers
  const dim3 bgrid(unsigned(H / kBwdUnits), 2, grid_for(B, kSeqTile));
  const dim3 sgrid(unsigned(std::min<int64_t>((steps + kShiftRows - 1) / kShiftRows, 1024)),
                   unsigned(std::min<int64_t>(B, 65535)));
  for (int l = top; l >= 0; --l) {
    float* dY = w.dY[l & 1];
    SeedArgs sd{dY, w.dhn, f.sq, int(H), D, l};
    hipLaunchKernelGGL(k_lstm_seed, dim3(unsigned(B)), dim3(256), 0, s, sd);
    WhhTArgs wt{{a->w_hh[l][0], a->w_hh[l][1]}, w.WT, int(H)};
    hipLaunchKernelGGL(k_lstm_whh_t, dim3(unsigned(H / 32), unsigned(4 * H / 32), 2), dim3(256), 0, s, wt);
    BGCN_CHECK_LAUNCH();
    BwdStepArgs st{f.G[l], f.C[l], dY, w.WT, w.dc, f.sq, B, int(H), 0};
    for (int64_t k = steps - 1; k >= 0; --k) {
      st.s = int(k);
      hipLaunchKernelGGL(k_lstm_bwd_step, bgrid, dim3(256), 0, s, st);
    }
    BGCN_CHECK_LAUNCH();
    const float* X = l == 0 ? a->x : f.Y[l - 1];
    const int64_t K = l == 0 ? F : 2 * H, ldx = l == 0 ? a->ldx : 2 * H;
    BGCN_TRY(gemm_tn_impl(f.G[l], 8 * H, X, ldx, ta->d_w_ih[l][0], ta->d_w_ih[l][1], K, 4 * H, 8 * H, K, N, w.tn,
                          w.tn_bytes, s, -1, nullptr));
    ShiftArgs sh{f.Y[l], w.Hprev, f.sq, B, int(H)};
    hipLaunchKernelGGL(k_lstm_shift, sgrid, dim3(256), 0, s, sh);
    BGCN_CHECK_LAUNCH();
    for (int d = 0; d < 2; ++d)
      BGCN_TRY(gemm_tn_impl(f.G[l] + d * 4 * H, 8 * H, w.Hprev + d * H, 2 * H, ta->d_w_hh[l][d], nullptr, H, 4 * H,
                            4 * H, H, N, w.tn, w.tn_bytes, s, -1, nullptr));
    float* dX = l > 0 ? w.dY[(l - 1) & 1] : ta->dx;
    if (dX)
      BGCN_TRY(gemm_xw2_impl(f.G[l], 8 * H, a->w_ih[l][0], a->w_ih[l][1], K, 4 * H, dX, l > 0 ? 2 * H : a->ldx, N, K,
                             8 * H, s));
  }
  return BGCN_OK;
}

}  // namespace bgcn

extern "C" size_t bgcn_lstm_train_workspace_size(int64_t num_nodes, int64_t num_seqs, int64_t in_feats, int64_t hid,
                                                 int64_t num_layers) {
  if (!bgcn::lstm_shape_ok(num_nodes, num_seqs, in_feats, hid, num_layers)) return 0;
  bgcn::TrainWs w;
  bgcn::Carve c(nullptr, 0);
  return bgcn::carve_train(c, num_nodes, num_seqs, in_feats, hid, num_layers, nullptr, &w);
}

extern "C" int bgcn_lstm_train_grad(const bgcn_lstm_train_args* args, void* workspace, size_t workspace_bytes,
                                    bgcn_stream_t stream) {
  return bgcn::lstm_train_grad_impl(args, workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream));
}
