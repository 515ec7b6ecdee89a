// The LSTM baseline's forward, and bgcn_lstm_eval: the test loop body (model/Twitter/LSTM_Twitter.py:
// 146-173) for a whole batch of trees as one launch sequence on the caller's stream, everything in
// the caller's workspace.  Each tree is one sequence: the rows [seq_start[b], seq_start[b + 1]) of x
// (the last one runs to N).  nn.LSTM(in, H, num_layers = L, bidirectional, bias = False), h0 = c0 = 0.
//
//   k_lstm_setup    the sequences' (start, len), their validity (the status word), zero rows of
//                   every layer output above seq_start[0]
//   per layer l     G[N, 8H] = X_l [W_ih_fwd ; W_ih_rev]^T    (gemm_xwt, split = 4H;
//                                                               X_0 = x, X_l = Y_{l-1} [N, 2H])
//                   k_lstm_step x max_len: step s of both directions and all sequences
//   k_lstm_head     one workgroup per sequence: the 2L final states, fc, log_softmax, the NLL
//                   term, the argmax
//   k_lstm_finish   one workgroup: mean loss and correct count, fixed order
//
// Stream order between the step launches is the only dependency between workgroups.  The kernels
// and lstm_forward, their launch sequence, exist once, here: the training entry point
// (bgcn_lstm_train.hip) calls lstm_forward with save = true (k_lstm_step<true> keeps the activated
// gates and the cell state of every row for the backward), so both entry points run the same code.
#include "bgcn_lstm.h"

namespace bgcn {
namespace {

constexpr int kUnits = 8;   // hidden units per workgroup: 8 x 4 gates = the MFMA's 32 rows

// ---- setup.  Block 0: validity of seq_start over all sequences; one fault empties every
// sequence (len = 0: the steps do nothing, the head sees zero states), so a faulted batch
// touches no row twice and nothing out of range.  Every block: zero the rows above the first
// sequence in each layer output.
struct SetupArgs {
  const int64_t* seq_start;
  int64_t B, N, max_len;
  SeqInfo sq;
  float* Y[kMaxLayers];
  int L;
  int64_t ldy;   // 2H
  int32_t* status;
};
__global__ __launch_bounds__(256) void k_lstm_setup(SetupArgs a) {
  const int t = threadIdx.x;
  if (blockIdx.x == 0) {
    int bad = 0;
    for (int64_t b = t; b < a.B; b += 256) {
      const int64_t st = a.seq_start[b], en = b + 1 < a.B ? a.seq_start[b + 1] : a.N;
      bad |= (st < 0 || st >= a.N || en <= st || en > a.N || en - st > a.max_len) ? 1 : 0;
    }
    bad = __syncthreads_or(bad);
    for (int64_t b = t; b < a.B; b += 256) {
      const int64_t st = a.seq_start[b], en = b + 1 < a.B ? a.seq_start[b + 1] : a.N;
      a.sq.start[b] = bad ? 0 : int32_t(st);
      a.sq.len[b] = bad ? 0 : int32_t(en - st);
    }
    if (t == 0) *a.status = bad ? BGCN_STATUS_SEQUENCE : 0;   // the call's first launch
  }
  const int64_t total = lstm_first_start(a.seq_start, a.N) * a.ldy;
  for (int l = 0; l < a.L; ++l)
    for (int64_t i = int64_t(blockIdx.x) * 256 + t; i < total; i += int64_t(gridDim.x) * 256) a.Y[l][i] = 0.f;
}

// ---- one step.  Workgroup (slice, dir, tile): hidden units [8 slice, 8 slice + 8) of direction
// dir for the sequences [32 tile, 32 tile + 32).  The 32 x 32 tile D[i][j] = sum_k W_hh[row(i)][k]
// h_prev[j][k], row(i) = (i >> 3) H + 8 slice + (i & 7) (gate i >> 3 in the order i, f, g, o), on
// v_mfma_f32_32x32x2_f32 with k split over the four waves (wave w: [w H / 4, (w + 1) H / 4)).
// Lane (r = l & 31, h = l >> 5) loads 8 consecutive k of its W row and of its sequence's h_prev
// per 16-k iteration (k0 + 8h ..); MFMA t pairs k0 + t with k0 + 8 + t on both operands.  D's
// register 4g + u of lane (j, h) is gate g of unit u + 4h of sequence j: the four waves' partial
// tiles meet in LDS and thread (wave u, lane (j, h)) adds them in wave order, adds G, applies the
// gates and owns c[dir][j][unit].  SAVE (the training forward): the activated gates i, f, g, o go
// over the row's own four entries of G and the new cell state into C[row], for the backward.
struct StepArgs {
  float* G;            // [N, 8H]
  const float* Whh[2]; // [4H, H] per direction
  float* Y;            // [N, 2H] this layer's output; h_prev is read from it
  float* c;            // [2, B, H]
  SeqInfo sq;
  int64_t B;
  int H;
  int s;
  float* C;            // SAVE: [N, 2H] the cell state of every row
};
__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

template <bool SAVE>
__global__ __launch_bounds__(256) void k_lstm_step(StepArgs a) {
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
  const int64_t prow = dir == 0 ? row - 1 : row + 1;
  const bool hp_ok = active && s > 0;
  const int64_t ldy = 2 * int64_t(H);

  // the epilogue's operands, requested before the product: unit w + 4h of sequence r
  const int hid = blockIdx.x * kUnits + w + 4 * h;
  float gin[4] = {0.f, 0.f, 0.f, 0.f}, cprev = 0.f;
  float* cp = a.c + (int64_t(dir) * a.B + (sj < a.B ? sj : 0)) * H + hid;
  if (active) {
    const float* g = a.G + row * (8 * int64_t(H)) + int64_t(dir) * 4 * H + hid;
#pragma unroll
    for (int q = 0; q < 4; ++q) gin[q] = g[q * H];
    if (s > 0) cprev = *cp;
  }

  f32x16 acc;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = 0.f;
  if (s > 0) {   // h_prev = 0 at s = 0: the product is zero
    const float* wr = a.Whh[dir] + (int64_t(r >> 3) * H + blockIdx.x * kUnits + (r & 7)) * H;
    const float* hp = a.Y + (hp_ok ? prow : 0) * ldy + int64_t(dir) * H;
    const int k1 = (w + 1) * (H >> 2);
    for (int k = w * (H >> 2) + 8 * h; k < k1; k += 16) {
      const float4 a0 = ld4(wr + k), a1 = ld4(wr + k + 4);
      // (a lane without a previous row loads row 0, in bounds, and drops it: no branch in the loop)
      float4 b0 = ld4(hp + k), b1 = ld4(hp + k + 4);
      if (!hp_ok) b0 = b1 = f4zero();
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
  float pre[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int reg = 4 * q + w;
    pre[q] = gin[q] + (((part[0][reg][l] + part[1][reg][l]) + part[2][reg][l]) + part[3][reg][l]);
  }
  const float ig = sigmoidf_(pre[0]), fg = sigmoidf_(pre[1]), gg = tanhf(pre[2]), og = sigmoidf_(pre[3]);
  const float cn = fg * cprev + ig * gg;
  *cp = cn;
  a.Y[row * ldy + int64_t(dir) * H + hid] = og * tanhf(cn);
  if constexpr (SAVE) {
    float* g = a.G + row * (8 * int64_t(H)) + int64_t(dir) * 4 * H + hid;
    g[0] = ig;
    g[H] = fg;
    g[2 * H] = gg;
    g[3 * H] = og;
    a.C[row * ldy + int64_t(dir) * H + hid] = cn;
  }
}

// ---- head, workgroup b = sequence b: h_n (l0 fwd, l0 rev, l1 fwd, ...) gathered from the layer
// outputs (forward: the sequence's last row, reverse: its first), fc by the four waves (class c
// by wave c % 4), then wave 0: log_softmax, the NLL term, the first maximal class.
struct LstmHeadArgs {
  const float* Y[kMaxLayers];
  SeqInfo sq;
  int64_t B;
  int H, L, C;
  const float *W, *bias;   // [C, 2 L H], [C]
  const int64_t* y;
  float *logp, *h_n, *loss_row;
  int32_t* predw;
  int64_t* pred;
  int32_t* status;
};
__global__ __launch_bounds__(256) void k_lstm_head(LstmHeadArgs a) {
  __shared__ __attribute__((aligned(16))) float hn[2 * kMaxLayers * 1024];
  __shared__ float z[kMaxOut];
  const int t = threadIdx.x, w = t >> 6, l = t & 63;
  const int64_t b = blockIdx.x;
  const int H = a.H, D = 2 * a.L * H;
  const int64_t start = a.sq.start[b], len = a.sq.len[b];
  for (int idx = t; idx < D; idx += 256) {
    const int lay = idx / (2 * H), rem = idx - lay * 2 * H, dir = rem / H, k = rem - dir * H;
    float v = 0.f;
    if (len > 0) v = a.Y[lay][(dir == 0 ? start + len - 1 : start) * (2 * int64_t(H)) + rem];
    hn[idx] = v;
    if (a.h_n) a.h_n[(int64_t(2 * lay + dir) * a.B + b) * H + k] = v;
  }
  __syncthreads();
  for (int c = w; c < a.C; c += 4) {
    const float* wr = a.W + int64_t(c) * D;
    float p = 0.f;
    for (int k = 4 * l; k < D; k += 256) {
      const float4 x = ld4(&hn[k]), v = ld4(wr + k);
      p = fmaf(x.x, v.x, fmaf(x.y, v.y, fmaf(x.z, v.z, fmaf(x.w, v.w, p))));
    }
    p = wave_sum(p);
    if (l == 0) z[c] = p + a.bias[c];
  }
  __syncthreads();
  if (w != 0) return;
  seq_head_tail(z, a.C, b, l, a.y, a.logp, a.loss_row, a.predw, a.pred, a.status);
}

// the mean NLL and the correct count over the sequences: strided thread sums, then a halving tree
__global__ __launch_bounds__(256) void k_lstm_finish(const float* __restrict__ loss_row,
                                                     const int32_t* __restrict__ predw,
                                                     const int64_t* __restrict__ y, int64_t B,
                                                     float* __restrict__ loss, int32_t* __restrict__ correct) {
  __shared__ float ls[256];
  __shared__ int32_t cs[256];
  const int t = threadIdx.x;
  float s = 0.f;
  int32_t n = 0;
  for (int64_t b = t; b < B; b += 256) {
    s += loss_row[b];
    n += (y && y[b] == int64_t(predw[b])) ? 1 : 0;
  }
  ls[t] = s;
  cs[t] = n;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
      ls[t] += ls[t + o];
      cs[t] += cs[t + o];
    }
    __syncthreads();
  }
  if (t == 0) {
    if (loss) *loss = y ? ls[0] / float(B) : 0.f;
    if (correct) *correct = cs[0];
  }
}

}  // namespace

bool lstm_shape_ok(int64_t N, int64_t B, int64_t F, int64_t H, int64_t L) {
  return N > 0 && B > 0 && N < (int64_t(1) << 31) - 1 && B < (int64_t(1) << 31) - 1 && F > 0 && F % 4 == 0 &&
         F < (int64_t(1) << 31) && H % 64 == 0 && H >= 64 && H <= 1024 && L >= 1 && L <= kMaxLayers;
}

int seq_finish(const float* loss_row, const int32_t* predw, const int64_t* y, int64_t B, float* loss,
               int32_t* correct, hipStream_t s) {
  if (!loss && !correct) return BGCN_OK;
  hipLaunchKernelGGL(k_lstm_finish, dim3(1), dim3(256), 0, s, loss_row, predw, y, B, loss, correct);
  BGCN_CHECK_LAUNCH();
  return BGCN_OK;
}

int lstm_check_args(const bgcn_lstm_args* a, const void* ws) {
  BGCN_CHECK_ARG(a, "null args");
  BGCN_CHECK_ARG(lstm_shape_ok(a->num_nodes, a->num_seqs, a->in_feats, a->hid, a->num_layers),
                 "unsupported shape (in_feats % 4, hid % 64 in [64, 1024], layers in [1, 4])");
  BGCN_CHECK_ARG(a->out_feats >= 1 && a->out_feats <= kMaxOut, "out_feats must be in [1, 64]");
  BGCN_CHECK_ARG(a->max_len >= 1, "max_len must be at least 1");
  BGCN_CHECK_ARG(a->x && a->seq_start && a->fc_w && a->fc_b && a->logp && a->status, "null pointer");
  BGCN_CHECK_ARG(a->ldx >= a->in_feats && a->ldx % 4 == 0 && a16(a->x), "x rows must be 16-byte aligned (ldx % 4)");
  for (int l = 0; l < a->num_layers; ++l)
    for (int d = 0; d < 2; ++d)
      BGCN_CHECK_ARG(a->w_ih[l][d] && a->w_hh[l][d] && a16(a->w_ih[l][d]) && a16(a->w_hh[l][d]),
                     "null or unaligned LSTM weight");
  BGCN_CHECK_ARG(a16(a->fc_w) && a16(a->out) && a16(ws), "fc_w, out and the workspace must be 16-byte aligned");
  return BGCN_OK;
}

void carve_lstm_fwd(Carve& c, int64_t N, int64_t B, int64_t H, int64_t L, bool save, float* out, LstmFwdWs* w) {
  const size_t n = size_t(N), nb = size_t(B), h = size_t(H);
  for (int l = 0; l < kMaxLayers; ++l) {
    w->G[l] = l >= L ? nullptr : (save || l == 0) ? c.take<float>(n * 8 * h) : w->G[0];
    w->Y[l] = l < L ? c.take<float>(n * 2 * h) : nullptr;
    w->C[l] = l < L && save ? c.take<float>(n * 2 * h) : nullptr;
  }
  if (out) w->Y[L - 1] = out;   // the last layer straight into the caller's [N, 2H]
  w->c = c.take<float>(2 * nb * h);
  w->sq.start = c.take<int32_t>(nb);
  w->sq.len = c.take<int32_t>(nb);
  w->loss_row = c.take<float>(nb);
  w->predw = c.take<int32_t>(nb);
}

int lstm_forward(const bgcn_lstm_args* a, const LstmFwdWs& w, bool save, float* h_n, hipStream_t s) {
  const int64_t N = a->num_nodes, B = a->num_seqs, F = a->in_feats, H = a->hid, L = a->num_layers;
  SetupArgs su{a->seq_start, B, N, a->max_len, w.sq, {w.Y[0], w.Y[1], w.Y[2], w.Y[3]}, int(L), 2 * H, a->status};
  hipLaunchKernelGGL(k_lstm_setup, dim3(64), dim3(256), 0, s, su);
  BGCN_CHECK_LAUNCH();

  const int64_t steps = std::min<int64_t>(a->max_len, N);
  const dim3 grid(unsigned(H / kUnits), 2, grid_for(B, kSeqTile));
  const auto step = save ? k_lstm_step<true> : k_lstm_step<false>;
  for (int l = 0; l < L; ++l) {
    const float* X = l == 0 ? a->x : w.Y[l - 1];
    const int64_t K = l == 0 ? F : 2 * H, ldx = l == 0 ? a->ldx : 2 * H;
    BGCN_TRY(gemm_xwt_impl(X, ldx, a->w_ih[l][0], a->w_ih[l][1], K, 4 * H, w.G[l], 8 * H, N, 8 * H, K, s, nullptr));
    StepArgs st{w.G[l], {a->w_hh[l][0], a->w_hh[l][1]}, w.Y[l], w.c, w.sq, B, int(H), 0, w.C[l]};
    for (int64_t k = 0; k < steps; ++k) {
      st.s = int(k);
      hipLaunchKernelGGL(step, grid, dim3(256), 0, s, st);
    }
    BGCN_CHECK_LAUNCH();
  }

  LstmHeadArgs hd{{w.Y[0], w.Y[1], w.Y[2], w.Y[3]}, w.sq, B, int(H), int(L), int(a->out_feats), a->fc_w, a->fc_b,
                  a->y, a->logp, h_n, w.loss_row, w.predw, a->pred, a->status};
  hipLaunchKernelGGL(k_lstm_head, dim3(unsigned(B)), dim3(256), 0, s, hd);
  BGCN_CHECK_LAUNCH();
  return seq_finish(w.loss_row, w.predw, a->y, B, a->loss, a->correct, s);
}

int lstm_eval_impl(const bgcn_lstm_args* a, void* ws, size_t ws_bytes, hipStream_t s) {
  BGCN_TRY(lstm_check_args(a, ws));
  LstmFwdWs w;
  Carve c(ws, ws_bytes);
  carve_lstm_fwd(c, a->num_nodes, a->num_seqs, a->hid, a->num_layers, false, a->out, &w);
  BGCN_CHECK_ARG(ws && c.ok(), "workspace too small");
  return lstm_forward(a, w, false, a->h_n, s);
}

}  // namespace bgcn

extern "C" size_t bgcn_lstm_workspace_size(int64_t num_nodes, int64_t num_seqs, int64_t in_feats, int64_t hid,
                                           int64_t num_layers) {
  if (!bgcn::lstm_shape_ok(num_nodes, num_seqs, in_feats, hid, num_layers)) return 0;
  bgcn::LstmFwdWs w;
  bgcn::Carve c(nullptr, 0);
  bgcn::carve_lstm_fwd(c, num_nodes, num_seqs, hid, num_layers, false, nullptr, &w);
  return bgcn::align_up(c.off, 256);
}

extern "C" int bgcn_lstm_eval(const bgcn_lstm_args* args, void* workspace, size_t workspace_bytes,
                              bgcn_stream_t stream) {
  return bgcn::lstm_eval_impl(args, workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream));
}
