// bgcn_lstm_eval: the LSTM baseline's test loop body (model/Twitter/LSTM_Twitter.py:146-173) for a
// whole batch of trees as one launch sequence on the caller's stream, everything in the caller's
// workspace.  Each tree is one sequence: the rows [seq_start[b], seq_start[b + 1]) of x (the last
// one runs to N).  nn.LSTM(in, H, num_layers = L, bidirectional, bias = False), h0 = c0 = 0.
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
// live in bgcn_lstm_body.h, shared with the training entry point (bgcn_lstm_train.hip).
#include "bgcn_lstm_body.h"

namespace bgcn {

int lstm_eval_impl(const bgcn_lstm_args* a, void* ws, size_t ws_bytes, hipStream_t s) {
  BGCN_CHECK_ARG(a, "null args");
  const int64_t N = a->num_nodes, B = a->num_seqs, F = a->in_feats, H = a->hid, L = a->num_layers,
                C = a->out_feats;
  BGCN_CHECK_ARG(shape_ok(N, B, F, H, L), "unsupported shape (in_feats % 4, hid % 64 in [64, 1024], layers in [1, 4])");
  BGCN_CHECK_ARG(C >= 1 && C <= kMaxOut, "out_feats must be in [1, 64]");
  BGCN_CHECK_ARG(a->max_len >= 1, "max_len must be at least 1");
  BGCN_CHECK_ARG(a->x && a->seq_start && a->fc_w && a->fc_b && a->logp && a->status, "null pointer");
  BGCN_CHECK_ARG(a->ldx >= F && a->ldx % 4 == 0 && a16(a->x), "x rows must be 16-byte aligned (ldx % 4)");
  for (int l = 0; l < L; ++l)
    for (int d = 0; d < 2; ++d)
      BGCN_CHECK_ARG(a->w_ih[l][d] && a->w_hh[l][d] && a16(a->w_ih[l][d]) && a16(a->w_hh[l][d]),
                     "null or unaligned LSTM weight");
  BGCN_CHECK_ARG(a16(a->fc_w) && a16(a->out) && a16(ws), "fc_w, out and the workspace must be 16-byte aligned");
  LstmWs w;
  Carve c(ws, ws_bytes);
  carve_lstm(c, N, B, H, L, &w);
  BGCN_CHECK_ARG(ws && c.ok(), "workspace too small");
  if (a->out) w.Y[L - 1] = a->out;   // the last layer straight into the caller's [N, 2H]

  SetupArgs su{a->seq_start, B, N, a->max_len, w.sq, {w.Y[0], w.Y[1], w.Y[2], w.Y[3]}, int(L), 2 * H, a->status};
  hipLaunchKernelGGL(k_lstm_setup, dim3(64), dim3(256), 0, s, su);
  BGCN_CHECK_LAUNCH();

  const int64_t steps = std::min<int64_t>(a->max_len, N);
  const dim3 grid(unsigned(H / kUnits), 2, grid_for(B, kSeqTile));
  for (int l = 0; l < L; ++l) {
    const float* X = l == 0 ? a->x : w.Y[l - 1];
    const int64_t K = l == 0 ? F : 2 * H, ldx = l == 0 ? a->ldx : 2 * H;
    BGCN_TRY(gemm_xwt_impl(X, ldx, a->w_ih[l][0], a->w_ih[l][1], K, 4 * H, w.G, 8 * H, N, 8 * H, K, s, nullptr));
    StepArgs st{w.G, {a->w_hh[l][0], a->w_hh[l][1]}, w.Y[l], w.c, w.sq, B, int(H), 0, nullptr};
    for (int64_t k = 0; k < steps; ++k) {
      st.s = int(k);
      hipLaunchKernelGGL(k_lstm_step<false>, grid, dim3(256), 0, s, st);
    }
    BGCN_CHECK_LAUNCH();
  }

  LstmHeadArgs hd{{w.Y[0], w.Y[1], w.Y[2], w.Y[3]}, w.sq, B, int(H), int(L), int(C), a->fc_w, a->fc_b, a->y,
                  a->logp, a->h_n, w.loss_row, w.predw, a->pred, a->status};
  hipLaunchKernelGGL(k_lstm_head, dim3(unsigned(B)), dim3(256), 0, s, hd);
  BGCN_CHECK_LAUNCH();
  if (a->loss || a->correct) {
    hipLaunchKernelGGL(k_lstm_finish, dim3(1), dim3(256), 0, s, w.loss_row, w.predw, a->y, B, a->loss, a->correct);
    BGCN_CHECK_LAUNCH();
  }
  return BGCN_OK;
}

}  // namespace bgcn

extern "C" size_t bgcn_lstm_workspace_size(int64_t num_nodes, int64_t num_seqs, int64_t in_feats, int64_t hid,
                                           int64_t num_layers) {
  if (!bgcn::shape_ok(num_nodes, num_seqs, in_feats, hid, num_layers)) return 0;
  bgcn::LstmWs w;
  bgcn::Carve c(nullptr, 0);
  return bgcn::carve_lstm(c, num_nodes, num_seqs, hid, num_layers, &w);
}

extern "C" int bgcn_lstm_eval(const bgcn_lstm_args* args, void* workspace, size_t workspace_bytes,
                              bgcn_stream_t stream) {
  return bgcn::lstm_eval_impl(args, workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream));
}
