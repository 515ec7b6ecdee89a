/*
 * bgcn.h - C ABI of the MI355X (gfx950) BiGCN message-passing path.
 *
 * This is the drop-in boundary of the build.  The reference reaches the hot path
 * through module-level Python symbols of third-party packages (no plugin system):
 *
 *   from torch_geometric.nn import GCNConv      model/Twitter/BiGCN_Twitter.py:15
 *                                               model/Weibo/BiGCN_Weibo.py:13
 *   from torch_scatter import scatter_mean      model/Twitter/BiGCN_Twitter.py:6
 *                                               model/Weibo/BiGCN_Weibo.py:5
 *
 * called from TDrumorGCN/BUrumorGCN.forward (BiGCN_Twitter.py:42,56,65,92,105,113).
 * Each entry point below names the reference operation it replaces.  The Python
 * mirror (bigcn_amd/) binds these with ctypes; INTEGRATION.md shows the binding a
 * maintainer of the reference would add.
 *
 * Conventions (all entry points):
 *   - every tensor pointer is a DEVICE pointer owned by the caller; the library
 *     never allocates or frees caller memory.  Scratch comes from a caller-provided
 *     workspace whose size is returned by the matching *_workspace_size() call;
 *   - every call is asynchronous on the given stream and performs no host sync.  Global
 *     state: the thread-local error string, the opt-in kernel-timing hook, and two
 *     auxiliary HIP streams ("lanes") per device (each created on first use) that the
 *     fused encoder and train step fork independent branches onto and join back into the
 *     caller's stream (inline on the legacy null stream); bgcn_train_step's next-batch
 *     preparation is waited for by the next call instead (bgcn_join_side);
 *   - return value: 0 = ok, BGCN_EINVAL (-1) = invalid argument / shape,
 *     BGCN_EHIP (-2) = HIP launch error.  bgcn_last_error() gives a thread-local
 *     message.  Data-dependent errors (an edge index outside [0, N)) cannot be
 *     reported synchronously: the offending edge is skipped and *status is set to 1
 *     on the device (the Python layer raises IndexError, like index_select would).
 *   - fp32 everywhere (the reference's dtype); rows are row-major with a leading
 *     dimension ("ld", in elements).
 */
#ifndef BGCN_H_
#define BGCN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* bgcn_stream_t; /* == hipStream_t */

#define BGCN_OK 0
#define BGCN_EINVAL (-1)
#define BGCN_EHIP (-2)

#define BGCN_ABI_VERSION 12

/* Degree convention of gcn_norm: PyG >= 1.6 normalises by TARGET (col) degree,
 * PyG 1.3.2 (the version readme.md:28 pins) by SOURCE (row) degree. */
#define BGCN_DEGREE_ON_COL 0
#define BGCN_DEGREE_ON_ROW 1

/* epilogue flags of bgcn_spmm */
#define BGCN_EPI_NONE 0
#define BGCN_EPI_RELU 1

int bgcn_abi_version(void);
const char* bgcn_last_error(void);

/* --------------------------------------------------------------------------
 * K1  gcn_norm + add_remaining_self_loops + propagate's index preparation.
 * Replaces: torch_geometric GCNConv.forward -> gcn_norm (explicit call form at
 * explain_PHEME.py:62-63), invoked by every GCNConv call of BiGCN_Twitter.py:42,56,92,105.
 *
 * edge_index: int64 [2, E] (row 0 = source, row 1 = target), PyG layout.
 * edge_weight: optional fp32 [E] (NULL = all ones; EBGCN's variant, EBGCN.py:84).
 * Existing self loops are dropped and one loop (i,i) of weight 1 is appended per node.
 * Outputs two CSR views of the normalised adjacency (capacity E + N entries each):
 *   by target  (forward aggregation): t_ptr[N+1], t_row[], t_col[] = source, t_w[]
 *   by source  (backward, A^T)      : s_ptr[N+1], s_row[], s_col[] = target, s_w[]
 * Entries of a row keep edge order with the self loop last, which is the summation
 * order of PyG's scatter-add.  *_row holds the row id of each entry (COO form).
 * Deterministic (no float atomics): counting sort with a run-based placement when each
 * key's edges are contiguous (always true for propagation trees), else an ordered
 * general placement; the choice is made on the device.
 * The number of valid entries is t_ptr[N] (= s_ptr[N]), on the device.
 * -------------------------------------------------------------------------- */
size_t bgcn_graph_workspace_size(int64_t num_edges, int64_t num_nodes);
int bgcn_build_graph(const int64_t* edge_index, const float* edge_weight, int64_t num_edges,
                     int64_t num_nodes, int degree_on,
                     int32_t* t_ptr, int32_t* t_row, int32_t* t_col, float* t_w,
                     int32_t* s_ptr, int32_t* s_row, int32_t* s_col, float* s_w,
                     int32_t* status, void* workspace, size_t workspace_bytes,
                     bgcn_stream_t stream);

/* The D^-1/2 vector (dinv[N], fp32: deg^-1/2 with inf -> 0, the degree including the self
 * loop) a bgcn_build_graph call left in its workspace (valid while that workspace is kept
 * unmodified; same sizes as the build).  Input of bgcn_edge_weight_grad. */
int bgcn_graph_dinv(const void* workspace, size_t workspace_bytes, int64_t num_edges, int64_t num_nodes,
                    const float** dinv);

/* gcn_norm backward: dL/d edge_weight of GCNConv(x, edge_index, edge_weight) - EBGCN learns
 * its edge weights (model/Twitter/EBGCN.py:101-102 edge_pred = sigmoid(fc(...)), passed as
 * GCNConv(..., edge_weight=edge_pred) at :84,178).  Inputs, all [N, ld] fp32 rows of width F
 * (a multiple of 4; pad with zero columns): h = x W^T (the propagate input), agg = A_hat h
 * (the propagate output without the bias), dout = dL/d out, dz = A_hat^T dout; dinv from
 * bgcn_graph_dinv of the graph built from the same edge_index / edge_weight / degree_on.
 * Writes d_edge_weight[E] in edge order: through norm_e = dinv[src] w_e dinv[dst] and through
 * the degree of each node (PyG >= 1.6: target side, 'row': source side); an input self loop
 * receives its node's loop-weight gradient (add_remaining_self_loops); an edge with an index
 * outside [0, N) gets 0.  Deterministic (no float atomics). */
size_t bgcn_edge_weight_grad_workspace_size(int64_t num_nodes);
int bgcn_edge_weight_grad(const int64_t* edge_index, int64_t num_edges, int64_t num_nodes, int degree_on,
                          const float* dinv, const float* h, const float* agg, const float* dout,
                          const float* dz, int64_t ld, int32_t F, float* d_edge_weight, void* workspace,
                          size_t workspace_bytes, bgcn_stream_t stream);

/* Both directions of one batch in one launch sequence (the fused step's TD graph of
 * edge_index and BU graph of BU_edge_index; dataset.py:80-90).  No edge weights.
 * batch (optional, ABI 7): the [N] tree id per node of the collated batch; with it every
 * edge whose ends lie in different trees sets BGCN_STATUS_CROSS_TREE in *status.  PyG
 * collation never makes such an edge, and the fused encoder's fast readout backward
 * (tree-scaled sign-word aggregation) needs to know that; the status word then travels
 * with the graphs (bgcn_graph_view.tree_status) and a set bit switches that aggregation to
 * per-neighbour tree scales (same result as k_readout_bwd + the plain aggregation). */
#define BGCN_STATUS_CROSS_TREE 16
typedef struct bgcn_csr_out {
  int32_t* t_ptr; int32_t* t_row; int32_t* t_col; float* t_w;
  int32_t* s_ptr; int32_t* s_row; int32_t* s_col; float* s_w;
} bgcn_csr_out;
size_t bgcn_graph_pair_workspace_size(int64_t td_num_edges, int64_t bu_num_edges, int64_t num_nodes);
int bgcn_build_graph_pair(const int64_t* td_edge_index, int64_t td_num_edges,
                          const int64_t* bu_edge_index, int64_t bu_num_edges, int64_t num_nodes,
                          int degree_on, const bgcn_csr_out* td, const bgcn_csr_out* bu,
                          const int64_t* batch, int32_t* status, void* workspace,
                          size_t workspace_bytes, bgcn_stream_t stream);

/* --------------------------------------------------------------------------
 * K3/K4  MessagePassing.propagate(aggr='add') with message norm * x_j, + bias.
 * Replaces: the gather x[row] * norm + scatter_add to col inside GCNConv
 * (forward, CSR by target) and its autograd backward (CSR by source).
 * out[r, :F] = epi( sum_{p in row r} w[p] * in[col[p], :F]  (+ bias) )
 * Atomic-free and deterministic: the nnz range is split evenly over lane groups
 * (merge path) and rows that cross a split are combined in a fixed order.
 * `capacity` = allocated entries (E + N); entries [ptr[rows], capacity) must carry
 * row = -1 (bgcn_build_graph writes them), so the kernels never wait on the count.
 * F: a positive multiple of 4 (64 and 128 take the narrow kernels).
 * -------------------------------------------------------------------------- */
size_t bgcn_spmm_workspace_size(int64_t capacity, int32_t F);
int bgcn_spmm(const int32_t* ptr, const int32_t* row, const int32_t* col, const float* w,
              int64_t rows, int64_t capacity, const float* in, int64_t ld_in, float* out,
              int64_t ld_out, int32_t F, const float* bias, int epilogue,
              void* workspace, size_t workspace_bytes, bgcn_stream_t stream);

/* --------------------------------------------------------------------------
 * K2  GCNConv.lin: Y[M, Nc] = X[M, K] * W[Nc, K]^T  (fp32 in, fp32 MFMA accumulate).
 * Replaces: torch.nn.functional.linear / aten mm inside GCNConv (lin before propagate).
 * W rows [0, split) come from W0, rows [split, Nc) from W1 (lets TD and BU conv1
 * share one pass over X: Nc = 128, split = 64).  W1 may be NULL if split >= Nc.
 * -------------------------------------------------------------------------- */
int bgcn_gemm_xwt(const float* X, int64_t ldx, const float* W0, const float* W1, int64_t ldw,
                  int64_t split, float* Y, int64_t ldy, int64_t M, int64_t Nc, int64_t K,
                  bgcn_stream_t stream);

/* Input gradient of GCNConv.lin: Y[M, Nc] = X[M, K] * W[K, Nc]  (dX = dZ * W).
 * Replaces: the autograd backward of F.linear w.r.t. its input inside GCNConv. */
int bgcn_gemm_xw(const float* X, int64_t ldx, const float* W, int64_t ldw, float* Y, int64_t ldy,
                 int64_t M, int64_t Nc, int64_t K, bgcn_stream_t stream);

/* Column sums out[c] = sum_r A[r, c] (bias gradient of GCNConv; deterministic). */
size_t bgcn_colsum_workspace_size(int64_t rows, int32_t C);
int bgcn_colsum(const float* A, int64_t lda, int64_t rows, int32_t C, float* out,
                void* workspace, size_t workspace_bytes, bgcn_stream_t stream);

/* --------------------------------------------------------------------------
 * K10  weight gradient of GCNConv.lin: C[Mc, Nc] = G[K, Mc]^T * X[K, Nc]
 * (reduction over the K = node dimension, split over node chunks with partial
 * slabs in the workspace and a fixed-order reduction: deterministic).
 * Output rows [0, split) go to C0 (ld ldc), rows [split, Mc) to C1.
 * -------------------------------------------------------------------------- */
size_t bgcn_gemm_tn_workspace_size(int64_t Mc, int64_t Nc, int64_t K);
int bgcn_gemm_tn(const float* G, int64_t ldg, const float* X, int64_t ldx, float* C0, float* C1,
                 int64_t ldc, int64_t split, int64_t Mc, int64_t Nc, int64_t K,
                 void* workspace, size_t workspace_bytes, bgcn_stream_t stream);

/* --------------------------------------------------------------------------
 * K8  torch_scatter.scatter_mean(src, index, dim=0, dim_size=B)  (fwd and bwd).
 * Replaces: scatter_mean at BiGCN_Twitter.py:65,113 / BiGCN_Weibo.py:43,73.
 * index: int64 [n] (any order; values outside [0,B) are ignored and flag *status).
 * count[B] receives max(count, 1) as fp32 (saved for backward).  A sorted index
 * (PyG's batch vector) takes a deterministic segmented path, any other order a
 * float-atomic path; the choice is made on the device (no host sync).
 * -------------------------------------------------------------------------- */
size_t bgcn_scatter_mean_workspace_size(int64_t B);
int bgcn_scatter_mean_fwd(const float* src, int64_t ld_src, const int64_t* index, int64_t n,
                          int32_t C, int64_t B, float* out, int64_t ld_out, float* count,
                          int32_t* status, void* workspace, size_t workspace_bytes,
                          bgcn_stream_t stream);
int bgcn_scatter_mean_bwd(const float* dout, int64_t ld_dout, const int64_t* index,
                          const float* count, int64_t n, int32_t C, int64_t B, float* dsrc,
                          int64_t ld_dsrc, bgcn_stream_t stream);

/* --------------------------------------------------------------------------
 * K9  the classifier head: x = self.fc(x); x = F.log_softmax(x, dim=1)
 * Replaces: BiGCN_Twitter.py:129-130 / BiGCN_Weibo.py:87-88 (torch.nn.Linear(256, C) +
 * log_softmax, and their autograd backward) on the per-op path.
 * head_in [B, 256] = cat(BU_x, TD_x); fc_w [C, 256], fc_b [C] (the Linear's layout);
 * logp [B, C]; 0 < C <= 16; head_in, fc_w and dhead_in 16-byte aligned.
 * The backward takes any dlogp [B, C] (the gradient of whatever loss follows) and writes
 * dhead_in [B, 256], fc_dw [C, 256], fc_db [C] (sums over the trees in index order).
 * -------------------------------------------------------------------------- */
int bgcn_head_forward(const float* head_in, const float* fc_w, const float* fc_b, int64_t num_graphs,
                      int32_t num_classes, float* logp, bgcn_stream_t stream);
int bgcn_head_backward(const float* head_in, const float* logp, const float* dlogp, const float* fc_w,
                       int64_t num_graphs, int32_t num_classes, float* dhead_in, float* fc_dw,
                       float* fc_db, bgcn_stream_t stream);

/* --------------------------------------------------------------------------
 * EBGCN (model/Twitter/EBGCN.py), eval mode: the two operations it adds over BiGCN.  Everything
 * else of its forward is the entry points above (conv1, bgcn_build_graph with edge_weight =
 * edge_pred + bgcn_spmm for conv2's aggregation, bgcn_scatter_mean_fwd, bgcn_head_forward).
 * Additive entry points: BGCN_ABI_VERSION is unchanged.
 *
 * bgcn_bn_fold: an eval-mode BatchNorm1d as one multiply-add per channel,
 *   g = gamma / sqrt(running_var + eps),  t = beta - running_mean * g      (y = g x + t).
 *
 * bgcn_edge_infer: edge_pred of TDrumorGCN.edge_infer / BUrumorGCN.edge_infer (EBGCN.py:95-116,
 * :189-212) without the Bayesian branch (its only product, the KL edge loss, is dropped by the
 * evaluation loop, :338).  h [N, 64] (ld ldh) = conv1's output; edge_index int64 [2, E];
 * conv_w [64, 64] = sim_valconv0.weight; (bn_g, bn_t) [64] = sim_valnorm0 folded by bgcn_bn_fold;
 * out_w [64], out_b [1] = sim_valconv_out; fc1_w [edge_num, 64]; edge_pred [E].
 * Per edge e, with a = h[(row_e - 1) mod N] and b = h[(col_e - 1) mod N] - the reference's
 * `x[row - 1]` as written: ids are read one lower than the edge list says and id 0 reads the
 * LAST node - :
 *   D[c][l] = |a[c] - b[l]|;  Y = conv_w D;  Z = leaky_relu(bn_g[o] Y[o][l] + bn_t[o], 0.01);
 *   s[l] = sum_o out_w[o] Z[o][l] + out_b;  edge_pred[e] = mean_k sigmoid(sum_l fc1_w[k][l] s[l]).
 * The 64 x 64 x 64 product per edge runs on the fp32 MFMA with D generated in registers (about
 * 512 B read and 4 B written per edge); one workgroup takes BGCN_EDGE_INFER_TILE edges.
 * Deterministic, no workspace.  hid must be 64 and 1 <= edge_num <= 8 (else BGCN_EINVAL).  An
 * edge with an end outside [0, N) reads nothing, gets edge_pred 0 and sets *status to 1.
 *
 * bgcn_ebgcn_conv2_lin: conv2's lin over relu(bn1(cat(h1, x[root of the node's tree])))
 * (EBGCN.py:72-84; no dropout, as in the reference's EBGCN forward):
 *   z2[i] = relu(g_h . h1[i] + t_h) W2[:, :64]^T + r[batch[i]]
 *   r[b]  = relu(g_x . x[rootindex[b]] + t_x) W2[:, 64:]^T      (once per tree, not per node)
 * (bn_g, bn_t) [64 + F] = bn1 folded, g_h / g_x its first 64 / last F channels; both NULL = bn1
 * skipped (the reference's one-node batch, :80).  w2 [64, 64 + F] = conv2.lin.weight; x [N, F]
 * fp32; z2 [N, 64].  hid must be 64 and F a multiple of 4 (else BGCN_EINVAL).  A rootindex
 * outside [0, N) or a batch id outside [0, B) contributes zeros and sets *status to 1.
 * -------------------------------------------------------------------------- */
#define BGCN_EDGE_INFER_TILE 32
int bgcn_bn_fold(const float* gamma, const float* beta, const float* running_mean,
                 const float* running_var, float eps, int64_t channels, float* g, float* t,
                 bgcn_stream_t stream);
int bgcn_edge_infer(const float* h, int64_t ldh, int64_t num_nodes, int64_t hid,
                    const int64_t* edge_index, int64_t num_edges, const float* conv_w,
                    const float* bn_g, const float* bn_t, const float* out_w, const float* out_b,
                    const float* fc1_w, int32_t edge_num, float* edge_pred, int32_t* status,
                    bgcn_stream_t stream);
size_t bgcn_ebgcn_conv2_lin_workspace_size(int64_t num_nodes, int64_t num_graphs, int64_t in_feats);
int bgcn_ebgcn_conv2_lin(const float* h1, int64_t ldh, const float* x, int64_t ldx,
                         const int64_t* batch, const int64_t* rootindex, int64_t num_nodes,
                         int64_t num_graphs, int64_t in_feats, int64_t hid, const float* w2,
                         const float* bn_g, const float* bn_t, float* z2, int64_t ldz, int32_t* status,
                         void* workspace, size_t workspace_bytes, bgcn_stream_t stream);

/* --------------------------------------------------------------------------
 * Explain (explain_PHEME.py:91-242, :530-533), inference only: after every stage of a direction
 * each node's activation row is summed to one number and the nodes of a tree are ranked by it.
 * Additive entry points: BGCN_ABI_VERSION is unchanged.
 *
 * bgcn_explain_sums: the per-node stage sums of one direction, sums [S, num_nodes] (row stride
 * ld_sums), stage-major.  h1 [N, 64] = conv1's output, h2 [N, 64] = conv2's output BEFORE its
 * relu, x [N, F] fp32; (bn_g, bn_t) [64 + F] = bn1 folded by bgcn_bn_fold (g_h / g_x its first
 * 64 / last F channels), both NULL = the BiGCN stage list.  With r = rootindex[batch[n]]:
 *   S = 5 (BiGCN)                              S = 6 (EBGCN)
 *   0 sum h1[n]                                0 sum h1[n]
 *   1 sum h1[n] + sum x[r]                     1 sum h1[n] + sum x[r]
 *   2 sum relu(h1[n]) + sum relu(x[r])         2 sum (g_h h1[n] + t_h) + sum (g_x x[r] + t_x)
 *   3 sum h2[n]                                3 sum relu(g_h h1[n] + t_h) + sum relu(g_x x[r] + t_x)
 *   4 sum relu(h2[n]) + sum h1[r]              4 sum h2[n]
 *                                              5 sum relu(h2[n]) + sum h1[r]
 * (the reference's conv1_output_sum, conv1_output_cat_x_sum, [conv1_output_cat_x_bn1_sum,]
 * conv2_input_sum, conv2_output_sum, scatter_mean_input_sum; eval-mode dropout is the identity).
 * No concat is materialised and every root term is computed once per tree.  x_sum [N] (optional,
 * NULL = skip) receives sum_f x[n][f]: the one pass over all of X, one wave per row with 16-byte
 * streaming loads.  Deterministic (fixed summation order, no float atomics).  hid must be 64 and
 * F a multiple of 4 (else BGCN_EINVAL).  A rootindex outside [0, N) or a batch id outside [0, B)
 * is not read, contributes zeros and sets *status bit 0.
 *
 * bgcn_segment_rank: torch.topk(values, k = n) per tree and stage.  values [S, N] fp32 (row
 * stride ld); batch int64 [N], the PyG batch vector (non-decreasing; tree ids without nodes are
 * fine); order int32 [S, N] and sorted fp32 [S, N] (row stride N).  Tree t's slots are its node
 * range: order holds the tree's LOCAL node indices (node id minus the tree's first node) by
 * descending value, sorted the values in that order (bit copies).  The order is total: equal
 * values by ascending node index, -0.0 equal to +0.0, every NaN above +inf (as torch) and NaNs
 * among themselves by ascending index.  Segment bounds are derived on the device.  A segment of
 * at most BGCN_SEGMENT_RANK_LDS nodes is sorted in LDS by one workgroup per (stage, tree); longer
 * ones are ranked by counting through global memory (O(n^2) compares, any length).
 * Deterministic.  A batch vector that decreases anywhere, or holds an id outside [0, B), sets
 * *status bit 0; the outputs are then left unwritten.
 * -------------------------------------------------------------------------- */
#define BGCN_SEGMENT_RANK_LDS 4096
size_t bgcn_explain_sums_workspace_size(int64_t num_graphs);
int bgcn_explain_sums(const float* h1, int64_t ldh1, const float* h2, int64_t ldh2, const float* x,
                      int64_t ldx, const int64_t* batch, const int64_t* rootindex, int64_t num_nodes,
                      int64_t num_graphs, int64_t in_feats, int64_t hid, const float* bn_g,
                      const float* bn_t, float* sums, int64_t ld_sums, float* x_sum, int32_t* status,
                      void* workspace, size_t workspace_bytes, bgcn_stream_t stream);
size_t bgcn_segment_rank_workspace_size(int64_t num_graphs);
int bgcn_segment_rank(const float* values, int64_t ld, int64_t num_stages, const int64_t* batch,
                      int64_t num_nodes, int64_t num_graphs, int32_t* order, float* sorted,
                      int32_t* status, void* workspace, size_t workspace_bytes, bgcn_stream_t stream);

/* --------------------------------------------------------------------------
 * Compare (compare_similarity.py:38-183): the reference scores, per tree, every pair of node
 * rankings - by three graph centralities and by the models' stage sums - with five statistics
 * over the rankings' first k entries.  Additive entry points: BGCN_ABI_VERSION is unchanged.
 *
 * bgcn_tree_centrality: cent [3, num_nodes] fp32 (row stride ld), rows out_degree, betweenness,
 * closeness (the reference's order), of the top-down edge list edge_index int64 [2, num_edges]
 * (parent -> child, global node ids, any edge order) and the PyG batch vector.  The script that
 * wrote the reference's centrality files is not part of it; the definition taken here is
 * networkx's out_degree_centrality, betweenness_centrality and closeness_centrality on the
 * DiGraph of a tree's edges with default arguments, which for a tree of n nodes and a node of c
 * children, depth d and subtree size s (itself included) are
 *   out_degree = c / (n - 1) (1 when n = 1)     betweenness = d (s - 1) / ((n - 1)(n - 2)) (0 when
 *   n <= 2)     closeness = 2 d / ((d + 1)(n - 1)) (0 when d = 0).
 * c, d, s, n are computed exactly in integers; each value is one fp64 division rounded once to
 * fp32, so nodes with equal (c, d, s) get bit-equal values and bgcn_segment_rank's tie rule
 * (ascending node index) decides between them.  One workgroup per tree: depths and subtree sizes
 * by pointer jumping (ceil(log2 n) rounds, integer atomics only), in LDS for a tree of at most
 * BGCN_TREE_CENTRALITY_LDS nodes, on a workspace slice for a longer one.  Deterministic.
 * A forest is accepted (a DropEdge'd list: several parentless nodes per tree; depth and subtree
 * size are then per component, n stays the tree's node count), as are tree ids without nodes.
 * Refused, with *status bit 0 set and the tree's outputs left unwritten: a second incoming edge
 * on a node (also BGCN_STATUS_TWO_PARENTS), an edge that leaves its tree (also
 * BGCN_STATUS_CROSS_TREE; both trees), a cycle (also BGCN_STATUS_CYCLE), an endpoint outside
 * [0, N) (the other endpoint's tree).  A batch vector that decreases, or holds an id outside
 * [0, B), sets bit 0 and nothing is written.
 *
 * bgcn_rank_similarity: orders int32 [num_lists, num_nodes] (row stride ld) are rankings as
 * bgcn_segment_rank writes them (per tree: local node indices, best first); num_lists in [1, 32]
 * and k in [2, 32] (BGCN_RANK_SIMILARITY_MAX), else BGCN_EINVAL; at most 2^26 nodes (the sums are
 * exact in int64).  sim fp64 [B, 5, num_lists, num_lists], valid int32 [B].  A tree of n <= k nodes
 * gets zeros and valid 0 (the reference's `continue`).  Otherwise valid is 1 and for lists i, j,
 * x and y their first k entries:
 *   0 Pearson r of x and y as numbers     1 Spearman rho (Pearson of the entries' ranks inside
 *   their list)     2 Kendall tau     3 Somers' D     4 Jaccard of the two index sets.
 * The lists hold k distinct indices, so no ties: tau-b = tau-a = D.  Every sum is an exact int64;
 * each value is one fp64 division (after one sqrt for 0 and 1), so 2-4 are exact rationals
 * rounded once and the matrix is symmetric bit for bit.  A list that repeats an index, or holds
 * one outside [0, n), inside its first k is not a ranking: *status bit 1 is set, the tree's block
 * is NaN and valid 0.  One workgroup per tree.  Deterministic.
 * -------------------------------------------------------------------------- */
#define BGCN_TREE_CENTRALITY_LDS 2048
#define BGCN_RANK_SIMILARITY_MAX 32
#define BGCN_STATUS_TWO_PARENTS 32
#define BGCN_STATUS_CYCLE 64
size_t bgcn_tree_centrality_workspace_size(int64_t num_nodes, int64_t num_graphs);
int bgcn_tree_centrality(const int64_t* edge_index, int64_t num_edges, const int64_t* batch,
                         int64_t num_nodes, int64_t num_graphs, float* cent, int64_t ld, int32_t* status,
                         void* workspace, size_t workspace_bytes, bgcn_stream_t stream);
size_t bgcn_rank_similarity_workspace_size(int64_t num_graphs);
int bgcn_rank_similarity(const int32_t* orders, int64_t ld, int64_t num_lists, const int64_t* batch,
                         int64_t num_nodes, int64_t num_graphs, int32_t k, double* sim, int32_t* valid,
                         int32_t* status, void* workspace, size_t workspace_bytes, bgcn_stream_t stream);

/* --------------------------------------------------------------------------
 * The confusion matrix every number of the reference's validation loop derives from
 * (tools/evaluate.py:3-139 called at BiGCN_Twitter.py:223; explain_PHEME.py:480,609 keeps the
 * matrix itself): counts[a * C + p] = #{i : y[i] == a && pred[i] == p}, int32, row = actual,
 * column = predicted.  pred, y: int64 [B], any B >= 0; num_classes C in [1, 16].
 * One launch: accumulate == 0 overwrites all C * C bins (zeros for B == 0; no zeroing launch or
 * memset is needed before the call), accumulate != 0 adds to them (B == 0: counts untouched).
 * Integer arithmetic: exact and the same on every run.  An entry whose pred or y lies outside
 * [0, C) is not counted and sets bit 0 of *status.  BGCN_EINVAL before any device work for a
 * null pred, y, counts or status, num_classes outside [1, 16], B < 0. */
int bgcn_confusion(const int64_t* pred, const int64_t* y, int64_t B, int num_classes, int32_t* counts,
                   int accumulate, int32_t* status, bgcn_stream_t stream);

/* --------------------------------------------------------------------------
 * DropEdge (Process/dataset.py:68-90): per tree, keep a uniform random subset of
 * exactly int(E_t * (1 - droprate)) edges (count computed in double as Python does),
 * in their original order; droprate <= 0 keeps every edge (the reference's
 * `if droprate > 0`).  TD (list 0) and BU (list 1) are drawn independently; either
 * list may be NULL.  The draw is a counter-based function of (seed, list, edge
 * position) instead of Python's `random.sample`; same distribution, different stream.
 * Lists: int64 [2, E] (row stride E) in PyG collation order - each tree's edges
 * contiguous, trees ascending; tree of an edge = batch[src].
 *   masked = 0: the kept edges, compacted in order, into out [2, ld] (ld = row stride);
 *               counts[0..1] (device, optional) receive the kept totals.  ld below the
 *               total sets *status bit 0 and the excess is not written.
 *   masked = 1: out [2, ld >= E]; within each tree's range its kept edges first (in
 *               order), then every dropped edge (s, d) as the self loop (d, d).
 *               bgcn_build_graph removes input self loops, so the (unweighted) graph
 *               equals that of the compacted list and no kept count is needed.
 * An edge out of range, crossing trees or out of tree order sets *status bit 0.
 * -------------------------------------------------------------------------- */
size_t bgcn_drop_edges_workspace_size(int64_t num_graphs);
int bgcn_drop_edges(const int64_t* td_edge_index, int64_t td_num_edges, double td_droprate,
                    int64_t* td_out, int64_t ld_td_out, const int64_t* bu_edge_index,
                    int64_t bu_num_edges, double bu_droprate, int64_t* bu_out, int64_t ld_bu_out,
                    const int64_t* batch, int64_t num_nodes, int64_t num_graphs, uint64_t seed,
                    int32_t masked, int64_t* counts, int32_t* status, void* workspace,
                    size_t workspace_bytes, bgcn_stream_t stream);

/* --------------------------------------------------------------------------
 * Fused bidirectional BiGCN encoder: TDrumorGCN + BUrumorGCN forward/backward
 * (BiGCN_Twitter.py:26-67 and :77-114, Weibo :22-44 / :52-74), producing the
 * head input cat(BU_x, TD_x) [B, 256] of BiGCN.forward (:126-128).
 * The fc / log_softmax / nll head (:129-130, :184) stays in PyTorch.
 *
 * Internal layout: per-node matrices are [N, 2*H] with TD in columns [0, H) and
 * BU in [H, 2H).  Dropout (F.dropout p = 0.5 over the [N, H+F] concat, :54) keep
 * bits are either generated in-kernel from (seed, direction, node, word) or read
 * from an injected bitmask keep_words[2][N][nw], nw = ceil((H+F)/32),
 * bit j of word w = column 32w + j; set bit = keep (x2).
 * -------------------------------------------------------------------------- */
/* The aggregation plan of one CSR orientation (chunk bounds + the list of long rows),
 * written by the graph builders into their workspace; all NULL = no plan. */
typedef struct bgcn_spmm_plan {
  const void* bnd; const int32_t* longs; const int32_t* nlong;
} bgcn_spmm_plan;

typedef struct bgcn_graph_view {
  const int32_t* t_ptr; const int32_t* t_row; const int32_t* t_col; const float* t_w;
  const int32_t* s_ptr; const int32_t* s_row; const int32_t* s_col; const float* s_w;
  int64_t capacity; /* E + N */
  /* optional (ABI 6): the plans of the forward (by target) and backward (by source)
   * aggregations, from bgcn_graph_pair_plans; zeros = merge-path chunks + fix-up */
  bgcn_spmm_plan plan[2];
  /* optional (ABI 7): the status word of a bgcn_build_graph_pair call made WITH its batch
   * argument (BGCN_STATUS_CROSS_TREE tells whether an edge crosses trees).  The fused
   * encoder takes its sign-word readout backward only when both views carry it (or the
   * batch was prepared by bgcn_prepare_batch); NULL keeps k_readout_bwd. */
  const int32_t* tree_status;
} bgcn_graph_view;

/* The aggregation plans a bgcn_build_graph_pair call left in its workspace (valid while
 * that workspace is kept unmodified; same sizes as the build): plan[0] = forward
 * aggregation (rows = targets), plan[1] = backward (rows = sources), per direction.  A
 * bgcn_graph_view carrying them lets the fused encoder take the planned aggregation
 * (complete rows per chunk, one launch, no fix-up) and the sign-word readout backward,
 * as bgcn_train_step does with its prepared batch. */
int bgcn_graph_pair_plans(const void* workspace, size_t workspace_bytes, int64_t td_num_edges,
                          int64_t bu_num_edges, int64_t num_nodes, bgcn_spmm_plan td[2],
                          bgcn_spmm_plan bu[2]);

/* Feature path of the fused encoder.  AUTO: X is read once and every row compacted to a
 * list of its (col, val) non-zeros: the first BGCN_SPARSE_CAP in an ELL list, the rest of
 * a longer row spilled to a per-batch pool of BGCN_SPARSE_SPILL_PER_ROW entries per row of
 * capacity (the words of a post are not capped, Process/getTwittergraph.py:16-24);
 * products with X / X[root] then skip the zero entries (exact: bag-of-words rows hold
 * ~10-20 non-zeros of 5000).  Only when a batch's spilled entries exceed the pool
 * (more than N * (BGCN_SPARSE_CAP + BGCN_SPARSE_SPILL_PER_ROW) non-zeros in all) does the
 * batch fall back to the dense MFMA kernels on the device (no host sync).
 * DENSE: always the dense MFMA kernels.
 * SPARSE: the AUTO path without the dense fallback - the caller guarantees the batch fits
 * the pool (e.g. known from the sparse source features); the gated dense kernels are then
 * not launched at all (shorter step).  A batch that does not fit makes the results
 * invalid and sets bit 2 of the step's *status. */
#define BGCN_FEAT_AUTO 0
#define BGCN_FEAT_DENSE 1
#define BGCN_FEAT_SPARSE 2
/* element type of the node features x (x_dtype): fp32, or bfloat16 (the bf16
 * configuration; bag-of-words counts are exact in bf16, every product accumulates in
 * fp32, so results equal the fp32 path's on the same values) */
#define BGCN_DTYPE_F32 0
#define BGCN_DTYPE_BF16 1
#define BGCN_SPARSE_CAP 32
#define BGCN_SPARSE_SPILL_PER_ROW 32

typedef struct bgcn_bigcn_args {
  /* batch */
  const void* x; int64_t ldx;    /* [N, F] node features (data.x), x_dtype  */
  int64_t num_nodes;             /* N                                       */
  int64_t num_graphs;            /* B                                       */
  int64_t in_feats;              /* F (5000 Twitter/Weibo BoW)              */
  int64_t hid;                   /* H = out_feats = 64                      */
  const int64_t* batch;          /* [N] sorted tree id per node             */
  const int64_t* rootindex;      /* [B] GLOBAL root node ids (PyG collate)  */
  bgcn_graph_view td, bu;        /* graphs of edge_index / BU_edge_index    */
  /* parameters, reference state_dict layout */
  const float* td_w1; const float* td_b1; const float* td_w2; const float* td_b2;
  const float* bu_w1; const float* bu_b1; const float* bu_w2; const float* bu_b2;
  /* dropout */
  int training; uint64_t seed; const uint32_t* keep_words; /* NULL = generate */
  /* feature path (AUTO needs the four buffers below; they are saved for backward) */
  int feat_mode;
  int32_t* x_flags;              /* [8] ([0] != 0: spill pool full -> dense;
                                    [1] spill pool fill)                    */
  int32_t* x_nnz;                /* [N]                                     */
  int32_t* x_cols;               /* [N][BGCN_SPARSE_CAP]                    */
  float* x_vals;                 /* [N][BGCN_SPARSE_CAP]                    */
  /* saved activations (caller-owned, kept for backward) */
  int32_t* tree_ptr;             /* [B+1]                                   */
  float* h1;                     /* [N, 2H] conv1 outputs (pre-relu)        */
  float* h2;                     /* [N, 2H] conv2 outputs (pre-relu)        */
  /* forward output */
  float* head_in;                /* [B, 4H] = cat(BU_x, TD_x)              */
  /* backward input / outputs */
  const float* dhead_in;         /* [B, 4H]                                 */
  float* td_dw1; float* td_db1; float* td_dw2; float* td_db2;
  float* bu_dw1; float* bu_db1; float* bu_dw2; float* bu_db2;
  /* 1: a backward will follow - the forward also builds backward-only state (the CSC
   * of X for dW1) on the library's auxiliary stream, overlapped with the forward */
  int32_t save_for_backward;
  int32_t x_dtype;               /* BGCN_DTYPE_F32 (0) / BGCN_DTYPE_BF16    */
  /* optional (ABI 11): the batch already prepared by bgcn_prepare_batch (same x, batch,
   * rootindex and edge lists, no DropEdge rates, the same degree_on and feat_mode), e.g.
   * by a data pipeline on another stream while the previous batch trained.  The forward
   * then takes the graphs, tree pointers, tree items and the ELL / CSC of X from it instead
   * of building them: td, bu, x_flags .. x_vals and tree_ptr are ignored (may be zero).
   * The work that produced it must be ordered before the forward on `stream`, and the
   * buffer kept unmodified until the backward has run.  NULL: the forward builds them. */
  const void* prepared; size_t prepared_bytes;
  int64_t td_num_edges, bu_num_edges;   /* the prepared batch's edge counts (its layout) */
} bgcn_bigcn_args;

/* The workspace carries state from the forward to the backward (node -> root map,
 * tree work items, root keep masks, CSC of X): pass the backward the SAME workspace,
 * unmodified, and the same args as the forward (plus dhead_in and the gradient
 * pointers).  Both calls may use the library's per-device auxiliary stream for
 * independent branches; every branch is joined back into `stream` before the call's
 * work on `stream` ends, so the caller sees ordinary single-stream semantics. */
size_t bgcn_bigcn_workspace_size(int64_t num_nodes, int64_t num_graphs, int64_t in_feats,
                                 int64_t hid);
int bgcn_bigcn_forward(const bgcn_bigcn_args* args, void* workspace, size_t workspace_bytes,
                       bgcn_stream_t stream);
int bgcn_bigcn_backward(const bgcn_bigcn_args* args, void* workspace, size_t workspace_bytes,
                        bgcn_stream_t stream);

/* --------------------------------------------------------------------------
 * Batch preparation: everything about a batch that does not depend on the weights -
 * K1 (gcn_norm + CSR, both orientations) for TD and BU, tree pointers, node -> root map,
 * tree work items, the ELL compaction of X (BGCN_FEAT_AUTO) and the CSC of X - into a
 * caller-owned "prepared" buffer (size from bgcn_prepare_workspace_size).
 * bgcn_train_step can prepare the NEXT batch on its auxiliary lane while it trains on
 * the current one (the HBM-bound pass over X then overlaps the latency-bound chain).
 * -------------------------------------------------------------------------- */
typedef struct bgcn_batch {
  const void* x; int64_t ldx;    /* [N, F] node features (x_dtype below)     */
  int64_t num_nodes;             /* N                                        */
  int64_t num_graphs;            /* B                                        */
  const int64_t* batch;          /* [N] sorted tree id per node              */
  const int64_t* rootindex;      /* [B] global root node ids                 */
  const int64_t* td_edge_index; int64_t td_num_edges;   /* [2, E_td]         */
  const int64_t* bu_edge_index; int64_t bu_num_edges;   /* [2, E_bu]         */
  /* DropEdge on the device (optional; zero = off): when a rate is > 0 the lists above
   * are the undropped ones and preparation draws the kept subsets itself
   * (bgcn_drop_edges, masked form) from drop_seed before building the graphs. */
  double td_droprate, bu_droprate;
  uint64_t drop_seed;
  int32_t x_dtype;               /* BGCN_DTYPE_F32 (0) / BGCN_DTYPE_BF16      */
  /* Compacted node features (ABI 7; the host-fed input path): with x == NULL the features
   * arrive as the CSR of their non-zeros, the form DataLoader workers emit from the
   * per-tree npz rows (Process/dataset.py:94 x, getTwittergraph.py:67-72 word counts)
   * so that a batch crosses PCIe as ~4 MB instead of N x 20 KB:
   *   x_row_ptr [N + 1]  entries of node i are [x_row_ptr[i], x_row_ptr[i + 1])
   *   x_col [nnz]        column ids in [0, in_feats), strictly ascending within a row
   *   x_val [nnz]        the non-zero values (fp32; zeros must be left out)
   * Preparation then fills the ELL / spill pool / CSC of X from these lists instead of
   * reading X (identical contents, so a step computes the same bits as from the dense x),
   * and the step must run BGCN_FEAT_SPARSE: the caller has checked that the batch fits the
   * pool (sum over rows of max(nnz - BGCN_SPARSE_CAP, 0) <= N * BGCN_SPARSE_SPILL_PER_ROW;
   * otherwise expand it with bgcn_csr_to_dense and pass the dense x).  ldx = in_feats. */
  const int32_t* x_row_ptr; const int32_t* x_col; const float* x_val;
} bgcn_batch;

/* Expand a CSR of node features (bgcn_batch.x_row_ptr / x_col / x_val) into the dense
 * [N, ldx] matrix x of x_dtype (the reference's data.x layout, Process/dataset.py:94):
 * zeros everywhere else.  The host-fed path's fallback for a batch whose rows overflow the
 * sparse path's pool.  Column ids outside [0, F) set *status bit 0 and are skipped. */
int bgcn_csr_to_dense(const int32_t* x_row_ptr, const int32_t* x_col, const float* x_val, int64_t num_nodes,
                      int64_t in_feats, void* x, int64_t ldx, int32_t x_dtype, int32_t* status,
                      bgcn_stream_t stream);

size_t bgcn_prepare_workspace_size(int64_t num_nodes, int64_t num_graphs, int64_t in_feats,
                                   int64_t td_num_edges, int64_t bu_num_edges);
/* feat_mode: BGCN_FEAT_AUTO / _SPARSE build the ELL/CSC of X, BGCN_FEAT_DENSE skips them.
 * A bad edge index sets bit 0 of the buffer's status word (reported by the step). */
int bgcn_prepare_batch(const bgcn_batch* batch, int64_t in_feats, int32_t degree_on,
                       int32_t feat_mode, void* prepared, size_t prepared_bytes,
                       bgcn_stream_t stream);

/* --------------------------------------------------------------------------
 * One training step up to the optimiser, as ONE call (the loop body of
 * BiGCN_Twitter.py:183-188): the fused encoder forward on a prepared batch, the head
 * fc -> log_softmax (:129-130) and nll_loss mean (:186), and the complete backward.
 * Every gradient is WRITTEN (not accumulated), so grads[] may point into a flat
 * data-parallel bucket; the all-reduce and bgcn_adam_step follow.  Parameter order:
 * td_w1 td_b1 td_w2 td_b2 bu_w1 bu_b1 bu_w2 bu_b2 fc_w [C, 256] fc_b [C] (the
 * reference state_dict layout).  *status (optional, zeroed by the call): bit 0 = an
 * edge index outside [0, N) or a batch id outside [0, B) (or, host-fed features, a row of
 * x_col with a column outside [0, F) or out of ascending order, or a negative x_row_ptr
 * start / count: the row is then left empty), bit 1 = a label outside [0, C),
 * bit 2 = a batch whose feature rows overflow the spill pool under BGCN_FEAT_SPARSE,
 * bit 3 = an internal cross-workgroup hand-off timed out (never expected).  ANY set bit
 * makes the step's results invalid: through status_flag the optimiser skips the update.
 * status_seen (optional, never cleared by the library): every step ORs its status into
 * it, so a training loop can check the validity of many steps with one host read.
 *   prepared / prepared_ready: the current batch's prepared buffer; when not ready the
 *   call prepares it first (on the same stream).
 *   next / next_prepared (optional): a batch to prepare during this step on the
 *   auxiliary lane; pass it as the next call's prepared buffer with prepared_ready = 1.
 *   status_flag (optional): receives float(status & 15) once the forward has seen every
 *   flag; placed at the tail of the flat gradient bucket it travels through the DP
 *   all-reduce, so bgcn_adam_step's skip_flag skips the update on EVERY rank when any
 *   rank's step was invalid.
 * -------------------------------------------------------------------------- */
#define BGCN_STEP_PARAMS 10
struct bgcn_adam_args;
typedef struct bgcn_step_args {
  bgcn_batch cur;                /* the batch trained on                     */
  int64_t in_feats;              /* F                                        */
  int64_t num_classes;           /* C in [1, 16] (Twitter 4, Weibo 2)        */
  const int64_t* y;              /* [B] labels                               */
  int32_t degree_on;             /* BGCN_DEGREE_ON_COL / _ROW                */
  int32_t training;              /* dropout on/off                           */
  uint64_t seed;                 /* dropout draw                             */
  int32_t feat_mode;             /* BGCN_FEAT_AUTO / _DENSE / _SPARSE        */
  const float* params[BGCN_STEP_PARAMS];
  float* grads[BGCN_STEP_PARAMS];
  float* loss;                   /* [1] mean NLL                             */
  float* logp;                   /* [B, C] log-probabilities, or NULL        */
  int32_t* status;               /* [1] or NULL                              */
  void* prepared; size_t prepared_bytes; int32_t prepared_ready;
  const bgcn_batch* next;        /* or NULL                                  */
  void* next_prepared; size_t next_prepared_bytes;
  float* status_flag;            /* [1] or NULL                              */
  /* weight images (optional): the transposed / split copies of the conv weights the
   * step's sparse-path kernels read (bgcn_weight_images_size).  images_current = 1: the
   * buffer already holds them for the CURRENT params (written by bgcn_adam_step with the
   * same buffer, params untouched since) and the step skips deriving them; 0: the step
   * derives them into the buffer. */
  void* images; int32_t images_current;
  int32_t* status_seen;          /* [1] or NULL: OR of every step's status     */
  /* defer_dw1 = 1: the call returns with every gradient written EXCEPT the two conv1
   * weight gradients (grads[0], grads[4]), which bgcn_train_step_dw1 writes later - so a
   * data-parallel caller can all-reduce the rest of the bucket while dW1 computes
   * (overlap the conv1 dW with communication). */
  int32_t defer_dw1;
  /* adam (optional, ABI 10): the optimiser step of this training step (bgcn_adam_step's
   * arguments, its tensors the ten step parameters with grad = grads[k]), performed by the
   * call: fused into the backward's last launch (each dW1 / dW2 / db1 block updates the
   * parameters whose gradients it has just finished, one extra block the head's and db2's)
   * where the step runs the sparse path in one call, else as the separate launch.  The
   * result is bit-identical to calling bgcn_adam_step after the step.  NULL: no update. */
  const struct bgcn_adam_args* adam;
} bgcn_step_args;

/* Bytes of a weight-image buffer for in_feats = F (W1^T [F][128], W2^T [2][F+64][64]
 * and the bf16 split images of W2[:, :64]); persistent, caller-owned. */
size_t bgcn_weight_images_size(int64_t in_feats);

/* workspace of the step itself (the prepared buffers are separate) */
size_t bgcn_train_step_workspace_size(int64_t num_nodes, int64_t num_graphs, int64_t in_feats,
                                      int64_t num_classes, int64_t td_num_edges,
                                      int64_t bu_num_edges);
int bgcn_train_step(const bgcn_step_args* args, void* workspace, size_t workspace_bytes,
                    bgcn_stream_t stream);
/* The conv1 weight gradients of a step run with defer_dw1 = 1: the same args, workspace
 * and prepared buffer, on the same stream, before either is reused.  The reference's
 * conv1 dW (BiGCN_Twitter.py:187 loss.backward(), the GCNConv lin weight of :22/:73). */
int bgcn_train_step_dw1(const bgcn_step_args* args, void* workspace, size_t workspace_bytes,
                        bgcn_stream_t stream);
/* (ABI 8) One evaluation step: the test loop body of BiGCN_Twitter.py:207-222
 *   model.eval(); val_out = model(Batch_data); val_loss = F.nll_loss(val_out, Batch_data.y)
 *   _, val_pred = val_out.max(dim=1); correct = val_pred.eq(Batch_data.y).sum()
 * as one call with no host sync: the forward of the (prepared or not) batch in eval mode,
 * the head, then on the device *loss = the mean NLL, correct[0] = the number of trees whose
 * argmax class (the first maximal one, as torch's max) equals y, and pred[b] (optional,
 * [B] int64) = that argmax (what the reference hands to evaluation4class).  args is the
 * training step's struct: training must be 0 and cur must carry no DropEdge; grads,
 * status_flag and defer_dw1 are ignored; logp (optional) receives the log-probabilities;
 * status / status_seen as in the training step; next / next_prepared prefetch the next
 * evaluation batch.  Workspace: bgcn_train_step_workspace_size. */
int bgcn_eval_step(const bgcn_step_args* args, int32_t* correct, int64_t* pred, void* workspace,
                   size_t workspace_bytes, bgcn_stream_t stream);
/* The saved pre-activation conv outputs of the last step run in a step workspace (the
 * fused step's form of the per-stage dumps of explain_PHEME.py:91-162): h1 = conv1 output
 * H1 (pre-relu, also the detached x2), h2 = conv2 output H2 (pre-relu), each [N, 128]
 * fp32 with TD in columns [0, 64) and BU in [64, 128).  Pointers into `workspace` (valid
 * until it is reused); the sizes must be those of the step. */
int bgcn_train_step_saved(void* workspace, size_t workspace_bytes, int64_t num_nodes,
                          int64_t num_graphs, int64_t in_feats, int64_t num_classes, float** h1,
                          float** h2);
/* A next-batch preparation (args->next) may still run on the library's auxiliary lane
 * when bgcn_train_step returns; the next bgcn_train_step call orders its stream after it.
 * bgcn_join_side makes `stream` wait for all auxiliary-lane work - call it before
 * releasing a next_prepared buffer that no later step will consume. */
int bgcn_join_side(bgcn_stream_t stream);

/* --------------------------------------------------------------------------
 * EBGCN evaluation step: the test loop body of model/Twitter/EBGCN.py:328-354
 *   model.eval(); val_out, _, _ = model(Batch_data); val_loss = F.nll_loss(val_out, Batch_data.y)
 *   _, val_pred = val_out.max(dim=1); correct = val_pred.eq(Batch_data.y).sum()
 * as one call: one launch sequence, no host round trip, no allocation (everything lives in the
 * caller's workspace).  Additive entry points: BGCN_ABI_VERSION is unchanged.
 *
 * Both directions' adjacency structure is built once (the unweighted pair build); conv1 of both
 * directions shares one pass over x; bgcn_edge_infer and bgcn_ebgcn_conv2_lin run per direction;
 * conv2 aggregates over the same t_ptr / t_col with a second value array that a reweight step
 * fills from edge_pred: the weighted degree (each node's self loop of weight 1 added last, input
 * self loops dropped, summed on the side degree_on names, in row order), dinv = deg^-1/2
 * (inf -> 0) and dinv[src] * edge_pred * dinv[dst].  For an edge list without self loops (every
 * propagation tree) these are bgcn_build_graph(edge_weight = edge_pred)'s values; that build
 * gives a node with an input self loop the loop's weight instead of 1.  A direction with
 * infer == 0 or no edges aggregates conv2 with conv1's values.  The eval-mode BatchNorms (bn1 and
 * sim_valnorm0 of both directions) are folded inside the call.  The readout runs one workgroup
 * per tree: the mean of relu(h2) over the tree's nodes summed in node order, h1[root] copied
 * (zeros for a tree without nodes, as scatter_mean), the head row laid out BU first
 * (EBGCN.py:227), then fc, log_softmax, the tree's NLL term and its argmax (the first maximal
 * class, as torch's max); a last single-workgroup launch reduces the mean loss and the correct
 * count over the trees in a fixed order.  Deterministic (no float atomics).
 * A batch vector that is not sorted sets BGCN_STATUS_BATCH_UNSORTED (information, the results
 * are valid): each tree's workgroup then picks its nodes out of the whole vector, in node order.
 * An edge, root or tree index out of range contributes zeros and sets bit 0 of *status; a label
 * outside [0, C) contributes no loss and sets bit 1.  *status is zeroed by the call.
 *
 * BGCN_EINVAL with the first failing check's message, before any HIP call: "bad sizes",
 * "num_classes must be in [1, 16]", "edge_num must be in [1, 8]", a nonzero droprate ("drops no
 * edges"), x that is not dense fp32, in_feats / ldx not multiples of 4, "null parameter pointer",
 * a null loss / correct / status, "workspace too small".
 * -------------------------------------------------------------------------- */
#define BGCN_STATUS_BATCH_UNSORTED 128
typedef struct bgcn_ebgcn_dir {   /* one direction's parameters (TDrumorGCN / BUrumorGCN), fp32 */
  const float* conv1_w; const float* conv1_b;   /* conv1.lin.weight [64, F], conv1.bias [64]   */
  const float* conv2_w; const float* conv2_b;   /* conv2.lin.weight [64, 64 + F], conv2.bias   */
  const float* bn1_weight; const float* bn1_bias;              /* bn1, [64 + F] each            */
  const float* bn1_mean; const float* bn1_var;
  const float* sim_conv_w;                      /* sim_network.sim_valconv0.weight [64, 64]    */
  const float* sim_norm_weight; const float* sim_norm_bias;    /* sim_valnorm0, [64] each       */
  const float* sim_norm_mean; const float* sim_norm_var;
  const float* sim_out_w; const float* sim_out_b;              /* sim_valconv_out [64], [1]     */
  const float* fc1_w;                           /* fc1.weight [edge_num, 64]                   */
  float bn1_eps; float sim_norm_eps;
  int32_t infer;                                /* edge_infer_td / edge_infer_bu               */
} bgcn_ebgcn_dir;
typedef struct bgcn_ebgcn_eval_args {
  bgcn_batch batch;              /* dense fp32 x; no DropEdge                */
  bgcn_ebgcn_dir td, bu;
  const float* fc_w;             /* [C, 256]                                 */
  const float* fc_b;             /* [C]                                      */
  int64_t in_feats;              /* F, a multiple of 4                       */
  int64_t num_classes;           /* C in [1, 16]                             */
  int32_t edge_num;              /* in [1, 8]                                */
  int32_t degree_on;             /* BGCN_DEGREE_ON_COL / _ROW                */
  const int64_t* y;              /* [B] labels, or NULL (loss 0, correct 0)  */
  float* logp;                   /* [B, C] or NULL                           */
  float* loss;                   /* [1] mean NLL                             */
  int32_t* correct;              /* [1]                                      */
  int64_t* pred;                 /* [B] or NULL                              */
  float* td_edge_pred;           /* [E_td] or NULL                           */
  float* bu_edge_pred;           /* [E_bu] or NULL                           */
  int32_t* status;               /* [1]                                      */
} bgcn_ebgcn_eval_args;
size_t bgcn_ebgcn_eval_workspace_size(int64_t num_nodes, int64_t num_graphs, int64_t in_feats,
                                      int64_t td_num_edges, int64_t bu_num_edges, int edge_num);
int bgcn_ebgcn_eval_step(const bgcn_ebgcn_eval_args* args, void* workspace, size_t workspace_bytes,
                         bgcn_stream_t stream);
/* The pieces of the last bgcn_ebgcn_eval_step run in `workspace` with these sizes (valid until it
 * is reused), for inspection: dir 0 = TD, 1 = BU.  t_ptr [N + 1] / t_col [E + N] = the by-target
 * structure; t_w = conv1's values; t_w2 = the reweighted values conv2 aggregated with (written
 * only for a direction with infer != 0 and edges); slot [E] = each edge's entry in that structure
 * (-1: a dropped self loop or an edge with an end out of range). */
typedef struct bgcn_ebgcn_eval_view {
  const int32_t* t_ptr; const int32_t* t_col; const float* t_w; const float* t_w2;
  const int32_t* slot;
} bgcn_ebgcn_eval_view;
int bgcn_ebgcn_eval_saved(void* workspace, size_t workspace_bytes, int64_t num_nodes, int64_t num_graphs,
                          int64_t in_feats, int64_t td_num_edges, int64_t bu_num_edges, int edge_num,
                          int dir, bgcn_ebgcn_eval_view* out);

/* --------------------------------------------------------------------------
 * EBGCN edge inference in TRAINING mode: TDrumorGCN.edge_infer / BUrumorGCN.edge_infer
 * (model/Twitter/EBGCN.py:95-116, :189-212) with batch-statistics BatchNorm, the Bayesian branch,
 * the KL edge loss, and the backward.  Additive entry points: BGCN_ABI_VERSION is unchanged.
 *
 * Per edge e, a = h[(row_e - 1) mod N], b = h[(col_e - 1) mod N] (the reference's indexing, as
 * bgcn_edge_infer), D[c][l] = |a[c] - b[l]|.  Each network n of net[] = { sim_network, W_mean,
 * W_bias, B_mean, B_bias }:
 *   Y_n[e][o][l] = sum_c conv_w[o][c] D[e][c][l]
 *   mu_n[o], v_n[o] = mean and biased variance of Y_n[.][o][.] over the n_el = 64 E_valid values
 *   Z = leaky_relu(norm_weight (Y - mu) / sqrt(v + eps) + norm_bias, 0.01)
 *   out_n[e][l] = sum_o out_w[o] Z[e][o][l] + out_b
 * and with s = out_sim:
 *   p[e][k] = sigmoid(sum_l fc1[k][l] s[e][l]);  edge_pred[e] = mean_k p[e][k]
 *   y = sigmoid(out_Wmean s + out_Bmean + relu(log(s^2 exp(out_Wbias) + exp(out_Bbias))) noise)
 *   p_y = softmax_k(fc2 y);  edge_loss = (1 / E_valid) sum_e sum_k p_y (log p_y - log_softmax_k(p))
 * batch_mean / batch_var [5, 64] receive mu_n and the UNBIASED variance v_n n_el / (n_el - 1):
 * what torch.nn.BatchNorm1d blends into its running statistics (the caller does the blend).
 * The variance is two-pass: the mean is formed first (mu = conv_w . mean(D)), the pass that sums
 * squares sums them of centred values, and block partials are merged in fp64.
 *
 * p_y is a constant target (the reference's th.normal has no gradient): the backward reaches h,
 * the sim network's five parameters and fc1 only.  It takes d_pred [E] and d_loss [1] (device)
 * and the tensors the forward saved (s [E, 64], p and p_y [E, edge_num], sim_mean and sim_rstd
 * [64], num_valid [1]) and OVERWRITES d_h [N, ldd >= 64] and the six parameter gradients.
 *
 * Y is a 64 x 64 x 64 product per edge and network on the fp32 MFMA and is never stored: the
 * forward computes it twice (statistics, apply), the backward three times.  Deterministic: no
 * float atomics; cross-block sums go through block partials in the workspace and a fixed-order
 * second step, d_h is an ordered per-node sum over a counting sort of the 2 E edge ends.
 * An edge with an end outside [0, N) reads nothing, adds to no sum, gets edge_pred 0 and sets
 * bit 0 of *status (the forward does not zero *status).
 *
 * BGCN_EINVAL before any HIP call: hid != 64 ("hidden size must be 64"), edge_num outside [1, 8]
 * ("edge_num"), num_edges <= 0 ("at least one edge"), h not 16-byte aligned or ldh % 4 != 0, a
 * null pointer, "workspace too small".  One workspace size serves both calls; 0 = bad sizes.
 * -------------------------------------------------------------------------- */
typedef struct bgcn_edge_net {     /* one per-edge network (create_network, EBGCN.py:33-46), fp32 */
  const float* conv_w;             /* <name>conv0.weight [64, 64]                  */
  const float* norm_weight;        /* <name>norm0.weight [64]                      */
  const float* norm_bias;          /* <name>norm0.bias [64]                        */
  const float* out_w;              /* <name>conv_out.weight [64]                   */
  const float* out_b;              /* <name>conv_out.bias [1]                      */
  float eps;                       /* <name>norm0.eps                              */
} bgcn_edge_net;
typedef struct bgcn_edge_train_fwd_args {
  const float* h; int64_t ldh;     /* conv1's output [N, ldh >= 64]                */
  int64_t num_nodes; int64_t hid;  /* hid == 64                                    */
  const int64_t* edge_index; int64_t num_edges;   /* [2, E], E > 0                 */
  bgcn_edge_net net[5];            /* sim_network, W_mean, W_bias, B_mean, B_bias  */
  const float* fc1_w; const float* fc2_w;         /* [edge_num, 64] each           */
  int32_t edge_num;                /* in [1, 8]                                    */
  const float* noise;              /* [E, 64] the standard-normal draw             */
  float* edge_pred;                /* [E]                                          */
  float* edge_loss;                /* [1]                                          */
  float* s; float* p; float* p_y;  /* saved: [E, 64], [E, edge_num] x 2            */
  float* sim_mean; float* sim_rstd;   /* saved: [64] each, the sim network's       */
  int32_t* num_valid;              /* saved: [1] edges with both ends in range     */
  float* batch_mean; float* batch_var;   /* [5, 64] each (unbiased variance)       */
  int32_t* status;                 /* [1]                                          */
} bgcn_edge_train_fwd_args;
typedef struct bgcn_edge_train_bwd_args {
  const float* h; int64_t ldh;
  int64_t num_nodes; int64_t hid;
  const int64_t* edge_index; int64_t num_edges;
  bgcn_edge_net sim;               /* out_b is not read                            */
  const float* fc1_w;
  int32_t edge_num;
  const float* s; const float* p; const float* p_y;
  const float* sim_mean; const float* sim_rstd;
  const int32_t* num_valid;
  const float* d_pred;             /* [E]                                          */
  const float* d_loss;             /* [1]                                          */
  float* d_h; int64_t ldd;         /* [N, ldd >= 64]                               */
  float* d_conv_w; float* d_norm_weight; float* d_norm_bias;   /* [64, 64], [64], [64] */
  float* d_out_w; float* d_out_b;  /* [64], [1]                                    */
  float* d_fc1_w;                  /* [edge_num, 64]                               */
} bgcn_edge_train_bwd_args;
size_t bgcn_edge_infer_train_workspace_size(int64_t num_nodes, int64_t num_edges);
int bgcn_edge_infer_train_fwd(const bgcn_edge_train_fwd_args* args, void* workspace, size_t workspace_bytes,
                              bgcn_stream_t stream);
int bgcn_edge_infer_train_bwd(const bgcn_edge_train_bwd_args* args, void* workspace, size_t workspace_bytes,
                              bgcn_stream_t stream);

/* --------------------------------------------------------------------------
 * EBGCN bn1 + relu + conv2's lin in TRAINING mode (model/Twitter/EBGCN.py:72-84) and the backward,
 * without the dense [N, 64 + F] concat.  Additive entry points: BGCN_ABI_VERSION is unchanged.
 *
 * The concat row of node i is c_i = [h1_i | x[rootindex[batch_i]]]; n_b = nodes of tree b, N = the
 * valid nodes.  Forward:
 *   h columns: mean / biased variance over the N rows of h1
 *   x columns: mean = (1/N) sum_b n_b x[r_b],  var = (1/N) sum_b n_b (x[r_b] - mean)^2
 *   bn_g = gamma / sqrt(var + eps),  bn_t = beta - mean bn_g
 *   z2_i = relu(g_h h1_i + t_h) W2[:, :64]^T + r[batch_i],  r[b] = a_x[b] W2[:, 64:]^T,
 *   a_x[b] = relu(g_x x[r_b] + t_x)
 * z2 has the bits of bgcn_ebgcn_conv2_lin called with the returned bn_g / bn_t (it is that code).
 * batch_var is the BIASED variance; torch blends var N / (N - 1) into running_var (the caller
 * does the blend, with *num_valid).  Backward, dR[b] = sum_{i in b} dz2_i, a_h = relu(y_h):
 *   dW2[:, :64] = dz2^T a_h                dW2[:, 64:] = dR^T a_x      (B rows, not N)
 *   dY_h = (dz2 W2[:, :64]) . [y_h > 0]    dY_x[b] = (dR[b] W2[:, 64:]) . [y_x[b] > 0]
 *   dbeta = column sums of dY (N rows / B rows);  dgamma = those of dY . chat, chat = (c - mean) rstd
 *   dh1_i = g_h . (dY_h,i - dbeta_h / N - chat_h,i . dgamma_h / N)        (x gets no gradient)
 * The backward OVERWRITES dh1 [N, ldd >= 64], dw2 [64, 64 + F] (leading dimension 64 + F), dgamma
 * and dbeta [64 + F].
 *
 * Nothing of size N x F is read or written; the largest arrays are [B, F] and [N, 64].
 * Workspace (one size serves both calls): bgcn_ebgcn_conv2_lin's, the statistics' block partials
 * ([ceil(N / 256)] and [ceil(B / 32)] triples per column), a_h and dz2 W2[:, :64] [N, 64] each,
 * dR [B, 64], dR W2[:, 64:] [B, F], the backward's block partials and bgcn_gemm_tn's split
 * partials; 0 = bad sizes.
 * Deterministic: no float atomics; every float sum goes through block partials and one ordered
 * pass, variances are of centred values (an ordered merge of per-block (n, mean, M2) triples).
 * The batch vector need not be sorted.
 *
 * A node is invalid when its tree id is outside [0, B) or its tree's rootindex outside [0, N): it
 * is never read through, is left out of N and of every statistic, gets a zero z2 row and a zero
 * dh1 row, and sets bit 0 of *status (the forward does not zero *status).  A tree id without
 * nodes has weight 0.  With *num_valid < 2 there are no batch statistics: every output of both
 * calls is zero (decided on the device).
 *
 * BGCN_EINVAL before any HIP call: hid != 64 ("hidden size must be 64"), in_feats not a positive
 * multiple of 4 ("in_feats"), N <= 0 or B <= 0, "batch too large", leading dimensions not
 * multiples of 4 or too short, a negative eps, a "null pointer", pointers not "16-byte aligned",
 * "workspace too small".
 * -------------------------------------------------------------------------- */
typedef struct bgcn_conv2_lin_train_fwd_args {
  const float* h1; int64_t ldh;    /* conv1's output [N, ldh >= 64]                */
  const float* x; int64_t ldx;     /* the features [N, ldx >= F], fp32             */
  const int64_t* batch;            /* [N] node -> tree                             */
  const int64_t* rootindex;        /* [B] tree -> root node                        */
  int64_t num_nodes; int64_t num_graphs; int64_t in_feats;
  int64_t hid;                     /* hid == 64                                    */
  const float* w2;                 /* conv2.lin.weight [64, 64 + F]                */
  const float* gamma; const float* beta;   /* bn1.weight, bn1.bias [64 + F]        */
  float eps;                       /* bn1.eps                                      */
  float* z2; int64_t ldz;          /* [N, ldz >= 64]                               */
  float* batch_mean; float* batch_var;     /* [64 + F] each (biased variance)      */
  float* bn_g; float* bn_t;        /* saved: [64 + F] each, the fold               */
  float* a_x;                      /* saved: [B, F] the activated root table       */
  int32_t* tree_count;             /* saved: [B] valid nodes per tree              */
  int32_t* num_valid;              /* saved: [1] valid nodes                       */
  int32_t* status;                 /* [1]                                          */
} bgcn_conv2_lin_train_fwd_args;
typedef struct bgcn_conv2_lin_train_bwd_args {
  const float* dz2; int64_t lddz;  /* [N, lddz >= 64]                              */
  const float* h1; int64_t ldh;
  const float* x; int64_t ldx;
  const int64_t* batch;
  const int64_t* rootindex;
  int64_t num_nodes; int64_t num_graphs; int64_t in_feats;
  int64_t hid;
  const float* w2;
  float eps;
  const float* batch_mean; const float* batch_var;
  const float* bn_g; const float* bn_t;
  const float* a_x;
  const int32_t* tree_count;
  const int32_t* num_valid;
  float* dh1; int64_t ldd;         /* [N, ldd >= 64]                               */
  float* dw2;                      /* [64, 64 + F]                                 */
  float* dgamma; float* dbeta;     /* [64 + F] each                                */
} bgcn_conv2_lin_train_bwd_args;
size_t bgcn_ebgcn_conv2_lin_train_workspace_size(int64_t num_nodes, int64_t num_graphs, int64_t in_feats);
int bgcn_ebgcn_conv2_lin_train_fwd(const bgcn_conv2_lin_train_fwd_args* args, void* workspace,
                                   size_t workspace_bytes, bgcn_stream_t stream);
int bgcn_ebgcn_conv2_lin_train_bwd(const bgcn_conv2_lin_train_bwd_args* args, void* workspace,
                                   size_t workspace_bytes, bgcn_stream_t stream);

/* --------------------------------------------------------------------------
 * Optimiser step of the training loop: torch.optim.Adam with the reference's three
 * parameter groups (BiGCN_Twitter.py:146-153, step at :189) as ONE fused launch.
 * amsgrad = False; weight_decay is L2 added to the gradient (torch Adam semantics).
 * grad_scale multiplies every gradient first (1/world for a summed DP bucket).
 * bias_correction1 = 1 - beta1^t, bias_correction2_sqrt = sqrt(1 - beta2^t).
 * skip_flag (optional): when *skip_flag != 0 on the device the launch leaves every
 * parameter and moment untouched (an invalid step, see bgcn_step_args.status_flag) and
 * adds one to *skip_count (optional).
 * block_start is scratch filled by the library.
 * -------------------------------------------------------------------------- */
#define BGCN_ADAM_MAX_TENSORS 16
typedef struct bgcn_adam_tensor {
  float* param; const float* grad; float* exp_avg; float* exp_avg_sq;
  int64_t numel; float lr;
} bgcn_adam_tensor;
typedef struct bgcn_adam_args {
  bgcn_adam_tensor t[BGCN_ADAM_MAX_TENSORS];
  int64_t block_start[BGCN_ADAM_MAX_TENSORS];
  int count;
  float beta1, beta2, eps, weight_decay;
  float bias_correction1, bias_correction2_sqrt, grad_scale;
  const float* skip_flag;        /* [1] or NULL                              */
  /* weight images (optional): with images set, the tensors whose image_role is one of
   * BGCN_IMAGE_* (conv weights [64][F] / [64][F+64]) are updated tile by tile and their
   * updated values also written into the image buffer of a step with in_feats =
   * images_in_feats, which the next bgcn_train_step then uses with images_current = 1
   * (an invalid step leaves params and images untouched alike). */
  void* images; int64_t images_in_feats;
  int32_t image_role[BGCN_ADAM_MAX_TENSORS];
  /* skip_count (optional): incremented on the device each time skip_flag skips the
   * update, so the number of invalid steps of a run is one host read at its end */
  int32_t* skip_count;
} bgcn_adam_args;
#define BGCN_IMAGE_NONE 0
#define BGCN_IMAGE_TD_W1 1
#define BGCN_IMAGE_BU_W1 2
#define BGCN_IMAGE_TD_W2 3
#define BGCN_IMAGE_BU_W2 4
int bgcn_adam_step(const bgcn_adam_args* args, bgcn_stream_t stream);

/* --------------------------------------------------------------------------
 * The same update for MANY tensors in ONE launch: up to BGCN_ADAM_MULTI_MAX_TENSORS tensors in
 * up to BGCN_ADAM_MULTI_MAX_GROUPS learning-rate groups (an EBGCN has 68 parameter tensors in five
 * groups, EBGCN.py:249-260).  Additive entry points: BGCN_ABI_VERSION is unchanged.
 *
 * What is fixed between steps lives in a TABLE in device memory, one bgcn_adam_multi_tensor per
 * tensor: param, exp_avg, exp_avg_sq, numel, the group and first_block, the tensor's first
 * workgroup (a workgroup updates one chunk of BGCN_ADAM_MULTI_CHUNK elements of one tensor;
 * first_block[k] = sum over j < k of ceil(numel[j] / BGCN_ADAM_MULTI_CHUNK)).
 * bgcn_adam_multi_plan fills a HOST image of it from the caller's entries (param, exp_avg,
 * exp_avg_sq, numel, group; first_block is written by the plan) and returns the launch's workgroup
 * count; the caller copies the image to the device once, and again only when a tensor's storage
 * changes.  What changes every step travels in the kernel arguments (no per-step host-to-device
 * copy): the gradient pointers, the groups' learning rates, the step's constants, skip_flag and
 * skip_count.  grad[k] == NULL is torch.optim.Adam's `grad is None`: tensor k's parameter and both
 * moments are not touched (no weight decay either).  A workgroup finds its tensor by a binary
 * search over first_block.  The arithmetic is bgcn_adam_step's (the same bits); skip_flag and
 * skip_count behave as there.
 *
 * BGCN_EINVAL, decided on the host before any launch: count outside [1, 128], a null table, a
 * table buffer smaller than bgcn_adam_multi_table_size(count), a group outside [0, 8), numel < 0,
 * a null param / exp_avg / exp_avg_sq where numel > 0, more than 2^31 - 1 workgroups (plan);
 * count outside [1, 128], a null table, blocks < 0 (step).
 * -------------------------------------------------------------------------- */
#define BGCN_ADAM_MULTI_MAX_TENSORS 128
#define BGCN_ADAM_MULTI_MAX_GROUPS 8
#define BGCN_ADAM_MULTI_CHUNK 1024
typedef struct bgcn_adam_multi_tensor {
  float* param; float* exp_avg; float* exp_avg_sq;
  int64_t numel;
  int64_t first_block;           /* written by bgcn_adam_multi_plan          */
  int32_t group;                 /* index into bgcn_adam_multi_args.lr       */
  int32_t reserved;
} bgcn_adam_multi_tensor;
typedef struct bgcn_adam_multi_args {
  const bgcn_adam_multi_tensor* table;   /* device memory, [count]          */
  int32_t count;
  int64_t blocks;                /* bgcn_adam_multi_plan's total             */
  const float* grad[BGCN_ADAM_MULTI_MAX_TENSORS];   /* NULL: no gradient this step */
  float lr[BGCN_ADAM_MULTI_MAX_GROUPS];
  float beta1, beta2, eps, weight_decay;
  float bias_correction1, bias_correction2_sqrt, grad_scale;
  const float* skip_flag;        /* [1] or NULL                              */
  int32_t* skip_count;           /* [1] or NULL                              */
} bgcn_adam_multi_args;
size_t bgcn_adam_multi_table_size(int count);   /* 0 for a count outside [1, 128] */
int bgcn_adam_multi_plan(const bgcn_adam_multi_tensor* tensors, int count, void* table_host,
                         size_t table_bytes, int64_t* blocks);
int bgcn_adam_multi_step(const bgcn_adam_multi_args* args, bgcn_stream_t stream);

/* --------------------------------------------------------------------------
 * The loss of EBGCN's training loop (EBGCN.py:301-306), its accuracy (:311-312), the gradient
 * the backward starts from and the step's skip decision, in one single-workgroup launch:
 *   loss    = -mean_i logp[i][y_i] + edge_loss_td * *td_loss + edge_loss_bu * *bu_loss
 *             (td_loss / bu_loss NULL: that direction's edge inference is off, no term)
 *   correct = #{i : argmax_c logp[i][c] == y_i}, pred[i] (optional) that argmax, the first index
 *             of the row maximum as torch.max gives it
 *   dlogp   = [B, C]: -1 / B at (i, y_i), 0 elsewhere
 * A label outside [0, C) sets bit 1 (value 2) of *status, as bgcn_ebgcn_eval_step does; that tree
 * adds nothing to the loss (the mean still divides by B) and its dlogp row is zero.  *skip_flag =
 * 1 when *status is non-zero after that (set by the step's forward or here), else 0: the
 * optimiser's skip_flag.  *status_seen (optional) |= *status.  The sums are deterministic: tree i
 * goes to lane i % 256 in order, a fixed butterfly per wave, the four waves in order.
 * BGCN_EINVAL: num_graphs < 1, num_classes outside [1, 16], a null logp / y / loss / correct /
 * dlogp / status / skip_flag.
 * -------------------------------------------------------------------------- */
int bgcn_ebgcn_train_loss(const float* logp, const int64_t* y, int64_t num_graphs, int32_t num_classes,
                          const float* td_loss, const float* bu_loss, float edge_loss_td, float edge_loss_bu,
                          float* loss, int32_t* correct, int64_t* pred, float* dlogp, int32_t* status,
                          float* skip_flag, int32_t* status_seen, bgcn_stream_t stream);

/* Materialise the in-kernel dropout keep bits (for tests / debugging):
 * words[dir][n][w] for dir in {0 (TD), 1 (BU)}. */
int bgcn_keep_words(uint64_t seed, int64_t num_nodes, int32_t num_words, uint32_t* words,
                    bgcn_stream_t stream);

/* Timing hook for bench.py: accumulated HIP-event time (ms) and launch count of a
 * kernel class of the fused encoder since bgcn_set_kernel_timing(mask) (process-wide;
 * events are recorded on the launch stream; mask bit c enables class c, 0 disables and
 * keeps the recorded events for bgcn_kernel_timing).  Classes:
 *   0 conv1 (dense: X*W1^T MFMA; auto: k_compact_conv1, or the gather from a prepared ELL)
 *   1 dW1 dense MFMA
 *   2 conv2 (dense MFMA + sparse root gather)            3 dW2 relu(H1) block MFMA
 *   4 gated dense conv1 fallback (auto)                  5 dW1 + dW2 root columns over CSC(X)
 *   6 gated dense dW1 fallback (auto)                   7 ELL compaction of X (batch preparation)
 * Span classes of bgcn_train_step (diagnostics): 8 the next batch's preparation on the
 * auxiliary lane, 9 the caller stream's own chain up to the final join, 10 the whole call. */
int bgcn_set_kernel_timing(int enable);
int bgcn_kernel_timing(int kernel_class, float* total_ms, int64_t* launches);
/* The same classes' device-side spans, for the kernels that stamp themselves (class 7, the
 * batch preparation's pass over X - or over the compacted rows - k_prep_b): per launch, the
 * first block's start to the last block's end on the device's constant wall clock
 * (hipDeviceAttributeWallClockRate), i.e. the kernel's own duration as rocprofv3 reports
 * it, without the dispatch delay an event bracket on a busy lane includes.  Synchronises. */
int bgcn_kernel_span(int kernel_class, float* total_ms, int64_t* launches);

/* ---- Native host-fed loader (ABI 9; replaces, for the fused step, the reference's
 * DataLoader(traindata_list, batch_size, shuffle=True, num_workers=5) + Batch_data.to(device),
 * model/Twitter/BiGCN_Twitter.py:168,174-176, and feed.py's worker-process DataLoader).
 * A tree store (feed.TreeStore's arrays, caller-owned for the loader's lifetime): */
typedef struct bgcn_tree_store {
  int64_t num_trees, in_feats;
  const int64_t* tree_node;   /* [T+1] node offsets */
  const int32_t* node_nnz;    /* [Nall] non-zeros per node */
  const int64_t* entry_off;   /* [T+1] non-zero offsets */
  const int32_t* cols;        /* [nnz] ascending per node */
  const float* vals;          /* [nnz] */
  const int64_t* tree_edge;   /* [T+1] edge offsets */
  const int32_t* edges;       /* [2, edges_ld]: (parent, child) in local ids */
  int64_t edges_ld;
  const int32_t* rootindex;   /* [T] local */
  const int64_t* y;           /* [T] */
} bgcn_tree_store;
/* One packed batch: feed.pack_batch's layout (sections x_row_ptr int32 [N+1], x_col int32,
 * x_val fp32, edge_index int64 [2,E], BU_edge_index int64 [2,E], batch int64 [N], rootindex
 * int64 [B], y int64 [B], ptr int64 [B+1], each at a 256-byte aligned byte offset off[k]). */
typedef struct bgcn_loader_batch {
  int64_t num_nodes, num_graphs, nnz, td_num_edges, bu_num_edges, nnz_max, spill, bytes;
  int64_t off[9];
  int64_t seq;
} bgcn_loader_batch;
/* indices (optional): the trees of the dataset (else all); batches of batch_size in a
 * Fisher-Yates order per epoch from `seed` (shuffle) or in order; num_threads collating
 * threads over nslots page-locked slots (pinned = 0: plain memory, host-only use). */
int bgcn_loader_create(const bgcn_tree_store* store, const int64_t* indices, int64_t num_indices,
                       int64_t batch_size, int drop_last, int shuffle, uint64_t seed, int64_t epochs,
                       int num_threads, int nslots, int bf16_values, int pinned, void** handle);
int64_t bgcn_loader_slot_bytes(void* handle);   /* an upper bound of any batch's bytes */
int64_t bgcn_loader_len(void* handle);          /* batches over all epochs */
/* The next batch in order: its layout in *out, its trees (store ids) in trees[0..B) when
 * given; with dst, one host-to-device copy of its bytes into dst on `stream` (the slot is
 * reused once that copy completed); without dst (host-only loader), *host_bytes points at
 * the packed bytes until the next call.  Returns 1 after the last batch. */
int bgcn_loader_next(void* handle, void* dst, size_t dst_bytes, bgcn_stream_t stream, bgcn_loader_batch* out,
                     int64_t* trees, int64_t trees_cap, const void** host_bytes);
/* (ABI 12) Block until the next batch is packed, without taking it (a copy timed after this
 * call holds only the copy); returns 1 after the last batch. */
int bgcn_loader_wait(void* handle);
/* (ABI 12) Where the loader's time goes, since creation or the last reset: batches packed,
 * thread-milliseconds inside the packing, thread-milliseconds waiting for a slot's turn (its
 * previous batch's copy issued and completed), caller milliseconds waiting in
 * bgcn_loader_next / bgcn_loader_wait for a packed batch, the collating threads, and the
 * caller's host milliseconds inside the copy-issuing HIP calls (total; the largest
 * hipMemcpyAsync and hipEventRecord call). */
typedef struct bgcn_loader_stats {
  int64_t packs;
  double pack_ms, slot_wait_ms, caller_wait_ms;
  int64_t threads;
  double copy_call_ms, copy_call_ms_max, record_call_ms_max;
} bgcn_loader_stats;
int bgcn_loader_get_stats(void* handle, bgcn_loader_stats* out, int reset);
void bgcn_loader_destroy(void* handle);

/* --------------------------------------------------------------------------
 * LSTM baseline, evaluation: the test loop body of model/Twitter/LSTM_Twitter.py:146-173
 *   for each tree: val_out[b] = model(cls[rootindex[b] : rootindex[b + 1]])   (the last to N)
 *   val_loss = F.nll_loss(val_out, y); _, val_pred = val_out.max(dim=1); correct = ...
 * for a whole batch of trees as one call: one launch sequence, no host round trip, no allocation
 * (everything lives in the caller's workspace).  Additive entry points: BGCN_ABI_VERSION is
 * unchanged.
 *
 * The model is nn.LSTM(in_feats, hid, num_layers, batch_first, bidirectional, bias = False) and
 * fc = nn.Linear(2 * num_layers * hid, out_feats).  w_ih[l][d] / w_hh[l][d] are weight_ih_l{l} /
 * weight_hh_l{l} (d = 1: the _reverse ones): [4 hid, K_l] and [4 hid, hid], K_0 = in_feats,
 * K_l = 2 hid, gate rows in the order i, f, g, o; c' = sig(f) c + sig(i) tanh(g),
 * h = sig(o) tanh(c'), h0 = c0 = 0.  Sequence b is the rows [seq_start[b], seq_start[b + 1]) of
 * x (the last one runs to num_nodes); the reverse direction runs over each sequence's own length.
 * Per layer one GEMM gives both directions' input projections G [N, 8 hid]; then one launch per
 * time step s < max_len covers both directions and every sequence still running (forward: row
 * start + s, reverse: row start + len - 1 - s), reading h of the previous step from the layer
 * output Y_l [N, 2 hid] (forward in columns [0, hid), reverse in [hid, 2 hid)) and writing its
 * own row there; stream order is the only dependency between the launches.  h_n is ordered
 * (l0 fwd, l0 rev, l1 fwd, ...): a forward direction's final state is Y_l at the sequence's last
 * row, a reverse direction's at its first.  logp = log_softmax(fc(h_n of the sequence, flattened
 * in that order)); with y, loss = the mean NLL, pred = the first maximal class (torch's max),
 * correct = the number of sequences with pred == y; without y, loss and correct are 0.  Rows of x
 * before seq_start[0] belong to no sequence: their rows of every Y_l (and of `out`) are zeros.
 * Deterministic: no float atomics, fixed summation orders.
 *
 * Validity is decided on the device.  *status is zeroed by the call; BGCN_STATUS_SEQUENCE is set by
 * a seq_start that does not increase strictly, a start outside [0, num_nodes), a sequence longer
 * than max_len (max_len is the number of step launches: the caller's bound, never a truncation),
 * or a label outside [0, out_feats).  A fault in seq_start or max_len empties every sequence of the
 * batch: no step runs, every final state is zero, nothing out of bounds is read or written and
 * the results are not to be used; a bad label contributes no loss.
 *
 * BGCN_EINVAL before any HIP call: in_feats not a positive multiple of 4, hid not a multiple of 64
 * in [64, 1024], num_layers outside [1, 4] ("unsupported shape"; bgcn_lstm_workspace_size returns
 * 0 for these), out_feats outside [1, 64], max_len < 1, a null x / seq_start / weight / fc /
 * logp / status, x, ldx or a weight not 16-byte aligned, "workspace too small".
 * -------------------------------------------------------------------------- */
#define BGCN_STATUS_SEQUENCE 256
#define BGCN_LSTM_SEQ_TILE 32    /* sequences per workgroup of a step launch */
typedef struct bgcn_lstm_args {
  const float* x;                /* [N, ldx] fp32, in_feats columns used     */
  int64_t ldx;
  int64_t num_nodes;             /* N                                        */
  int64_t in_feats;
  int64_t hid;                   /* H                                        */
  int64_t num_layers;            /* L                                        */
  int64_t out_feats;             /* C                                        */
  const int64_t* seq_start;      /* [B] first row of each sequence           */
  int64_t num_seqs;              /* B                                        */
  int64_t max_len;               /* step launches per layer                  */
  const float* w_ih[4][2];       /* [layer][direction]: [4H, K_l]            */
  const float* w_hh[4][2];       /* [4H, H]                                  */
  const float* fc_w;             /* [C, 2 L H]                               */
  const float* fc_b;             /* [C]                                      */
  const int64_t* y;              /* [B] labels, or NULL                      */
  float* logp;                   /* [B, C]                                   */
  float* h_n;                    /* [2 L, B, H] or NULL                      */
  float* out;                    /* [N, 2H] last layer's output, or NULL     */
  float* loss;                   /* [1] mean NLL, or NULL                    */
  int32_t* correct;              /* [1] or NULL                              */
  int64_t* pred;                 /* [B] or NULL                              */
  int32_t* status;               /* [1]                                      */
} bgcn_lstm_args;
size_t bgcn_lstm_workspace_size(int64_t num_nodes, int64_t num_seqs, int64_t in_feats, int64_t hid,
                                int64_t num_layers);
int bgcn_lstm_eval(const bgcn_lstm_args* args, void* workspace, size_t workspace_bytes, bgcn_stream_t stream);

/* --------------------------------------------------------------------------
 * LSTM baseline, training: one iteration of model/Twitter/LSTM_Twitter.py:96-126 up to the
 * optimiser - the forward of bgcn_lstm_eval, the mean NLL and the accuracy, and the gradient of
 * the loss with respect to every parameter (and, optionally, x) - for a whole batch of trees as
 * one launch sequence: no host round trip, no allocation.  Additive entry points:
 * BGCN_ABI_VERSION is unchanged.
 *
 * `fwd` is bgcn_lstm_eval's argument struct with y required; logp, loss, correct, pred, h_n and
 * out are bgcn_lstm_eval's bits on the same batch (the kernels are the same definitions; the
 * training forward also keeps, per layer, the activated gates [N, 8 hid] over the input
 * projections in place and the cell state of every row [N, 2 hid] in the workspace).
 *
 * Backward.  dz = (softmax - onehot(y)) / B per sequence; d_fc_w [C, 2 L hid] = dz^T h_n and
 * d_fc_b = the column sums of dz, over the sequences in order; d h_n = dz fc_w enters dY_l at the
 * sequence's last row (forward half) and first row (reverse half).  Per layer, from the last down,
 * one launch per time step s = max_len - 1 .. 0 covers both directions and every sequence with
 * s < len on the forward's row mapping: dh = dY_l[row] + W_hh^T dpre(step s + 1) (no recurrent
 * term and no carry at s = len - 1), then with the saved i, f, g, o, c and c_prev (0 at s = 0)
 *   dc = carry + dh o (1 - tanh^2 c)          dpre_o = dh tanh(c) o (1 - o)
 *   dpre_i = dc g i (1 - i)   dpre_g = dc i (1 - g^2)   dpre_f = dc c_prev f (1 - f)   carry = dc f
 * written over the row's gates.  After a layer's steps, with dG_l [N, 8 hid] those rows:
 *   d_w_ih[l][d] = dG_l[:, d]^T X_l;   d_w_hh[l][d] = dG_l[:, d]^T Hprev_l[:, d], Hprev the layer's
 *   output shifted by one row inside each sequence (forward: the previous row, reverse: the next
 *   one, zero where the sequence has none);   dX_l = dG_l [w_ih[l][0] ; w_ih[l][1]], which is added
 *   into dY_{l-1}, or written to dx [N, ldx] (in_feats columns; optional) for l = 0.
 * The gradient buffers are written whole, never accumulated into.  Deterministic: no float
 * atomics, every sum in a fixed order; two calls on the same inputs give the same bits.
 *
 * Rows of x before seq_start[0] belong to no sequence.  Their rows of dx are zeros, and they meet
 * zero rows of dG_0 in d_w_ih[0]: they must hold finite numbers.
 *
 * Validity: as bgcn_lstm_eval (*status, BGCN_STATUS_SEQUENCE; a fault in seq_start or max_len
 * empties every sequence, a bad label adds no loss and no gradient).  *skip_flag is 1.0f when
 * *status is non-zero after the forward, else 0.0f: the optimiser's skip flag
 * (bgcn_adam_multi_step, as bgcn_ebgcn_train_loss writes it).  A faulted batch reads and writes
 * nothing out of bounds; its gradients are not to be used.
 *
 * BGCN_EINVAL before any HIP call: bgcn_lstm_eval's conditions, a null y / gradient pointer /
 * skip_flag, a weight gradient or dx not 16-byte aligned, "workspace too small"
 * (bgcn_lstm_train_workspace_size; 0 for an unsupported shape).
 * -------------------------------------------------------------------------- */
typedef struct bgcn_lstm_train_args {
  bgcn_lstm_args fwd;            /* y required                               */
  float* d_w_ih[4][2];           /* [layer][direction]: [4H, K_l]            */
  float* d_w_hh[4][2];           /* [4H, H]                                  */
  float* d_fc_w;                 /* [C, 2 L H]                               */
  float* d_fc_b;                 /* [C]                                      */
  float* dx;                     /* [N, ldx] (fwd.ldx), or NULL              */
  float* skip_flag;              /* [1]                                      */
} bgcn_lstm_train_args;
size_t bgcn_lstm_train_workspace_size(int64_t num_nodes, int64_t num_seqs, int64_t in_feats, int64_t hid,
                                      int64_t num_layers);
int bgcn_lstm_train_grad(const bgcn_lstm_train_args* args, void* workspace, size_t workspace_bytes,
                         bgcn_stream_t stream);

/* --------------------------------------------------------------------------
 * TreeBERT baseline, evaluation and explain: the test loop body of model/Twitter/BERT_Twitter.py
 * (:20-42, :86-110) and the BERT branch of explain_PHEME.py (:581-600) for a whole batch of trees
 * as one call: one launch sequence, no host round trip, no allocation (everything lives in the
 * caller's workspace).  Additive entry points: BGCN_ABI_VERSION is unchanged.
 *
 * The model is BertModel(is_decoder = True) fed inputs_embeds in eval mode with no attention mask,
 * then fc(pooler_output) and log_softmax.  Sequence b is the rows [seq_start[b], seq_start[b + 1])
 * of x (the last one runs to num_nodes), n of them, x[t] its row t:
 *   embeddings  h = LN(x[t] + position_embeddings[t] + token_type_embeddings[0])
 *               (LN: biased variance, eps = ln_eps; word_embeddings is never read)
 *   per layer   q, k, v = Linear(h); per head (width 64): P = softmax(q k^T / 8) over the keys
 *               j <= t, ctx = P v;  a = LN(dense(ctx) + h);  o = LN(dense2(gelu(dense1(a))) + a),
 *               gelu(x) = x 0.5 (1 + erf(x / sqrt 2))
 *   head        pooled = tanh(pooler.dense(o_last[0])); logp = log_softmax(fc(pooled))
 * With y, loss = the mean NLL, pred = the first maximal class (torch's max), correct = the number
 * of sequences with pred == y; without y, loss and correct are 0.
 *
 * Root-only form (hidden, hidden_sum and attn_sum all NULL).  Row 0 attends to itself only and a
 * softmax over one key is exactly 1, so pooled is a function of the sequence's first row alone:
 * the call gathers the B root rows and runs embeddings + LN at position 0, then per layer the
 * value projection, the attention-output dense, the intermediate and output GEMMs with their row
 * kernels on [B, hidden].  No q, k or score is computed and no other row of x is read.
 *
 * Full form (any of the three given).  Every row goes through every layer; attention is a causal
 * two-pass kernel on the fp32 MFMA, one wave per (sequence, head, tile of 32 queries): pass 1 the
 * row maxima and normalisers over the key tiles, pass 2 the normalised P, ctx = P v and P's column
 * sums.  hidden [N, hidden] is last_hidden_state, hidden_sum [N] its row sums, attn_sum [N] per
 * key the sum of P over layers, heads and queries (attention_head.sum(-2).sum(1) summed over the
 * layers), reduced through workspace partials in a fixed order.  Rows before seq_start[0] belong to
 * no sequence: their hidden, hidden_sum and attn_sum are zeros.  logp comes from the full pass's own
 * row 0 of each sequence (the root-only chain is not run beside it).  Deterministic: no float
 * atomics, fixed summation orders.
 *
 * The launch grid covers max_pos queries per sequence with early exit: there is no max_len
 * argument and no host sync.
 *
 * Validity is decided on the device.  *status is zeroed by the call; BGCN_STATUS_SEQUENCE is set by
 * a seq_start that does not increase strictly, a start outside [0, num_nodes), a sequence longer
 * than max_pos (an index error in the reference; never truncated here), or a label outside
 * [0, out_feats).  A fault in seq_start or a length empties every sequence: nothing out of bounds
 * is read or written, every row counts as outside any sequence, and the results are not to be
 * used; a bad label contributes no loss.
 *
 * BGCN_EINVAL before any HIP call: hidden not 64 heads or outside [64, 1024], intermediate not a
 * multiple of 64 in [64, 4096], num_layers outside [1, 24], max_pos outside [1, 512], out_feats
 * outside [1, 64] ("unsupported shape"; bgcn_bert_workspace_size returns 0 for these), a null or
 * not 16-byte aligned pointer (x, ldx, every weight, logp, the optional outputs, the workspace),
 * "workspace too small".
 * -------------------------------------------------------------------------- */
#define BGCN_BERT_MAX_LAYERS 24
#define BGCN_BERT_QUERY_TILE 32   /* queries per workgroup of the attention kernel */
typedef struct bgcn_bert_layer {
  const float *q_w, *q_b, *k_w, *k_b, *v_w, *v_b;   /* attention.self: [hidden, hidden], [hidden] */
  const float *ao_w, *ao_b, *ao_ln_w, *ao_ln_b;     /* attention.output.dense / LayerNorm         */
  const float *i_w, *i_b;                           /* intermediate.dense: [intermediate, hidden] */
  const float *o_w, *o_b, *o_ln_w, *o_ln_b;         /* output.dense [hidden, intermediate] / LN   */
} bgcn_bert_layer;
typedef struct bgcn_bert_args {
  const float* x;                /* [N, ldx] fp32, hidden columns used        */
  int64_t ldx;
  int64_t num_nodes;             /* N                                         */
  const int64_t* seq_start;      /* [B] first row of each sequence            */
  int64_t num_seqs;              /* B                                         */
  int64_t hidden;                /* 64 heads                                  */
  int64_t heads;
  int64_t intermediate;
  int64_t num_layers;
  int64_t max_pos;               /* rows of pos_emb: the longest sequence     */
  int64_t out_feats;             /* C                                         */
  float ln_eps;
  int32_t reserved;
  const float* pos_emb;          /* [max_pos, hidden]                         */
  const float* type_emb;         /* [hidden]: token_type_embeddings row 0     */
  const float* emb_ln_w;         /* [hidden]                                  */
  const float* emb_ln_b;
  bgcn_bert_layer layer[BGCN_BERT_MAX_LAYERS];
  const float* pooler_w;         /* [hidden, hidden]                          */
  const float* pooler_b;
  const float* fc_w;             /* [C, hidden]                               */
  const float* fc_b;
  const int64_t* y;              /* [B] labels, or NULL                       */
  float* logp;                   /* [B, C]                                    */
  float* loss;                   /* [1] mean NLL, or NULL                     */
  int32_t* correct;              /* [1] or NULL                               */
  int64_t* pred;                 /* [B] or NULL                               */
  float* hidden_out;             /* [N, hidden] last_hidden_state, or NULL    */
  float* hidden_sum;             /* [N] or NULL                               */
  float* attn_sum;               /* [N] or NULL                               */
  int32_t* status;               /* [1]                                       */
} bgcn_bert_args;
size_t bgcn_bert_workspace_size(int64_t num_nodes, int64_t num_seqs, int64_t hidden, int64_t intermediate,
                                int64_t num_layers, int want_full);
int bgcn_bert_eval(const bgcn_bert_args* args, void* workspace, size_t workspace_bytes, bgcn_stream_t stream);

/* --------------------------------------------------------------------------
 * TreeBERT baseline, training: one iteration of model/Twitter/BERT_Twitter.py:89-119 up to the
 * optimiser - BertModel in training mode (its four dropout sites), the mean NLL, the accuracy and
 * the gradient of the loss with respect to every parameter the loss depends on (and, optionally,
 * x) - for a whole batch of trees as one launch sequence: no host round trip, no allocation.
 * Additive entry points: BGCN_ABI_VERSION is unchanged.
 *
 * Training is root-only by construction.  Position 0 attends to itself only, the pooler reads
 * position 0 and dropout is element-wise, so the loss is a function of each sequence's first row
 * also in training mode; the gradient of a softmax over one unmasked key is exactly 0.  `fwd` is
 * bgcn_bert_eval's argument struct with y required and hidden_out, hidden_sum and attn_sum NULL.
 * The forward is the root-only chain of bgcn_bert_eval on [B, hidden] (the same GEMMs, LayerNorm
 * and head definitions) with dropout; with both rates 0 logp, loss, correct and pred are
 * bgcn_bert_eval's bits.  The workspace keeps per layer the normalised rows and 1 / sqrt(var + eps)
 * of both LayerNorm inputs, ctx, the attention-output LayerNorm's output, the intermediate before
 * and after GELU, and the layer's output.
 *
 * Dropout.  Sites: 0 after the embeddings' LayerNorm; for layer l: 3 l + 1 on the attention
 * probabilities, 3 l + 2 after attention.output.dense (+ bias), 3 l + 3 after output.dense
 * (+ bias), the last two before the residual add.  Site 3 l + 1 has rate attn_dropout and one draw
 * per (sequence b, head): the probability row of position 0 is the single value 1, so
 * ctx[b, head] = keep v[b, head] / (1 - attn_dropout).  The others have rate hidden_dropout and one
 * draw per (sequence b, column).  With mix32 the 32-bit mixer
 *   x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16   (mod 2^32),
 * a draw is
 *   hash(seed, site, b, j) = mix32(mix32(mix32(b ^ lo32(seed)) ^ (site * 0x9E3779B9 + hi32(seed)))
 *                                  ^ (j * 0x85EBCA6B)),      j = the column, or the head,
 * the value is kept iff hash >= thr, thr = floor(p * 2^32 + 0.5) with the fp32 rate p taken to
 * double, and a kept value is multiplied by the fp32 quotient 1.0f / (1.0f - p).  p = 0 keeps
 * everything with scale exactly 1.  The backward regenerates the masks; none is stored.
 *
 * Backward.  dz = (softmax - onehot(y)) / B per sequence (a label outside [0, out_feats) gives a
 * zero row and sets BGCN_STATUS_SEQUENCE); d fc_w = dz^T pooled and d fc_b = the column sums of dz
 * over the sequences in order; through tanh and the pooler; then per layer from the last down:
 * LayerNorm backward (one wave per row), the dropout mask, output.dense, GELU' (erf form),
 * intermediate.dense, the second LayerNorm backward with the residual adds, attention.output.dense,
 * the per-head mask, value; then the embeddings' LayerNorm.  Weight gradients dW = dY^T X reduce
 * over the B rows in a fixed order, bias and LayerNorm gradients are fixed-order column sums.
 *   - every layer's d q_w, d q_b, d k_w, d k_b are written as zeros (not skipped);
 *   - d_pos_emb [max_pos, hidden] and d_type_emb [2, hidden] (both rows: the gradient buffer covers
 *     the whole token_type_embeddings tensor) hold the column sums over the sequences of the
 *     embeddings' gradient in row 0 and zeros elsewhere;
 *   - dx [N, ldx] (optional): the hidden columns of the sequences' first rows hold their gradient,
 *     the hidden columns of every other row zeros; columns past hidden are not written.
 * The gradient buffers are written whole, never accumulated into.  Deterministic: no float
 * atomics, every sum in a fixed order; two calls on the same inputs give the same bits.
 *
 * Validity: as bgcn_bert_eval (*status; a fault in seq_start or a length empties every sequence, a
 * bad label adds no loss and no gradient).  *skip_flag is 1.0f when *status is non-zero after the
 * forward, else 0.0f: the optimiser's skip flag (bgcn_adam_multi_step).  A faulted batch reads and
 * writes nothing out of bounds and still writes every gradient buffer whole; its gradients are not
 * to be used.
 *
 * BGCN_EINVAL before any HIP call: bgcn_bert_eval's conditions, a non-NULL hidden_out / hidden_sum
 * / attn_sum, a null y / gradient pointer / skip_flag, a gradient or dx not 16-byte aligned, a
 * dropout rate outside [0, 1), "workspace too small" (bgcn_bert_train_workspace_size; 0 for an
 * unsupported shape).
 * -------------------------------------------------------------------------- */
typedef struct bgcn_bert_train_args {
  bgcn_bert_args fwd;            /* y required; hidden_out, hidden_sum, attn_sum NULL */
  float* d_pos_emb;              /* [max_pos, hidden]                         */
  float* d_type_emb;             /* [2, hidden]                               */
  float* d_emb_ln_w;             /* [hidden]                                  */
  float* d_emb_ln_b;
  float* d_pooler_w;             /* [hidden, hidden]                          */
  float* d_pooler_b;
  float* d_fc_w;                 /* [C, hidden]                               */
  float* d_fc_b;
  bgcn_bert_layer d_layer[BGCN_BERT_MAX_LAYERS];   /* written through: the gradients' buffers */
  float* dx;                     /* [N, ldx] (fwd.ldx), or NULL               */
  float* skip_flag;              /* [1]                                       */
  uint64_t drop_seed;
  float hidden_dropout;          /* sites 0, 3 l + 2, 3 l + 3                 */
  float attn_dropout;            /* sites 3 l + 1                             */
} bgcn_bert_train_args;
size_t bgcn_bert_train_workspace_size(int64_t num_nodes, int64_t num_seqs, int64_t hidden, int64_t intermediate,
                                      int64_t num_layers);
int bgcn_bert_train_grad(const bgcn_bert_train_args* args, void* workspace, size_t workspace_bytes,
                         bgcn_stream_t stream);

/* --------------------------------------------------------------------------
 * bf16 weight images and the skinny-M split-K GEMM that reads them; the TreeBERT root-only
 * evaluation on them.  Additive entry points: BGCN_ABI_VERSION is unchanged.
 *
 * The root-only chain of bgcn_bert_eval is [B, hidden] GEMMs whose cost is reading each weight
 * once; a 128-column block tile gives such a product 6 - 24 workgroups.  Here the weights are kept
 * as bf16 images (half the bytes) and K is split over waves and workgroups, so that a 768 x 768
 * product already is 288 workgroups.  Opt-in: the rounding of the weights moves logp by up to
 * 1.5e-2 on the project's test cases, and a split sum has other fp32 bits than bgcn_gemm_xwt's.
 *
 * Image.  bgcn_w16_pack rounds W [Nc, K] (fp32, row stride ldw >= K) to bf16, to nearest even -
 * the bits of torch's .to(torch.bfloat16) - and stores it tiled in the operand order of
 * v_mfma_f32_32x32x16_bf16 (32 columns x 16 k = 1 KB per tile, the k-tiles of a column tile
 * consecutive).  The layout is the library's; bgcn_w16_image_size gives the bytes (0 for an
 * unsupported shape: Nc and K multiples of 64 in [64, 4096]).  image: 16-byte aligned.
 *
 * bgcn_gemm_xwt_w16: Y[M, Nc] = X[M, K] . W16[Nc, K]^T (+ bias[Nc]) for any M >= 1.  The bf16
 * weight is an exact MFMA operand, the fp32 activation is split into three bf16 planes, three
 * products per k-step, fp32 accumulate: given the rounded weights the product is fp32-grade.  The
 * four waves of a workgroup take different k-slices of one 32-column tile and add their
 * accumulators through LDS in wave order; each workgroup writes one partial into the workspace and
 * a second launch adds the partials in order, then the bias.  The split is a function of (Nc, K)
 * alone, so a row's bits do not depend on the other rows of the call.  No float atomics: two calls
 * give the same bits.  Nothing but Y's M x Nc elements and the workspace is written.  X and Y: 16-
 * byte aligned rows (ldx % 4, ldy % 4); bias: 16-byte aligned or NULL.
 *
 * bgcn_bert_eval_w16: bgcn_bert_eval's root-only form with the value, attention-output,
 * intermediate and output products of every layer and the pooler's read from images (packed from
 * v_w, ao_w, i_w, o_w and pooler_w); the partials are added by the row kernel that follows.  The
 * embeddings, biases, LayerNorm parameters and fc stay fp32 and come from `base`, which is checked
 * as bgcn_bert_eval checks it and must have hidden_out, hidden_sum and attn_sum NULL; the q and k
 * weights are never read.  Validity (*status) is bgcn_bert_eval's.
 *
 * BGCN_EINVAL before any HIP call: bgcn_bert_eval's conditions, a non-NULL hidden_out / hidden_sum
 * / attn_sum, "null or unaligned weight image", "workspace too small"
 * (bgcn_bert_w16_workspace_size; 0 for an unsupported shape).
 * -------------------------------------------------------------------------- */
size_t bgcn_w16_image_size(int64_t Nc, int64_t K);
int bgcn_w16_pack(const float* W, int64_t ldw, int64_t Nc, int64_t K, void* image, bgcn_stream_t stream);
size_t bgcn_gemm_xwt_w16_workspace_size(int64_t M, int64_t Nc, int64_t K);
int bgcn_gemm_xwt_w16(const float* X, int64_t ldx, const void* image, const float* bias, float* Y, int64_t ldy,
                      int64_t M, int64_t Nc, int64_t K, void* workspace, size_t workspace_bytes,
                      bgcn_stream_t stream);
typedef struct bgcn_bert_w16_args {
  bgcn_bert_args base;           /* hidden_out, hidden_sum, attn_sum NULL     */
  const void* v_w16[BGCN_BERT_MAX_LAYERS];    /* images of layer[l].v_w  [hidden, hidden]        */
  const void* ao_w16[BGCN_BERT_MAX_LAYERS];   /*           layer[l].ao_w [hidden, hidden]        */
  const void* i_w16[BGCN_BERT_MAX_LAYERS];    /*           layer[l].i_w  [intermediate, hidden]  */
  const void* o_w16[BGCN_BERT_MAX_LAYERS];    /*           layer[l].o_w  [hidden, intermediate]  */
  const void* pooler_w16;                     /*           pooler_w      [hidden, hidden]        */
} bgcn_bert_w16_args;
size_t bgcn_bert_w16_workspace_size(int64_t num_seqs, int64_t hidden, int64_t intermediate, int64_t num_layers);
int bgcn_bert_eval_w16(const bgcn_bert_w16_args* args, void* workspace, size_t workspace_bytes,
                       bgcn_stream_t stream);

/* --------------------------------------------------------------------------
 * Skinny-M split GEMMs on fp32 weights, and TreeBERT's training call on them.  Additive entry
 * points: BGCN_ABI_VERSION is unchanged.
 *
 * The chain of bgcn_bert_train_grad is [B, hidden] GEMMs against weights that the optimiser
 * rewrites at every step, so an image of them (above) is stale at once.  These three products read
 * the weight W [Nc, K] row-major as the parameter tensor stores it (row stride ldw), fp32 in and
 * out, and split the work until a 768 x 768 weight is 288 workgroups:
 *   bgcn_gemm_xwt_skinny   Y[M, Nc] = X[M, K] . W^T (+ bias[Nc]);  K is split into S slices
 *   bgcn_gemm_xw_skinny    Y[M, K]  = G[M, Nc] . W;                the rows of W are split into S
 *   bgcn_gemm_tn_skinny    dW[Nc, K] = G[M, Nc]^T . X[M, K];       one wave per 32 x 64 tile of dW,
 *                          the M rows in ascending order, no split and no workspace
 * The first two write S partials [S][M][width] into the workspace; a second launch adds them in
 * slice order, then the bias.  S is a function of (Nc, K) alone (the largest slice that leaves at
 * least 256 workgroups), never of M: row r of Y has the same bits whatever other rows the call
 * holds.  Arithmetic: v_mfma_f32_32x32x2_f32, fp32 operands and accumulator (an fmaf chain per
 * element): nothing is rounded but the sums, integer operands give exact results.  No float atomics:
 * two calls give the same bits.  Nothing but the output's elements and the workspace is written.
 *
 * Shapes: M >= 1, Nc and K multiples of 64 in [64, 4096].  Every matrix: non-null, 16-byte aligned,
 * row stride a multiple of 4 and at least the row width; bias 16-byte aligned or NULL.  workspace:
 * 16-byte aligned, bgcn_gemm_skinny_workspace_size(M, Nc, K) bytes (one figure for both split
 * products of a weight [Nc, K]; 0 for an unsupported shape).
 *
 * bgcn_bert_train_grad_skinny: bgcn_bert_train_grad with its products (value, attention.output,
 * intermediate, output and the pooler, forward and both backward products of each) on the kernels
 * above.  Same argument struct, same contract - validity, *skip_flag, *status, the dropout hash and
 * sites, exact-zero q / k gradients, every buffer written whole, deterministic - with one
 * exception: a split sum has other fp32 bits than bgcn_gemm_xwt's, so the forward is within fp32
 * rounding of bgcn_bert_eval's, not bit for bit.  The workspace is its own
 * (bgcn_bert_train_skinny_workspace_size; 0 for an unsupported shape).
 *
 * BGCN_EINVAL before any HIP call: an unsupported shape, a null or unaligned pointer, ld % 4 != 0,
 * ld below the row width, "workspace too small"; for the training call bgcn_bert_train_grad's
 * conditions.
 * -------------------------------------------------------------------------- */
size_t bgcn_gemm_skinny_workspace_size(int64_t M, int64_t Nc, int64_t K);
int bgcn_gemm_xwt_skinny(const float* X, int64_t ldx, const float* W, int64_t ldw, const float* bias, float* Y,
                         int64_t ldy, int64_t M, int64_t Nc, int64_t K, void* workspace, size_t workspace_bytes,
                         bgcn_stream_t stream);
int bgcn_gemm_xw_skinny(const float* G, int64_t ldg, const float* W, int64_t ldw, float* Y, int64_t ldy, int64_t M,
                        int64_t Nc, int64_t K, void* workspace, size_t workspace_bytes, bgcn_stream_t stream);
int bgcn_gemm_tn_skinny(const float* G, int64_t ldg, const float* X, int64_t ldx, float* dW, int64_t ldw, int64_t M,
                        int64_t Nc, int64_t K, bgcn_stream_t stream);
size_t bgcn_bert_train_skinny_workspace_size(int64_t num_nodes, int64_t num_seqs, int64_t hidden,
                                             int64_t intermediate, int64_t num_layers);
int bgcn_bert_train_grad_skinny(const bgcn_bert_train_args* args, void* workspace, size_t workspace_bytes,
                                bgcn_stream_t stream);

/* --------------------------------------------------------------------------
 * PHEME feature extraction: the bidirectional BERT encoder over token ids
 * (Process/getPHEMEgraph.py:104-118) for a whole tree of tweets as one launch sequence: no host
 * round trip, no allocation (everything lives in the caller's workspace).  Additive entry points:
 * BGCN_ABI_VERSION is unchanged.
 *
 * The model is a plain BertModel in eval mode: not a decoder and no attention mask, so every one of
 * the seq_len positions of a sequence, padding included, attends to every other.  Sequence b is the
 * row b of input_ids [num_seqs, seq_len] (int64), its token t at position t, row b seq_len + t of
 * every [num_seqs seq_len, .] matrix below:
 *   embeddings  h = LN(word_embeddings[id] + token_type_embeddings[0] + position_embeddings[t])
 *               (biased variance, eps = ln_eps): model.embeddings(input_ids), the array x / root
 *   per layer   q, k, v = Linear(h); per head (width 64): P = softmax(q k^T / 8) over all seq_len
 *               keys, ctx = P v;  a = LN(dense(ctx) + h);  o = LN(dense2(gelu(dense1(a))) + a),
 *               gelu(x) = x 0.5 (1 + erf(x / sqrt 2))
 *   cls         tanh(pooler.dense(o_last[0])): model(input_ids).pooler_output
 * Arithmetic: fp32 throughout, the GEMMs of bgcn_bert_eval (which change kernel at 8192 rows: the
 * results of two calls with another num_seqs seq_len agree within fp32 rounding, not bit for bit).
 * Attention is one pass over the key tiles with a running maximum and a rescaled sum, on the fp32
 * MFMA; keys past seq_len in the last tile add exactly 0 to the normaliser and to ctx.
 * Deterministic: no float atomics, fixed summation orders.
 *
 * The last layer.  pooler_output reads row 0 of the last layer's output only, so by default
 * (last_layer_full == 0) the last layer runs k | v over all rows and q, the attention of query 0,
 * the attention-output dense, the intermediate and output GEMMs and both LayerNorms on the
 * [num_seqs, hidden] first rows alone: exact, and 10/12 of that layer's GEMM work less.
 * last_layer_full != 0 runs the last layer on every row; hidden_out (last_hidden_state) needs it.
 * embed_only != 0: the embeddings alone (required then), no encoder layer; cls may be NULL and no
 * workspace is read.
 *
 * Validity is decided on the device.  *status is zeroed by the call; a token id outside [0, vocab)
 * sets BGCN_STATUS_TOKEN and is clamped into range before any read, so a flagged call stays in
 * bounds and finite (the flagged sequence's results are not to be used; the other sequences' are
 * unchanged).
 *
 * BGCN_EINVAL before any HIP call: bgcn_bert_eval's limits on hidden, heads, intermediate and
 * num_layers with num_seqs seq_len rows and num_seqs <= 65535 ("unsupported shape";
 * bgcn_bert_encode_workspace_size returns 0 for these), seq_len outside [1, max_pos] or max_pos
 * over 512, vocab < 1, a null or not 16-byte aligned weight or output (ld_embeddings % 4 != 0 or
 * below hidden), hidden_out with last_layer_full == 0, "workspace too small".
 * -------------------------------------------------------------------------- */
#define BGCN_STATUS_TOKEN 0x200   /* 512: the bit after BGCN_STATUS_SEQUENCE */
typedef struct bgcn_bert_encode_args {
  const int64_t* input_ids;      /* [num_seqs, seq_len]                       */
  int64_t num_seqs;
  int64_t seq_len;
  int64_t vocab;                 /* rows of word_emb                          */
  int64_t hidden;                /* 64 heads                                  */
  int64_t heads;
  int64_t intermediate;
  int64_t num_layers;
  int64_t max_pos;               /* rows of pos_emb                           */
  float ln_eps;
  int32_t reserved;
  const float* word_emb;         /* [vocab, hidden]                           */
  const float* pos_emb;          /* [max_pos, hidden]                         */
  const float* type_emb;         /* [hidden]: token_type_embeddings row 0     */
  const float* emb_ln_w;         /* [hidden]                                  */
  const float* emb_ln_b;
  bgcn_bert_layer layer[BGCN_BERT_MAX_LAYERS];
  const float* pooler_w;         /* [hidden, hidden]                          */
  const float* pooler_b;
  float* embeddings;             /* [num_seqs seq_len, ld_embeddings], or NULL */
  int64_t ld_embeddings;
  float* cls;                    /* [num_seqs, hidden] pooler_output          */
  float* hidden_out;             /* [num_seqs seq_len, hidden] last_hidden_state, or NULL */
  int32_t* status;               /* [1]                                       */
  int32_t last_layer_full;       /* != 0: the last layer on every row         */
  int32_t embed_only;            /* != 0: embeddings only, no encoder layer   */
} bgcn_bert_encode_args;
size_t bgcn_bert_encode_workspace_size(int64_t num_seqs, int64_t seq_len, int64_t hidden, int64_t intermediate,
                                       int64_t num_layers, int last_layer_full);
int bgcn_bert_encode(const bgcn_bert_encode_args* args, void* workspace, size_t workspace_bytes,
                     bgcn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* BGCN_H_ */
