// Batch preparation of the sparse-feature path (see bgcn_sparse.hip): the fused step's
// weight-independent work on one batch as merged launches.
#include <cstdlib>
#include <cstring>

#include "bgcn_compact_body.h"
#include "bgcn_csc_body.h"
#include "bgcn_drop_body.h"
#include "bgcn_graph_body.h"
#include "bgcn_internal.h"
#include "bgcn_items_body.h"
#include "bgcn_sparse.h"

namespace bgcn {
namespace {

// ---------------------------------------------------------------- batch preparation
// The fused step's weight-independent preparation of one batch (bgcn_prepare_batch /
// the next batch on the side lane) as six launches of 256-thread blocks, each carrying
// the independent steps of three chains side by side (a lone launch on a lane costs
// ~5 us however little it does):
//   A  zero the K1 counters | node -> root map, tree pointers, flag reset | DropEdge bounds
//   B  DropEdge select | tree work items | the pass over X (ELL compaction)
//   C  K1 count | CSC column histograms
//   D  K1 scan (decoupled look-back) | CSC per-column prefixes
//   E  K1 fill + self loops + D^-1/2 | CSC column starts
//   F  K1 normalisation + plans | CSC placement
struct PrepArgs {
  SparseState S;
  GraphBatch gb;
  DropList dl[2];
  const int64_t *batch, *rootindex;
  int32_t *node_root, *tree_ptr, *status;
  const void* X;
  int64_t ldx;
  const int32_t *xr_ptr, *xr_col;   // host-fed compacted features (X == nullptr), else null
  const float* xr_val;
  uint64_t* span;                   // device span stamps of the launch (timing class 7) or null
  int64_t* eptr;
  uint64_t seed;
  uint4* zero[2];
  int nzero[2];         // 16-byte words per zero range
  int nz, nRP, nR, nbd[2], lists;
  int nsel, ncomp;
  int nce, R;
  int ntile, nprefix;
  int ne, nn, np;
};

__global__ __launch_bounds__(256) void k_prep_a(PrepArgs a) {
  int b = int(blockIdx.x);
  if (b < a.nz) {   // 16 B per thread, 4 KB per block
    const int64_t w = int64_t(b) * 256 + threadIdx.x;
    const int64_t w0 = a.nzero[0];
    if (w < w0) a.zero[0][w] = make_uint4(0u, 0u, 0u, 0u);
    else if (w - w0 < a.nzero[1]) a.zero[1][w - w0] = make_uint4(0u, 0u, 0u, 0u);
    return;
  }
  b -= a.nz;
  if (b < a.nRP) {
    prologue_batch_body(a.S, a.batch, a.rootindex, a.node_root, a.tree_ptr, b, a.nR);
    return;
  }
  b -= a.nRP;
  const int d = b < a.nbd[0] ? 0 : 1;
  drop_bounds_body(a.dl[d], d, a.batch, a.S.N, a.S.B, a.eptr, a.status, d == 0 ? b : b - a.nbd[0]);
}

template <class TX>
__device__ inline void prep_b_body(const PrepArgs& a) {
  int b = int(blockIdx.x);
  if (b < a.nsel) {   // (tree, list) blocks first: they finish beside the pass over X
    const int d = b / int(a.S.B);
    drop_select_body(a.dl[d], d, int64_t(b % int(a.S.B)), a.batch, a.S.N, a.S.B, a.seed, a.eptr, 1,
                     nullptr, a.status);
    return;
  }
  b -= a.nsel;
  if (b == 0) {
    items_body(a.S, a.tree_ptr, a.rootindex);
    return;
  }
  if (a.xr_ptr) csr_ell_body(a.S, a.xr_ptr, a.xr_col, a.xr_val, b - 1, a.ncomp);
  else compact_body<false, TX>(a.S, static_cast<const TX*>(a.X), a.ldx, nullptr, b - 1, a.ncomp);
}

// a.span (the kernel-timing hook, class 7): every block min's its start and max's its end
// into the launch's wall-clock pair - the kernel's own span, as rocprofv3 reports it
// Register budget of the pass over X (min waves per SIMD of __launch_bounds__): with fp32
// X 1.5 blocks per CU run beside the training chain, and at the pass's natural 201 (-> 208)
// VGPRs the X-window kernels (conv2 116, the aggregations 88-116, the readout 106) fit only
// on the CUs holding ONE block of the pass: conv2's waves ran on 124 of 256 CUs and started
// up to 60 us late (profiles/r05_block_trace_instep.txt).  Capping the pass (3: 168 VGPRs,
// 4: 128, no spills) lets them in everywhere, but the step got SLOWER (twitter15 474k ->
// 453k / 445k, profiles/r05_pass_regs_ab.txt): the pass then ran 158 instead of 121 us
// beside a chain that was no faster - the X window is bound by the memory system, not by
// CU room, so the pass keeps its registers.
#ifndef BGCN_PREP_B_WAVES
#define BGCN_PREP_B_WAVES 2
#endif
template <class TX>
__device__ __forceinline__ void prep_b_stamped(const PrepArgs& a) {
  if (a.span && threadIdx.x == 0 && blockIdx.x < kSpanStarts)
    a.span[blockIdx.x] = uint64_t(wall_clock64());
  prep_b_body<TX>(a);
  if (a.span) {
    __syncthreads();
    if (threadIdx.x == 0)
      atomicMax(reinterpret_cast<unsigned long long*>(a.span) + kSpanStarts + blockIdx.x % kSpanEnds,
                static_cast<unsigned long long>(wall_clock64()));
  }
}

template <class TX>
__global__ __launch_bounds__(256, BGCN_PREP_B_WAVES) void k_prep_b(PrepArgs a) {
  prep_b_stamped<TX>(a);
}

// The unpaced pass (a step's own batch with nothing to prefetch: the full grid, no chain
// beside it) is bound by its own occupancy instead: three waves per SIMD (168 VGPRs, no
// spills) drain fp32 X in 0.099 ms at Twitter15 size against 0.108 ms with two
// (profiles/prep_one_path_ab.txt).  bf16 X takes 128 registers either way.
template <class TX>
__global__ __launch_bounds__(256, 3) void k_prep_b_alone(PrepArgs a) {
  prep_b_stamped<TX>(a);
}

// The graph lane's launches of the two-lane preparation carry only their K1 / DropEdge
// roles, as kernels of their own: a merged launch is allocated the registers of its
// heaviest role (k_prep_b: the fp32 pass over X, 201 VGPRs; k_prep_f: the CSC placement,
// 234), so the DropEdge select's 256 blocks held 201 registers per wave for the ~90 us they
// run beside the pass - one block per CU that the chain's conv2 (236 registers) then could
// not share: conv2's waves started up to 60 us late in the X window
// (profiles/r05_block_trace_instep.txt).
__global__ __launch_bounds__(256) void k_prep_select(PrepArgs a) {
  const int b = int(blockIdx.x);
  if (b >= a.nsel) return;
  const int d = b / int(a.S.B);
  drop_select_body(a.dl[d], d, int64_t(b % int(a.S.B)), a.batch, a.S.N, a.S.B, a.seed, a.eptr, 1, nullptr,
                   a.status);
}

__global__ __launch_bounds__(256) void k_prep_f_graph(PrepArgs a) {
  const int per = a.ne + a.nn + a.np;
  const int b = int(blockIdx.x);
  if (b < 2 * per) graph_rank_norm_body(a.gb, a.gb.g[b / per], b % per, a.ne, a.nn);
}

__global__ __launch_bounds__(256) void k_prep_c(PrepArgs a) {
  extern __shared__ __attribute__((aligned(16))) int32_t dsm[];
  int b = int(blockIdx.x);
  if (b < 2 * a.nce) {
    graph_count_body(a.gb, a.gb.g[b / a.nce], b % a.nce);
    return;
  }
  csc_hist_body(a.S, b - 2 * a.nce, dsm);
}

__global__ __launch_bounds__(256) void k_prep_d(PrepArgs a) {
  int b = int(blockIdx.x);
  if (b < 2 * a.ntile) {
    graph_scan_body(a.gb, a.gb.g[b / a.ntile]);
    return;
  }
  csc_prefix_body(a.S, a.R, b - 2 * a.ntile);
}

__global__ __launch_bounds__(256) void k_prep_e(PrepArgs a) {
  int b = int(blockIdx.x);
  const int per = a.ne + a.nn;
  if (b < 2 * per) {
    graph_fill_nodes_body(a.gb, a.gb.g[b / per], b % per, a.ne);
    return;
  }
  csc_colscan_body(a.S);
}

#ifndef BGCN_PREP_F_WAVES
#define BGCN_PREP_F_WAVES 2   // (3 caps the CSC placement at 168 VGPRs with 85 spilled: not taken)
#endif
__global__ __launch_bounds__(256, BGCN_PREP_F_WAVES) void k_prep_f(PrepArgs a) {
  extern __shared__ __attribute__((aligned(16))) int32_t dsm[];
  int b = int(blockIdx.x);
  const int per = a.ne + a.nn + a.np;
  if (b < 2 * per) {
    graph_rank_norm_body(a.gb, a.gb.g[b / per], b % per, a.ne, a.nn);
    return;
  }
  csc_place_body(a.S, b - 2 * per, dsm);
}

}  // namespace

#ifndef BGCN_PREP_LANES_DEFAULT
#define BGCN_PREP_LANES_DEFAULT 2   // profiles/r03_chain_experiments_late.txt
#endif
void bind_prepared(const Prepared& p, SparseState& S) {
  S.item_tree = p.item_tree; S.tree_item0 = p.tree_item0;
  S.item_beg = p.item_beg; S.item_end = p.item_end; S.item_root = p.item_root;
  S.hist = p.hist; S.col_total = p.col_total; S.col_start = p.col_start; S.col_end = p.col_end;
  S.csc = p.csc;
  S.ovf_off = p.x_ovf_off; S.ovf = p.x_ovf; S.ovf_cap = p.ovf_cap; S.long_rows = p.x_long;
}

// the sparse state of a prepared batch's buffers
static void prepared_state(const Prepared& p, int64_t N, int64_t B, int64_t F, int mode, SparseState& S) {
  S.mode = mode;
  S.N = N; S.F = F; S.B = B;
  S.max_items = int(N / kChunk + B + 1);
  S.flags = p.x_flags; S.nnz = p.x_nnz; S.cols = p.x_cols; S.vals = p.x_vals;
  bind_prepared(p, S);
  S.root_map = p.node_root;
  S.bstatus = p.status;
}

int prep_pipeline(const Prepared& p, const bgcn_batch* bt, int64_t F, int degree_on, int mode,
                  hipStream_t s, bool paced, int nlanes) {
  const int64_t N = bt->num_nodes, B = bt->num_graphs;
  BGCN_CHECK_HIP(hipMemsetAsync(p.status, 0, sizeof(int32_t), s));
  PrepArgs a{};
  SparseState& S = a.S;
  prepared_state(p, N, B, F, mode, S);
  a.batch = bt->batch; a.rootindex = bt->rootindex;
  a.node_root = p.node_root; a.tree_ptr = p.tree_ptr; a.status = p.status;
  a.X = bt->x; a.ldx = bt->ldx;
  if (!bt->x) { a.xr_ptr = bt->x_row_ptr; a.xr_col = bt->x_col; a.xr_val = bt->x_val; }
  // DropEdge (dataset.py:68-90) in the masked form: dropped edges become self loops, which
  // K1 removes - the graphs of the compacted lists, no kept count on the host
  const int64_t Etd = bt->td_num_edges, Ebu = bt->bu_num_edges;
  const bool drop = bt->td_droprate > 0.0 || bt->bu_droprate > 0.0;
  const int64_t* td = bt->td_edge_index;
  const int64_t* bu = bt->bu_edge_index;
  a.lists = drop ? 2 : 0;
  if (drop) {
    BGCN_CHECK_ARG(p.dws && p.dws_bytes >= drop_ws_size(B), "drop workspace too small");
    Carve c(p.dws, p.dws_bytes);
    a.eptr = c.take<int64_t>(size_t(2 * (B + 1)));
    a.dl[0] = DropList{td, Etd, p.td_drop, Etd, bt->td_droprate, 0u};
    a.dl[1] = DropList{bu, Ebu, p.bu_drop, Ebu, bt->bu_droprate, 1u};
    a.seed = bt->drop_seed;
    if (td) td = p.td_drop;
    if (bu) bu = p.bu_drop;
  }
  GraphArgs ga[2];
  graph_pair_args(td, Etd, bu, Ebu, &p.td, &p.bu, p.status, p.gws, p.gws_bytes, ga);
  size_t zb[2] = {0, 0};
  BGCN_TRY(graph_batch_setup(ga, 2, N, degree_on, &a.gb, zb, bt->batch));
  for (int k = 0; k < 2; ++k) {
    a.zero[k] = reinterpret_cast<uint4*>(a.gb.g[k].cnt_t);
    a.nzero[k] = int(zb[k] / 16);
    BGCN_CHECK_ARG(zb[k] % 16 == 0 && (reinterpret_cast<uintptr_t>(a.zero[k]) & 15) == 0, "zero range");
  }
  const bool xp = mode != 1;   // the pass over X and the CSC of X in these launches
  const int64_t Emax = std::max(Etd, Ebu);
  a.nz = int((a.nzero[0] + a.nzero[1] + 255) / 256);
  a.nR = int((N + 255) / 256);
  a.nRP = a.nR + int((B + 1 + 255) / 256);
  a.nbd[0] = drop ? int(Etd / 256 + 1) : 0;
  a.nbd[1] = drop ? int(Ebu / 256 + 1) : 0;
  a.nsel = drop ? int(2 * B) : 0;
  {   // The pass over X is paced: with fp32 X 1.5 4-wave blocks per CU stride over the
      // rows (~30 MB of loads in flight, ~4.5 TB/s).  A wave per row over all rows drains
      // X at 5.5 TB/s but floods the memory queues with ~100 MB of requests, and every
      // load of the latency-bound training chain beside it then waits behind them:
      // measured 0.293-0.295 ms per step paced vs 0.303-0.306 unpaced (twitter15; 224-288
      // blocks within 1%, 512 worse than either).  With the shorter chain of 512-thread
      // aggregation / tail blocks, 384 blocks: 0.2964-0.2966 vs 0.304-0.308 at 256
      // (profiles/r02_pace_ab.txt).  bf16 X (the prefix compaction, compact_by_prefix):
      // one block per CU - 192 / 256 / 320 / 512 / 1024 blocks / the full grid: weibo_bf16
      // 0.667 / 0.646 / 0.661 / 0.709 / 0.688 / 0.697 ms (profiles/r02_compact_ab.txt).
      // Not paced (a step's own batch with nothing to prefetch: no chain runs beside the
      // pass): the full grid.  BGCN_PREP_BLOCKS (read per call) overrides either: 0 = full
      // grid, n = n blocks.
    static const int ncu = [] {
      int dev = 0, n = 0;
      if (hipGetDevice(&dev) != hipSuccess ||
          hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        n = 256;
      return n > 0 ? n : 256;
    }();
    const bool bf = bt->x_dtype == BGCN_DTYPE_BF16;
    a.ncomp = xp ? int(grid_for(N, bf ? 8 : 4)) : 0;
    const int paced_cap = bf ? (compact_by_prefix<bf16_t>() ? ncu : 0) : ncu + ncu / 2;
    const int cap = int(knob("BGCN_PREP_BLOCKS", paced ? paced_cap : 0));
    if (cap > 0) a.ncomp = std::min(a.ncomp, cap);
    // host-fed compacted rows: 8 rows per block over every row, nothing to pace (nnz x 8 B)
    if (a.xr_ptr && xp) a.ncomp = int(grid_for(N, 8));
  }
  a.nce = graph_edge_blocks(Emax);
  a.R = xp ? int((N + kRowBlock - 1) / kRowBlock) : 0;
  a.ntile = int(graph_scan_tiles(N));
  a.nprefix = xp ? int(grid_for(F, kPrefixCols)) : 0;
  a.ne = graph_edge_blocks(Emax);
  a.nn = graph_node_blocks(N);
  a.np = graph_pos_blocks(Emax, N);
  const dim3 blk(256);
  const bool bf16 = bt->x_dtype == BGCN_DTYPE_BF16;
  void (*const prep_b)(PrepArgs) = paced ? (bf16 ? k_prep_b<bf16_t> : k_prep_b<float>)
                                         : (bf16 ? k_prep_b_alone<bf16_t> : k_prep_b_alone<float>);
  hipLaunchKernelGGL(k_prep_a, dim3(unsigned(a.nz + a.nRP + a.nbd[0] + a.nbd[1])), blk, 0, s, a);
  BGCN_CHECK_LAUNCH();
  const size_t hist_smem = xp ? size_t(F) * sizeof(int32_t) : 0;
  // Two lanes (the default; BGCN_PREP_LANES=1, read once, keeps one): DropEdge select + K1
  // run on a second lane beside the pass over X, and the CSC of X follows the pass on the
  // side lane - the roles of each merged launch split by chain.  K1's four latency-bound
  // launches then overlap the X window, where the chain is stalled anyway, instead of the
  // chain's second half: twitter15 0.2691-0.2724 vs 0.2732-0.2749 ms per step over five
  // interleaved rounds, synth1024_bf16 -0.7 %, weibo_bf16 within its noise (+0.5 %)
  const int default_lanes = int(BGCN_KNOB_ONCE("BGCN_PREP_LANES", BGCN_PREP_LANES_DEFAULT));
  const int lanes = nlanes > 0 ? nlanes : default_lanes;
  if (lanes == 2 && xp) {
    hipStream_t g = s;
    BGCN_TRY(aux_fork(s, kLaneGraph, &g));
    PrepArgs ag = a;           // graph chain: DropEdge select, K1 count / scan / fill / norm
    ag.ncomp = 0; ag.R = 0; ag.nprefix = 0;
    PrepArgs ax = a;           // X chain: tree items, the pass over X, the CSC of X
    ax.nsel = 0; ax.nce = 0; ax.ntile = 0; ax.ne = 0; ax.nn = 0; ax.np = 0;
    if (ag.nsel > 0) {
      hipLaunchKernelGGL(k_prep_select, dim3(unsigned(ag.nsel)), blk, 0, g, ag);
      BGCN_CHECK_LAUNCH();
    }
    if (ag.nce > 0) hipLaunchKernelGGL(k_prep_c, dim3(unsigned(2 * ag.nce)), blk, 0, g, ag);
    if (ag.ntile > 0) hipLaunchKernelGGL(k_prep_d, dim3(unsigned(2 * ag.ntile)), blk, 0, g, ag);
    if (ag.ne + ag.nn > 0) hipLaunchKernelGGL(k_prep_e, dim3(unsigned(2 * (ag.ne + ag.nn))), blk, 0, g, ag);
    if (ag.ne + ag.nn + ag.np > 0)
      hipLaunchKernelGGL(k_prep_f_graph, dim3(unsigned(2 * (ag.ne + ag.nn + ag.np))), blk, 0, g, ag);
    BGCN_CHECK_LAUNCH();
    timing_begin(7, s);
    ax.span = span_slot(7);
    hipLaunchKernelGGL(prep_b, dim3(unsigned(1 + ax.ncomp)), blk, 0, s, ax);
    BGCN_CHECK_LAUNCH();
    timing_end(7, s);
    hipLaunchKernelGGL(k_prep_c, dim3(unsigned(ax.R)), blk, hist_smem, s, ax);
    hipLaunchKernelGGL(k_prep_d, dim3(unsigned(ax.nprefix)), blk, 0, s, ax);
    hipLaunchKernelGGL(k_prep_e, dim3(1u), blk, 0, s, ax);
    hipLaunchKernelGGL(k_prep_f, dim3(unsigned(ax.R)), blk, 2 * hist_smem, s, ax);
    BGCN_CHECK_LAUNCH();
    BGCN_TRY(aux_join(s, kLaneGraph));
    return BGCN_OK;
  }
  timing_begin(7, s);
  a.span = span_slot(7);
  hipLaunchKernelGGL(prep_b, dim3(unsigned(a.nsel + 1 + a.ncomp)), blk, 0, s, a);
  BGCN_CHECK_LAUNCH();
  timing_end(7, s);
  if (2 * a.nce + a.R > 0) {
    hipLaunchKernelGGL(k_prep_c, dim3(unsigned(2 * a.nce + a.R)), blk, hist_smem, s, a);
    BGCN_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_prep_d, dim3(unsigned(2 * a.ntile + a.nprefix)), blk, 0, s, a);
  BGCN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_prep_e, dim3(unsigned(2 * (a.ne + a.nn) + (xp ? 1 : 0))), blk, 0, s, a);
  BGCN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_prep_f, dim3(unsigned(2 * (a.ne + a.nn + a.np) + a.R)), blk, 2 * hist_smem, s, a);
  BGCN_CHECK_LAUNCH();
  return BGCN_OK;
}

}  // namespace bgcn
