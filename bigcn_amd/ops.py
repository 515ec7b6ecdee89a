"""Autograd operators over the HIP kernels of libbgcn (the hot path of BiGCN).

* :class:`Graph` / :func:`build_graph` - ``gcn_norm`` + ``add_remaining_self_loops`` +
  CSR (K1), built once per batch and direction, shared by conv1/conv2 forward and
  backward (the reference recomputes it 4x per step, ``cached=False``).
* :func:`gcn_conv` - PyG-2.x ``GCNConv.forward`` (lin -> propagate -> +bias) with a
  HIP backward (K2, K3, K4, K10).
* :func:`scatter_mean` - ``torch_scatter.scatter_mean`` (K8).
* :func:`edge_infer` / :func:`ebgcn_conv2_lin` - what EBGCN's eval forward adds
  (``model/Twitter/EBGCN.py:72-116``): the edge-inference kernel and conv2's lin over the
  BatchNorm'd concat.
* :func:`edge_infer_train` - the same edge inference in training mode (``EBGCN.py:95-116``):
  batch-statistics BatchNorm, the Bayesian branch, the KL edge loss and the backward.
* :func:`ebgcn_conv2_lin_train` / :func:`gcn_aggregate` - conv2 of the training forward
  (``EBGCN.py:72-84``): batch-statistics bn1 + relu + conv2's lin and their backward without the dense
  concat, then the aggregation half of :func:`gcn_conv`.
* :func:`explain_sums` / :func:`segment_rank` - the reference's analysis (``explain_PHEME.py``):
  per-node stage sums without the concat, and a batched per-tree ``topk(k = n)``.
* :func:`tree_centrality` / :func:`rank_similarity` - the reference's comparison
  (``compare_similarity.py``): the trees' graph centralities and the per-tree similarity
  statistics of every pair of rankings.
* :func:`bigcn_encoder` - the fused TD+BU encoder of ``BiGCN.forward``
  (``model/Twitter/BiGCN_Twitter.py:125-128``), all of K1-K10 on the GPU.

Every function runs on the caller's current HIP stream and never falls back to a
CPU or PyTorch implementation.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _lib
from ._lib import BatchDesc, BiGCNArgs, GraphView, check, ptr, stream_handle, workspace

HID = 64


def _dev_check(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.BGCNError("bigcn_amd ops take device tensors (no CPU path)")


# ----------------------------------------------------------------------------- K1
_GRAPH_I32 = ("t_ptr", "s_ptr", "t_row", "t_col", "s_row", "s_col")
_GRAPH_F32 = ("t_w", "s_w")
_SEG_ALIGN = 64   # elements: every array starts 256-byte aligned inside its buffer


class Graph:
    """Normalised adjacency of one direction in both CSR orientations.

    ``t_*`` rows are targets (forward aggregation, ``out[i] = sum norm * h[src]``),
    ``s_*`` rows are sources (the transposed product of the backward pass).  The arrays
    live in two flat buffers (int32 / fp32, shared by the TD and BU graphs of a pair);
    the per-array tensors are views made on first access - the kernels take pointers."""

    __slots__ = ("num_nodes", "num_edges", "capacity", "status", "_bufs", "_lay", "_views", "_ptrs", "_plan",
                 "_plan_ws", "_tree_checked")

    def _array(self, name: str) -> torch.Tensor:
        v = self._views.get(name)
        if v is None:
            k, off, n = self._lay[name]
            v = self._bufs[k].narrow(0, off, n)
            self._views[name] = v
        return v

    def view(self) -> GraphView:
        v = GraphView()
        q = self._ptrs
        v.t_ptr, v.t_row, v.t_col, v.t_w = q["t_ptr"], q["t_row"], q["t_col"], q["t_w"]
        v.s_ptr, v.s_row, v.s_col, v.s_w = q["s_ptr"], q["s_row"], q["s_col"], q["s_w"]
        v.capacity = self.capacity
        if self._plan is not None:   # the aggregation plans of bgcn_build_graph_pair
            v.plan[0], v.plan[1] = self._plan
        if self._tree_checked:       # built with the batch vector: status carries BGCN_STATUS_CROSS_TREE
            v.tree_status = self.status.data_ptr()
        return v

    def check(self) -> None:
        """Host sync: raise IndexError if edge_index held an index outside [0, N)."""
        s = int(self.status.item())
        if s & 8:
            raise RuntimeError("libbgcn: an internal cross-workgroup hand-off timed out")
        if s & ~_lib.BGCN_STATUS_CROSS_TREE:   # (an edge across trees is legal, only noted)
            raise IndexError("edge_index contains an index out of range [0, num_nodes)")


for _name in _GRAPH_I32 + _GRAPH_F32:
    setattr(Graph, _name, property(lambda self, _n=_name: self._array(_n)))


def _seg(n: int) -> int:
    return (n + _SEG_ALIGN - 1) // _SEG_ALIGN * _SEG_ALIGN


def _alloc_graphs(edges, N: int, dev, status=None):
    """Graphs of E = edges[k] edges over N nodes, all arrays carved from one int32 and
    one fp32 allocation."""
    ni = sum(2 * _seg(N + 1) + 4 * _seg(E + N) for E in edges)
    nf = sum(2 * _seg(E + N) for E in edges)
    bi = torch.empty(ni, dtype=torch.int32, device=dev)
    bf = torch.empty(nf, dtype=torch.float32, device=dev)
    pi, pf = bi.data_ptr(), bf.data_ptr()
    st = torch.zeros(1, dtype=torch.int32, device=dev) if status is None else status
    out, oi, of = [], 0, 0
    for E in edges:
        cap = E + N
        g = Graph()
        g.num_nodes, g.num_edges, g.capacity, g.status = N, E, cap, st
        g._bufs, g._views, g._lay, g._ptrs = (bi, bf), {}, {}, {}
        g._plan = g._plan_ws = None
        g._tree_checked = False
        for name in _GRAPH_I32:
            n = N + 1 if name.endswith("ptr") else cap
            g._lay[name], g._ptrs[name] = (0, oi, n), pi + 4 * oi
            oi += _seg(n)
        for name in _GRAPH_F32:
            g._lay[name], g._ptrs[name] = (1, of, cap), pf + 4 * of
            of += _seg(cap)
        out.append(g)
    return out


def _alloc_graph(E: int, N: int, dev, status=None) -> Graph:
    return _alloc_graphs((E,), N, dev, status)[0]


def _csr_out(g: Graph) -> _lib.CsrOut:
    c = _lib.CsrOut()
    q = g._ptrs
    c.t_ptr, c.t_row, c.t_col, c.t_w = q["t_ptr"], q["t_row"], q["t_col"], q["t_w"]
    c.s_ptr, c.s_row, c.s_col, c.s_w = q["s_ptr"], q["s_row"], q["s_col"], q["s_w"]
    return c


def degree_code(degree_on: str) -> int:
    """C-ABI code of a gcn_norm degree convention: 'col' (PyG >= 1.6: target degree) -> 0,
    'row' (PyG 1.3.2: source degree) -> 1; anything else raises."""
    if degree_on == "col":
        return 0
    if degree_on == "row":
        return 1
    raise ValueError(f"degree_on must be 'col' or 'row', got {degree_on!r}")


def _i64c(t: torch.Tensor) -> torch.Tensor:
    """An index tensor as the kernels read it: int64 and contiguous, else converted."""
    if t.dtype == torch.int64 and t.is_contiguous():
        return t
    return t.to(torch.int64).contiguous()


def _check_ei(edge_index: torch.Tensor) -> torch.Tensor:
    if edge_index.dim() != 2 or edge_index.size(0) != 2:
        raise ValueError("edge_index must be [2, E]")
    return _i64c(edge_index)


def build_graph_pair(td_edge_index: torch.Tensor, bu_edge_index: torch.Tensor, num_nodes: int,
                     degree_on: str = "col", validate: bool = False, batch: Optional[torch.Tensor] = None):
    """TD and BU graphs of one batch in one launch sequence (the fused step's K1).  The
    build's workspace (≈3.5 MB at Twitter size, about the graphs' own size) stays with the
    two graphs: it holds their aggregation plans (``bgcn_graph_pair_plans``).

    ``batch`` (the collated batch vector, optional): the build also notes on the device
    whether an edge joins two trees.  Only graphs built with it let the fused encoder take
    its sign-word readout backward (which handles such edges by per-neighbour scales);
    without it the encoder keeps the general readout backward."""
    _dev_check(td_edge_index, bu_edge_index, batch)
    if batch is not None:
        if batch.numel() != int(num_nodes):
            raise ValueError("batch must have one entry per node")
        batch = batch.to(torch.int64).contiguous()
    dcode = degree_code(degree_on)
    td_ei, bu_ei = _check_ei(td_edge_index), _check_ei(bu_edge_index)
    N = int(num_nodes)
    dev = td_ei.device
    td, bu = _alloc_graphs((int(td_ei.size(1)), int(bu_ei.size(1))), N, dev)
    L = _lib.lib()
    ws = workspace(L.bgcn_graph_pair_workspace_size(td.num_edges, bu.num_edges, N), dev)
    a, b = _csr_out(td), _csr_out(bu)
    check(L.bgcn_build_graph_pair(td_ei.data_ptr(), td.num_edges, bu_ei.data_ptr(), bu.num_edges, N,
                                  dcode, ctypes.byref(a), ctypes.byref(b), ptr(batch),
                                  td.status.data_ptr(), ws.data_ptr(), ws.numel(), stream_handle()))
    td._tree_checked = bu._tree_checked = batch is not None
    # the build leaves both graphs' aggregation plans in its workspace: keep it with the
    # graphs so the fused encoder takes the planned aggregation
    pt, pb = (_lib.SpmmPlan * 2)(), (_lib.SpmmPlan * 2)()
    check(L.bgcn_graph_pair_plans(ws.data_ptr(), ws.numel(), td.num_edges, bu.num_edges, N,
                                  ctypes.addressof(pt), ctypes.addressof(pb)))
    td._plan, bu._plan = (pt[0], pt[1]), (pb[0], pb[1])
    td._plan_ws = bu._plan_ws = ws
    if validate:
        td.check()
    return td, bu


def build_graph(edge_index: torch.Tensor, num_nodes: int, edge_weight: Optional[torch.Tensor] = None,
                degree_on: str = "col", validate: bool = False) -> Graph:
    _dev_check(edge_index, edge_weight)
    dcode = degree_code(degree_on)
    ei = _check_ei(edge_index)
    ew = None if edge_weight is None else edge_weight.to(torch.float32).contiguous()
    E, N = int(ei.size(1)), int(num_nodes)
    dev = ei.device
    g = _alloc_graph(E, N, dev)
    L = _lib.lib()
    ws = workspace(L.bgcn_graph_workspace_size(E, N), dev)
    check(L.bgcn_build_graph(ptr(ei), ptr(ew), E, N, dcode,
                             *(g._ptrs[n] for n in ("t_ptr", "t_row", "t_col", "t_w",
                                                    "s_ptr", "s_row", "s_col", "s_w")),
                             ptr(g.status), ptr(ws), ws.numel(), stream_handle()))
    g._plan_ws = ws   # the build's workspace: D^-1/2 (bgcn_graph_dinv) for the edge-weight gradient
    if validate:
        g.check()
    return g


def _graph_dinv(g: Graph) -> int:
    """Device pointer of the D^-1/2 vector a single-graph build left in its workspace."""
    out = ctypes.c_void_p()
    ws = g._plan_ws
    check(_lib.lib().bgcn_graph_dinv(ws.data_ptr(), ws.numel(), g.num_edges, g.num_nodes, ctypes.byref(out)))
    return int(out.value)


def drop_edges(td_edge_index: Optional[torch.Tensor], bu_edge_index: Optional[torch.Tensor],
               batch: torch.Tensor, num_graphs: int, tddroprate: float = 0.0, budroprate: float = 0.0,
               seed: int = 0, masked: bool = False):
    """DropEdge of ``Process/dataset.py:68-90`` on the device, per tree of a collated batch:
    keep a uniform random subset of exactly ``int(E_t * (1 - rate))`` edges in their
    original order (``rate <= 0`` keeps all).  TD and BU are drawn independently from
    ``seed`` (a counter-based draw, not Python's ``random`` stream).

    ``masked=False`` returns the compacted lists (one host sync for the kept counts);
    ``masked=True`` returns ``[2, E]`` lists holding, per tree, the kept edges in order
    and then every dropped edge ``(s, d)`` as the self loop ``(d, d)``, which
    :func:`build_graph` removes (no sync)."""
    ref = td_edge_index if td_edge_index is not None else bu_edge_index
    if ref is None:
        raise ValueError("drop_edges: no edge list given")
    _dev_check(td_edge_index, bu_edge_index, batch)
    td = None if td_edge_index is None else _check_ei(td_edge_index)
    bu = None if bu_edge_index is None else _check_ei(bu_edge_index)
    batch = batch.to(torch.int64).contiguous()
    N, B = int(batch.numel()), int(num_graphs)
    dev = batch.device
    td_out = None if td is None else torch.empty_like(td)
    bu_out = None if bu is None else torch.empty_like(bu)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    L = _lib.lib()
    ws = workspace(L.bgcn_drop_edges_workspace_size(B), dev)
    Etd = 0 if td is None else int(td.size(1))
    Ebu = 0 if bu is None else int(bu.size(1))
    check(L.bgcn_drop_edges(ptr(td), Etd, float(tddroprate), ptr(td_out), max(Etd, 1),
                            ptr(bu), Ebu, float(budroprate), ptr(bu_out), max(Ebu, 1), ptr(batch), N, B,
                            int(seed) & (2**64 - 1), int(masked), ptr(counts), ptr(status), ptr(ws),
                            ws.numel(), stream_handle()))
    if masked:
        return td_out, bu_out
    kept = counts.cpu()
    if int(status.item()) & 1:
        raise IndexError("drop_edges: an edge index is out of range or the edges are not "
                         "grouped by tree in batch order")
    if td_out is not None:
        td_out = td_out[:, :int(kept[0])].contiguous()
    if bu_out is not None:
        bu_out = bu_out[:, :int(kept[1])].contiguous()
    return td_out, bu_out


# ----------------------------------------------------------------------------- K3/K4
def spmm(g: Graph, x: torch.Tensor, bias: Optional[torch.Tensor] = None, relu: bool = False,
         transposed: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``out = A_hat x (+bias)`` (or ``A_hat^T x``); x [N, F] with F % 4 == 0 (computed in
    fp32: other dtypes are converted)."""
    _dev_check(x, bias)
    if x.dim() != 2 or x.size(0) != g.num_nodes:
        raise ValueError(f"x must be [num_nodes={g.num_nodes}, F]")
    N, F = x.shape
    if x.dtype != torch.float32:
        x = x.float()
    if x.stride(1) != 1:
        x = x.contiguous()
    if bias is not None:
        bias = bias.to(torch.float32).contiguous()
        if bias.numel() != F:
            raise ValueError("bias must have F elements")
    if out is None:
        out = torch.empty(N, F, dtype=torch.float32, device=x.device)
    elif out.dtype != torch.float32 or out.shape != (N, F) or out.stride(1) != 1:
        raise ValueError("out must be a row-major fp32 [N, F] tensor")
    L = _lib.lib()
    ws = workspace(L.bgcn_spmm_workspace_size(g.capacity, F), x.device)
    p = [g._ptrs[("s_" if transposed else "t_") + n] for n in ("ptr", "row", "col", "w")]
    check(L.bgcn_spmm(p[0], p[1], p[2], p[3], N, g.capacity, ptr(x), x.stride(0),
                      ptr(out), out.stride(0), F, ptr(bias), 1 if relu else 0, ptr(ws), ws.numel(),
                      stream_handle()))
    return out


def _pad4(t: torch.Tensor) -> torch.Tensor:
    """Zero-pad the last dim to a multiple of 4 (spmm works on float4 rows)."""
    F = t.size(-1)
    if F % 4 == 0:
        return t.contiguous()
    return torch.nn.functional.pad(t, (0, 4 - F % 4)).contiguous()


def _linear(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """x [N, K] . w[O, K]^T on MFMA."""
    N, K = x.shape
    O = w.size(0)
    y = torch.empty(N, O, dtype=torch.float32, device=x.device)
    check(_lib.lib().bgcn_gemm_xwt(ptr(x), x.stride(0), ptr(w), 0, w.stride(0), O, ptr(y), O, N, O, K,
                                   stream_handle()))
    return y


def _rows_ok(t: torch.Tensor) -> bool:
    """A 2-D fp32 tensor the skinny kernels read in place: unit column stride, 16-byte aligned rows."""
    return (t.dim() == 2 and t.dtype == torch.float32 and t.stride(1) == 1 and t.stride(0) % 4 == 0
            and t.stride(0) >= t.size(1) and t.data_ptr() % 16 == 0)


def _skinny_operands(what, a, b, out, out_shape):
    _dev_check(a, b, out)
    if a.dim() != 2 or b.dim() != 2:
        raise ValueError(f"{what}: the operands must be 2-D")
    a, b = (t if _rows_ok(t) else t.float().contiguous() for t in (a, b))
    if out is None:
        out = torch.empty(out_shape, dtype=torch.float32, device=a.device)
    elif tuple(out.shape) != tuple(out_shape) or not _rows_ok(out) or out.device != a.device:
        raise ValueError(f"{what}: out must be an fp32 {tuple(out_shape)} device tensor with 16-byte aligned rows")
    return a, b, out


def _skinny_workspace(what, M, Nc, K, dev):
    need = _lib.lib().bgcn_gemm_skinny_workspace_size(M, Nc, K)
    if need == 0:
        raise _lib.BGCNError(f"{what}: unsupported shape (M >= 1, Nc and K multiples of 64 in [64, 4096])")
    return workspace(need, dev)


def gemm_xwt_skinny(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``x [M, K] . w [Nc, K]^T (+ bias [Nc])`` for a few rows against a large fp32 weight read as it is
    stored (``bgcn_gemm_xwt_skinny``: K split over 256 or more workgroups, the partials added in a fixed
    order; a row's bits do not depend on ``M``).  ``Nc``, ``K``: multiples of 64 in [64, 4096].  No autograd."""
    if x.dim() == 2 and w.dim() == 2 and x.size(1) != w.size(1):
        raise ValueError("gemm_xwt_skinny: x [M, K] and w [Nc, K] must share K")
    x, w, out = _skinny_operands("gemm_xwt_skinny", x, w, out, (x.size(0), w.size(0)))
    _dev_check(bias)
    if bias is not None:
        if bias.numel() != w.size(0):
            raise ValueError("gemm_xwt_skinny: bias must have Nc elements")
        bias = bias.float().contiguous()
    M, K, Nc = x.size(0), x.size(1), w.size(0)
    ws = _skinny_workspace("gemm_xwt_skinny", M, Nc, K, x.device)
    check(_lib.lib().bgcn_gemm_xwt_skinny(ptr(x), x.stride(0), ptr(w), w.stride(0), ptr(bias), ptr(out), out.stride(0),
                                          M, Nc, K, ptr(ws), ws.numel(), stream_handle()))
    return out


def gemm_xw_skinny(g: torch.Tensor, w: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``g [M, Nc] . w [Nc, K]``, the input gradient of :func:`gemm_xwt_skinny` (``bgcn_gemm_xw_skinny``: the rows
    of ``w`` split over the workgroups).  No autograd."""
    if g.dim() == 2 and w.dim() == 2 and g.size(1) != w.size(0):
        raise ValueError("gemm_xw_skinny: g [M, Nc] and w [Nc, K] must share Nc")
    g, w, out = _skinny_operands("gemm_xw_skinny", g, w, out, (g.size(0), w.size(1)))
    M, Nc, K = g.size(0), w.size(0), w.size(1)
    ws = _skinny_workspace("gemm_xw_skinny", M, Nc, K, g.device)
    check(_lib.lib().bgcn_gemm_xw_skinny(ptr(g), g.stride(0), ptr(w), w.stride(0), ptr(out), out.stride(0), M, Nc, K,
                                         ptr(ws), ws.numel(), stream_handle()))
    return out


def gemm_tn_skinny(g: torch.Tensor, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``g [M, Nc]^T . x [M, K]``, the weight gradient of :func:`gemm_xwt_skinny` (``bgcn_gemm_tn_skinny``: one wave
    per 32 x 64 tile of the result, the ``M`` rows in ascending order).  No autograd."""
    if g.dim() == 2 and x.dim() == 2 and g.size(0) != x.size(0):
        raise ValueError("gemm_tn_skinny: g [M, Nc] and x [M, K] must share M")
    g, x, out = _skinny_operands("gemm_tn_skinny", g, x, out, (g.size(1), x.size(1)))
    check(_lib.lib().bgcn_gemm_tn_skinny(ptr(g), g.stride(0), ptr(x), x.stride(0), ptr(out), out.stride(0), g.size(0),
                                         g.size(1), x.size(1), stream_handle()))
    return out


def _aggregate(g: Graph, z: torch.Tensor, bias, O: int) -> torch.Tensor:
    """``A_hat z + b`` for z of padded width; the first O columns, contiguous."""
    b = None if bias is None else _pad4(bias.view(1, -1)).view(-1)
    return spmm(g, z, b)[:, :O].contiguous()


def _aggregate_backward(g: Graph, dout: torch.Tensor, z, ei, degree_on: str, need_bias: bool):
    """The aggregation's backward: ``(A_hat^T dout`` of padded width, ``d edge_weight`` or None, ``d bias`` or
    None``)``.  ``z`` / ``ei`` (the padded aggregation input and the edge list) are given when the edge
    weights are learned."""
    L = _lib.lib()
    N, O = dout.shape
    d = _pad4(dout.float())
    dzp = spmm(g, d, transposed=True)                       # A_hat^T dout (padded width)
    dew = db = None
    if z is not None:
        # gcn_norm's backward (EBGCN.py:84,178 learn edge_weight): row dots of
        # (dout, A_hat h) and (h, A_hat^T dout), then one dot per edge
        agg = spmm(g, z)                                     # A_hat h, no bias
        E = int(ei.size(1))
        dew = torch.empty(E, dtype=torch.float32, device=dout.device)
        ws = workspace(L.bgcn_edge_weight_grad_workspace_size(N), dout.device)
        F4 = int(z.size(1))
        check(L.bgcn_edge_weight_grad(ptr(ei), E, N, degree_code(degree_on), _graph_dinv(g), ptr(z),
                                      ptr(agg), ptr(d), ptr(dzp), F4, F4, ptr(dew), ptr(ws), ws.numel(),
                                      stream_handle()))
    if need_bias:
        db = torch.empty(O, dtype=torch.float32, device=dout.device)
        dd = dout.float().contiguous()
        ws = workspace(L.bgcn_colsum_workspace_size(N, O), dout.device)
        check(L.bgcn_colsum(ptr(dd), dd.stride(0), N, O, ptr(db), ptr(ws), ws.numel(),
                            stream_handle()))
    return dzp, dew, db


class _GCNConvFn(torch.autograd.Function):
    """PyG-2.x GCNConv: out = A_hat (x W^T) + b, A_hat = gcn_norm(edge_index, edge_weight)."""

    @staticmethod
    def forward(ctx, x, weight, bias, g: Graph, edge_index=None, edge_weight=None, degree_on="col"):
        x = x.contiguous().float()
        weight = weight.contiguous()
        z = _pad4(_linear(x, weight))
        out = _aggregate(g, z, bias, weight.size(0))
        ctx.g = g
        ctx.degree_on = degree_on
        ew_grad = edge_weight is not None and ctx.needs_input_grad[5]
        # the edge-weight gradient needs h = x W^T (padded) and the edge list
        ctx.save_for_backward(x, weight, z if ew_grad else None, edge_index if ew_grad else None)
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    def backward(ctx, dout):
        x, weight, z, ei = ctx.saved_tensors
        L = _lib.lib()
        N, K = x.shape
        O = weight.size(0)
        ew_grad = len(ctx.needs_input_grad) > 5 and ctx.needs_input_grad[5] and z is not None
        dzp, dew, db = _aggregate_backward(ctx.g, dout, z if ew_grad else None, ei, ctx.degree_on,
                                           ctx.has_bias and ctx.needs_input_grad[2])
        dz = dzp[:, :O].contiguous()
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(N, K, dtype=torch.float32, device=x.device)
            check(L.bgcn_gemm_xw(ptr(dz), dz.stride(0), ptr(weight), weight.stride(0), ptr(dx), K,
                                 N, K, O, stream_handle()))
        if ctx.needs_input_grad[1]:
            dw = torch.empty(O, K, dtype=torch.float32, device=x.device)
            ws = workspace(L.bgcn_gemm_tn_workspace_size(O, K, N), x.device)
            check(L.bgcn_gemm_tn(ptr(dz), dz.stride(0), ptr(x), x.stride(0), ptr(dw), 0, K, O, O, K,
                                 N, ptr(ws), ws.numel(), stream_handle()))
        return (dx, dw, db, None, None, dew, None)[:len(ctx.needs_input_grad)]


class _GCNAggregateFn(torch.autograd.Function):
    """The aggregation half of :class:`_GCNConvFn`: out = A_hat z + b."""

    @staticmethod
    def forward(ctx, z, bias, g: Graph, edge_index=None, edge_weight=None, degree_on="col"):
        O = z.size(1)
        zp = _pad4(z.float())
        out = _aggregate(g, zp, bias, O)
        ctx.g = g
        ctx.degree_on = degree_on
        ew_grad = edge_weight is not None and ctx.needs_input_grad[4]
        ctx.save_for_backward(zp if ew_grad else None, edge_index if ew_grad else None)
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    def backward(ctx, dout):
        zp, ei = ctx.saved_tensors
        O = dout.size(1)
        ew_grad = len(ctx.needs_input_grad) > 4 and ctx.needs_input_grad[4] and zp is not None
        dzp, dew, db = _aggregate_backward(ctx.g, dout, zp if ew_grad else None, ei, ctx.degree_on,
                                           ctx.has_bias and ctx.needs_input_grad[1])
        dz = dzp[:, :O].contiguous() if ctx.needs_input_grad[0] else None
        return (dz, db, None, None, dew, None)[:len(ctx.needs_input_grad)]


def _conv_graph(g, num_nodes: int, edge_weight, degree_on: str, what: str):
    """``(graph, extra)`` for a convolution given an edge list or a :class:`Graph`: ``extra`` =
    ``(edge_index, edge_weight, degree_on)`` when the edge weights are learned (gcn_norm's backward,
    EBGCN.py:101-102 -> :84,178), else ``()``."""
    if edge_weight is not None and edge_weight.requires_grad and torch.is_grad_enabled():
        if isinstance(g, Graph):
            raise ValueError(f"{what}: a learned edge_weight needs edge_index (the graph is built from it)")
        ei = _check_ei(g)
        if edge_weight.dim() != 1 or edge_weight.numel() != ei.size(1):
            raise ValueError("edge_weight must be [E]")
        return build_graph(ei, num_nodes, edge_weight.detach(), degree_on), (ei, edge_weight, degree_on)
    if not isinstance(g, Graph):
        g = build_graph(g, num_nodes, edge_weight, degree_on)
    return g, ()


def gcn_conv(x: torch.Tensor, edge_index_or_graph, weight: torch.Tensor,
             bias: Optional[torch.Tensor] = None, edge_weight: Optional[torch.Tensor] = None,
             degree_on: str = "col", status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``status`` (int32 [1], optional): the graph's status word (bit 0: an edge index out of range) is
    OR-ed into it on the device, for a caller that reads one word at the end of a step."""
    _dev_check(x, weight, bias, edge_weight)
    g, extra = _conv_graph(edge_index_or_graph, x.size(0), edge_weight, degree_on, "gcn_conv")
    if status is not None:
        status.bitwise_or_(g.status)
    return _GCNConvFn.apply(x, weight, bias, g, *extra)


def gcn_aggregate(z: torch.Tensor, edge_index_or_graph, bias: Optional[torch.Tensor] = None,
                  edge_weight: Optional[torch.Tensor] = None, degree_on: str = "col",
                  status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The aggregation half of :func:`gcn_conv`: ``A_hat z + bias`` with ``A_hat = gcn_norm(edge_index,
    edge_weight)``, for a ``z = x W^T`` [N, O] computed elsewhere.  Gradients reach ``z``, ``bias`` and a
    learned ``edge_weight``; given ``z`` from the same product, the result has ``gcn_conv``'s bits.
    ``status``: as in :func:`gcn_conv`."""
    _dev_check(z, bias, edge_weight)
    if z.dim() != 2:
        raise ValueError("z must be [N, O]")
    if bias is not None and bias.numel() != z.size(1):
        raise ValueError("bias must have O elements")
    g, extra = _conv_graph(edge_index_or_graph, z.size(0), edge_weight, degree_on, "gcn_aggregate")
    if status is not None:
        status.bitwise_or_(g.status)
    return _GCNAggregateFn.apply(z, bias, g, *extra)


# ----------------------------------------------------------------------------- K8
class _ScatterMeanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, index, B):
        src = src.contiguous().float()
        n, C = src.shape
        out = torch.empty(B, C, dtype=torch.float32, device=src.device)
        cnt = torch.empty(B, dtype=torch.float32, device=src.device)
        status = torch.zeros(1, dtype=torch.int32, device=src.device)
        L = _lib.lib()
        ws = workspace(L.bgcn_scatter_mean_workspace_size(B), src.device)
        check(L.bgcn_scatter_mean_fwd(ptr(src), src.stride(0), ptr(index), n, C, B, ptr(out), C,
                                      ptr(cnt), ptr(status), ptr(ws), ws.numel(), stream_handle()))
        ctx.save_for_backward(index, cnt)
        ctx.shape = (n, C, B)
        return out

    @staticmethod
    def backward(ctx, dout):
        index, cnt = ctx.saved_tensors
        n, C, B = ctx.shape
        dout = dout.contiguous().float()
        dsrc = torch.empty(n, C, dtype=torch.float32, device=dout.device)
        check(_lib.lib().bgcn_scatter_mean_bwd(ptr(dout), dout.stride(0), ptr(index), ptr(cnt), n, C, B,
                                               ptr(dsrc), C, stream_handle()))
        return dsrc, None, None


def scatter_mean(src: torch.Tensor, index: torch.Tensor, dim: int = 0, out=None,
                 dim_size: Optional[int] = None) -> torch.Tensor:
    """``torch_scatter.scatter_mean(src, index, dim=0)`` on the GPU.  Like torch_scatter,
    ``dim_size=None`` means ``index.max() + 1`` (a host sync, as in the reference)."""
    if dim not in (0, -src.dim()):
        raise NotImplementedError("scatter_mean: only dim=0 is on the BiGCN path")
    _dev_check(src, index)
    index = index.to(torch.int64).contiguous()
    if dim_size is None:
        dim_size = int(index.max().item()) + 1 if index.numel() else 0
    if dim_size == 0:
        return src.new_zeros((0,) + tuple(src.shape[1:]))
    shp = src.shape
    res = _ScatterMeanFn.apply(src.reshape(shp[0], -1), index, int(dim_size))
    res = res.view((int(dim_size),) + tuple(shp[1:]))
    if out is not None:
        out.copy_(res)
        return out
    return res


# ----------------------------------------------------------------------------- EBGCN (eval)
EDGE_INFER_TILE = _lib.BGCN_EDGE_INFER_TILE   # edges per workgroup of the edge-inference kernel
_NO_TRAINING = ("bigcn_amd's EBGCN is the inference-only path (eval mode): training - batch-statistics "
                "BatchNorm, the Bayesian edge branch and its KL loss, the backward - is not implemented "
                "by forward.  EBGCN.train_forward(data) is the training forward.")


def bn_fold(bn: torch.nn.Module):
    """An eval-mode ``BatchNorm1d`` as ``y = g x + t`` (``bgcn_bn_fold``): ``g = weight /
    sqrt(running_var + eps)``, ``t = bias - running_mean g``; returns ``(g, t)``."""
    if bn.running_mean is None or bn.weight is None:
        raise ValueError("bn_fold needs an affine BatchNorm with running statistics")
    ps = [q.detach().to(torch.float32).contiguous() for q in (bn.weight, bn.bias, bn.running_mean, bn.running_var)]
    _dev_check(*ps)
    C = ps[0].numel()
    gt = torch.empty(2, C, dtype=torch.float32, device=ps[0].device)
    check(_lib.lib().bgcn_bn_fold(*(ptr(q) for q in ps), float(bn.eps), C, ptr(gt[0]), ptr(gt[1]), stream_handle()))
    return gt[0], gt[1]


def _f32c(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(torch.float32).contiguous()


def edge_infer(h: torch.Tensor, edge_index: torch.Tensor, direction_module, validate: bool = False,
               status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``edge_pred`` [E] of ``direction_module.edge_infer(h, edge_index)`` (``EBGCN.py:95-116``)
    in eval mode, on the edge-inference kernel (``bgcn_edge_infer``); the Bayesian branch, which
    only feeds the edge loss, is not run.

    ``h`` [N, 64] is conv1's output, ``direction_module`` a ``TDrumorGCN`` / ``BUrumorGCN`` of
    :mod:`bigcn_amd.ebgcn` (anything with the reference's ``sim_network`` and ``fc1``).  As in
    the reference, edge ``(r, c)`` reads the rows ``h[r - 1]`` and ``h[c - 1]`` (0 wraps to the
    last node).  An edge with an index outside [0, N) gets 0 and sets ``status`` (an int32 [1]
    device tensor, optional) to 1; ``validate=True`` syncs and raises IndexError instead."""
    if direction_module.training:
        raise NotImplementedError(_NO_TRAINING)
    conv, norm, _act, conv_out = direction_module.sim_network
    fc1 = direction_module.fc1.weight
    _dev_check(h, edge_index, fc1)
    ei = _check_ei(edge_index)
    if h.dim() != 2:
        raise ValueError("h must be [N, hidden]")
    h = _f32c(h) if (h.dtype != torch.float32 or h.stride(1) != 1 or h.requires_grad) else h
    N, H = h.shape
    E = int(ei.size(1))
    K = int(fc1.size(0))
    if conv.weight.shape != (H, H, 1) or conv_out.weight.shape != (1, H, 1) or fc1.shape != (K, H):
        raise ValueError("direction_module's sim_network / fc1 do not match h's hidden size")
    pred = torch.empty(E, dtype=torch.float32, device=h.device)
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=h.device)
    g, t = bn_fold(norm)
    wc, wo, bo, f1 = _f32c(conv.weight), _f32c(conv_out.weight), _f32c(conv_out.bias), _f32c(fc1)
    check(_lib.lib().bgcn_edge_infer(ptr(h), h.stride(0), N, H, ptr(ei), E, ptr(wc), ptr(g), ptr(t), ptr(wo),
                                     ptr(bo), ptr(f1), K, ptr(pred), ptr(status), stream_handle()))
    if validate and int(status.item()) & 1:
        raise IndexError("edge_index contains an index out of range [0, num_nodes)")
    return pred


# ----------------------------------------------------------------------------- EBGCN (training)
EDGE_NETWORKS = ("sim_network", "W_mean", "W_bias", "B_mean", "B_bias")   # bgcn_edge_train_fwd_args.net order


def _fill_edge_net(dst, tensors, eps) -> None:
    dst.conv_w, dst.norm_weight, dst.norm_bias, dst.out_w, dst.out_b = (ptr(t) for t in tensors)
    dst.eps = float(eps)


class _EdgeInferTrainFn(torch.autograd.Function):
    """``bgcn_edge_infer_train_fwd`` / ``_bwd``.  Inputs after ``meta``: h, the sim network's conv0
    weight, norm0 weight and bias, conv_out weight and bias, fc1's weight (the seven that receive
    a gradient), then the Bayesian networks' tensors, fc2's weight, the noise and the edge list."""

    @staticmethod
    def forward(ctx, meta, h, wc, gamma, beta, wo, bo, fc1, *rest):
        bayes, (fc2, noise, ei) = rest[:20], rest[20:]
        eps, status = meta["eps"], meta["status"]
        dev = h.device
        hc = _f32c(h)
        N, E, K = int(hc.size(0)), int(ei.size(1)), int(fc1.size(0))
        held = [_f32c(t) for t in (wc, gamma, beta, wo, bo, fc1, fc2) + tuple(bayes)]
        sim, f1, f2, bay = held[:5], held[5], held[6], held[7:]
        f32 = dict(dtype=torch.float32, device=dev)
        pred, loss = torch.empty(E, **f32), torch.empty(1, **f32)
        s, p, py = torch.empty(E, 64, **f32), torch.empty(E, K, **f32), torch.empty(E, K, **f32)
        sim_stats = torch.empty(2, 64, **f32)
        nvalid = torch.empty(1, dtype=torch.int32, device=dev)
        bmean, bvar = torch.empty(5, 64, **f32), torch.empty(5, 64, **f32)
        a = _lib.EdgeTrainFwdArgs()
        a.h, a.ldh, a.num_nodes, a.hid = hc.data_ptr(), hc.stride(0), N, int(hc.size(1))
        a.edge_index, a.num_edges = ei.data_ptr(), E
        _fill_edge_net(a.net[0], sim, eps[0])
        for n in range(4):
            _fill_edge_net(a.net[n + 1], bay[5 * n:5 * n + 5], eps[n + 1])
        a.fc1_w, a.fc2_w, a.edge_num, a.noise = f1.data_ptr(), f2.data_ptr(), K, noise.data_ptr()
        a.edge_pred, a.edge_loss, a.s, a.p, a.p_y = (t.data_ptr() for t in (pred, loss, s, p, py))
        a.sim_mean, a.sim_rstd, a.num_valid = sim_stats[0].data_ptr(), sim_stats[1].data_ptr(), nvalid.data_ptr()
        a.batch_mean, a.batch_var, a.status = bmean.data_ptr(), bvar.data_ptr(), status.data_ptr()
        L = _lib.lib()
        ws = workspace(L.bgcn_edge_infer_train_workspace_size(N, E), dev)
        check(L.bgcn_edge_infer_train_fwd(ctypes.addressof(a), ws.data_ptr(), ws.numel(), stream_handle()))
        ctx.save_for_backward(hc, ei, sim[0], sim[1], sim[2], sim[3], f1, s, p, py, sim_stats, nvalid)
        ctx.eps = eps[0]
        ctx.in_dtypes = tuple(t.dtype for t in (h, wc, gamma, beta, wo, bo, fc1))
        meta["batch_mean"], meta["batch_var"], meta["num_valid"] = bmean, bvar, nvalid
        return loss.view(()), pred

    @staticmethod
    def backward(ctx, d_loss, d_pred):
        hc, ei, wc, gamma, beta, wo, f1, s, p, py, sim_stats, nvalid = ctx.saved_tensors
        dev = hc.device
        N, E, K = int(hc.size(0)), int(ei.size(1)), int(f1.size(0))
        d_loss, d_pred = _f32c(d_loss).view(1), _f32c(d_pred)
        f32 = dict(dtype=torch.float32, device=dev)
        dh, dwc = torch.empty(N, 64, **f32), torch.empty(64, 64, **f32)
        dgamma, dbeta, dwo, dbo = (torch.empty(n, **f32) for n in (64, 64, 64, 1))
        df1 = torch.empty(K, 64, **f32)
        a = _lib.EdgeTrainBwdArgs()
        a.h, a.ldh, a.num_nodes, a.hid = hc.data_ptr(), hc.stride(0), N, 64
        a.edge_index, a.num_edges = ei.data_ptr(), E
        _fill_edge_net(a.sim, (wc, gamma, beta, wo, None), ctx.eps)
        a.fc1_w, a.edge_num = f1.data_ptr(), K
        a.s, a.p, a.p_y = s.data_ptr(), p.data_ptr(), py.data_ptr()
        a.sim_mean, a.sim_rstd, a.num_valid = sim_stats[0].data_ptr(), sim_stats[1].data_ptr(), nvalid.data_ptr()
        a.d_pred, a.d_loss = d_pred.data_ptr(), d_loss.data_ptr()
        a.d_h, a.ldd = dh.data_ptr(), 64
        a.d_conv_w, a.d_norm_weight, a.d_norm_bias = dwc.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr()
        a.d_out_w, a.d_out_b, a.d_fc1_w = dwo.data_ptr(), dbo.data_ptr(), df1.data_ptr()
        L = _lib.lib()
        ws = workspace(L.bgcn_edge_infer_train_workspace_size(N, E), dev)
        check(L.bgcn_edge_infer_train_bwd(ctypes.addressof(a), ws.data_ptr(), ws.numel(), stream_handle()))
        # (the passes share their recomputation: all seven are always computed)
        grads = (dh, dwc.view(64, 64, 1), dgamma, dbeta, dwo.view(1, 64, 1), dbo, df1)
        grads = tuple(g.to(dt) if need else None
                      for g, dt, need in zip(grads, ctx.in_dtypes, ctx.needs_input_grad[1:8]))
        return (None,) + grads + (None,) * 23


def edge_infer_train(h: torch.Tensor, edge_index: torch.Tensor, direction_module, noise: Optional[torch.Tensor] = None,
                     generator: Optional[torch.Generator] = None, status: Optional[torch.Tensor] = None):
    """``(edge_loss, edge_pred)`` of ``direction_module.edge_infer(h, edge_index)`` in TRAINING mode
    (``EBGCN.py:95-116``, ``:189-212``) as one autograd function on ``bgcn_edge_infer_train_fwd`` /
    ``_bwd``: the five per-edge networks with batch-statistics BatchNorm, fc1 -> sigmoid -> mean
    (``edge_pred`` [E]), the Bayesian draw and the KL edge loss (0-dim).

    Gradients reach ``h``, the sim network's five parameters and ``fc1.weight`` only: the
    reference's ``th.normal`` has no gradient, so the four Bayesian networks and ``fc2`` get none
    (their ``.grad`` stays ``None``).  All five ``norm0`` modules have their running statistics and
    ``num_batches_tracked`` updated as ``torch.nn.BatchNorm1d`` does in training.

    ``noise``: the standard-normal draw, fp32 ``[E, 64]`` (``y = sigmoid(mean + std * noise)``);
    ``None`` draws ``torch.randn`` on the device from ``generator``.  An edge with an index outside
    [0, N) gets ``edge_pred`` 0, adds to no statistic, loss or gradient and sets ``status`` (int32
    [1], optional) to 1.  ``E == 0`` raises ``ValueError``."""
    nets = [getattr(direction_module, n) for n in EDGE_NETWORKS]
    fc1, fc2 = direction_module.fc1.weight, direction_module.fc2.weight
    norms = [net[1] for net in nets]
    for bn in norms:
        if bn.momentum is None:
            raise ValueError("edge_infer_train: BatchNorm momentum=None (cumulative average) is not supported")
        if bn.running_mean is None or bn.weight is None:
            raise ValueError("edge_infer_train needs affine BatchNorms with running statistics")
    _dev_check(h, edge_index, fc1, fc2, noise)
    ei = _check_ei(edge_index)
    E = int(ei.size(1))
    if E == 0:
        raise ValueError("edge_infer_train needs at least one edge (BatchNorm has no batch to take statistics of)")
    if h.dim() != 2 or h.size(1) != 64:
        raise ValueError("h must be [N, 64]")
    K = int(fc1.size(0))
    if fc1.shape != (K, 64) or fc2.shape != (K, 64) or not 1 <= K <= 8:
        raise ValueError("fc1 / fc2 must be [edge_num, 64] with edge_num in [1, 8]")
    for net in nets:
        if net[0].weight.shape != (64, 64, 1) or net[3].weight.shape != (1, 64, 1):
            raise ValueError("the per-edge networks do not match the hidden size 64")
    if noise is None:
        noise = torch.randn(E, 64, dtype=torch.float32, device=h.device, generator=generator)
    elif noise.shape != (E, 64):
        raise ValueError("noise must be [E, 64]")
    noise = _f32c(noise)
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=h.device)
    meta = {"eps": [float(bn.eps) for bn in norms], "status": status}

    def tensors(net):
        return (net[0].weight, net[1].weight, net[1].bias, net[3].weight, net[3].bias)

    bayes = [t.detach() for net in nets[1:] for t in tensors(net)]
    loss, pred = _EdgeInferTrainFn.apply(meta, h, *tensors(nets[0]), fc1, *bayes, fc2.detach(), noise, ei)
    with torch.no_grad():
        # a batch without one valid edge has no statistics: it blends nothing (decided on the
        # device, no sync)
        some = meta["num_valid"] > 0
        for n, bn in enumerate(norms):
            m = some.to(bn.running_mean.dtype) * float(bn.momentum)
            bn.running_mean.add_(m * (meta["batch_mean"][n].to(bn.running_mean.dtype) - bn.running_mean))
            bn.running_var.add_(m * (meta["batch_var"][n].to(bn.running_var.dtype) - bn.running_var))
            if bn.num_batches_tracked is not None:
                bn.num_batches_tracked += some.to(bn.num_batches_tracked.dtype).view(())
    return loss, pred


def ebgcn_conv2_lin(h1: torch.Tensor, x: torch.Tensor, batch: torch.Tensor, rootindex: torch.Tensor,
                    weight: torch.Tensor, bn1: Optional[torch.nn.Module], validate: bool = False,
                    status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """conv2's lin of the eval-mode EBGCN direction (``EBGCN.py:72-84``): ``relu(bn1(cat(h1,
    x[root of the node's tree]))) W2^T`` [N, 64], the root block's F-wide product done once per
    tree (``bgcn_ebgcn_conv2_lin``).  ``bn1=None`` skips the BatchNorm (the reference's one-node
    batch).  A rootindex outside [0, N) or a batch id outside [0, B) contributes zeros and sets
    ``status`` (int32 [1], optional) to 1; ``validate=True`` syncs and raises IndexError."""
    _dev_check(h1, x, batch, rootindex, weight)
    h1, x, w2 = _f32c(h1), _f32c(x), _f32c(weight)
    batch, rootindex = batch.to(torch.int64).contiguous(), rootindex.to(torch.int64).contiguous()
    N, H = h1.shape
    F, B = int(x.size(1)), int(rootindex.numel())
    if x.size(0) != N or batch.numel() != N or w2.shape != (H, H + F):
        raise ValueError("ebgcn_conv2_lin: shapes do not match (h1 [N, 64], x [N, F], batch [N], W2 [64, 64 + F])")
    if N == 0:
        return h1.new_empty(0, H)
    g, t = bn_fold(bn1) if bn1 is not None else (None, None)
    if g is not None and g.numel() != H + F:
        raise ValueError("bn1 must cover the [hidden + input] concat")
    z2 = torch.empty(N, H, dtype=torch.float32, device=h1.device)
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=h1.device)
    L = _lib.lib()
    ws = workspace(L.bgcn_ebgcn_conv2_lin_workspace_size(N, B, F), h1.device)
    check(L.bgcn_ebgcn_conv2_lin(ptr(h1), h1.stride(0), ptr(x), x.stride(0), ptr(batch), ptr(rootindex), N, B, F, H,
                                 ptr(w2), ptr(g), ptr(t), ptr(z2), H, ptr(status), ptr(ws), ws.numel(),
                                 stream_handle()))
    if validate and int(status.item()) & 1:
        raise IndexError("rootindex / batch contains an index out of range")
    return z2


def _rows16(t: torch.Tensor) -> torch.Tensor:
    """``t`` [n, c] as fp32 rows the float4 kernels read in place (unit column stride, a row stride
    that is a multiple of 4, a 16-byte aligned base), else a contiguous fp32 copy."""
    t = t.detach()
    if t.dtype == torch.float32 and t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0:
        return t
    return t.to(torch.float32).contiguous()


class _Conv2LinTrainFn(torch.autograd.Function):
    """``bgcn_ebgcn_conv2_lin_train_fwd`` / ``_bwd``.  Gradients reach h1, W2, bn1's weight and bias.
    ``meta``: eps and status in; batch_mean, batch_var (biased), num_valid, bn_g and bn_t out."""

    @staticmethod
    def forward(ctx, meta, h1, weight, gamma, beta, x, batch, rootindex):
        dev = h1.device
        hc, w2, ga, be = _rows16(h1), _f32c(weight), _f32c(gamma), _f32c(beta)
        N, B, F = int(hc.size(0)), int(rootindex.numel()), int(x.size(1))
        f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        z2 = torch.empty(N, 64, **f32)
        stats = torch.empty(4, 64 + F, **f32)    # batch mean, biased batch variance, the fold's g and t
        a_x = torch.empty(B, F, **f32)
        tree_count, nvalid = torch.empty(B, **i32), torch.empty(1, **i32)
        a = _lib.Conv2LinTrainFwdArgs()
        a.h1, a.ldh, a.x, a.ldx = hc.data_ptr(), hc.stride(0), x.data_ptr(), x.stride(0)
        a.batch, a.rootindex = batch.data_ptr(), rootindex.data_ptr()
        a.num_nodes, a.num_graphs, a.in_feats, a.hid = N, B, F, int(hc.size(1))
        a.w2, a.gamma, a.beta, a.eps = w2.data_ptr(), ga.data_ptr(), be.data_ptr(), meta["eps"]
        a.z2, a.ldz = z2.data_ptr(), 64
        a.batch_mean, a.batch_var, a.bn_g, a.bn_t = (stats[k].data_ptr() for k in range(4))
        a.a_x, a.tree_count, a.num_valid = a_x.data_ptr(), tree_count.data_ptr(), nvalid.data_ptr()
        a.status = meta["status"].data_ptr()
        L = _lib.lib()
        ws = workspace(L.bgcn_ebgcn_conv2_lin_train_workspace_size(N, B, F), dev)
        check(L.bgcn_ebgcn_conv2_lin_train_fwd(ctypes.addressof(a), ws.data_ptr(), ws.numel(), stream_handle()))
        ctx.save_for_backward(hc, x, batch, rootindex, w2, stats, a_x, tree_count, nvalid)
        ctx.eps = meta["eps"]
        ctx.in_dtypes = tuple(t.dtype for t in (h1, weight, gamma, beta))
        meta["batch_mean"], meta["batch_var"], meta["bn_g"], meta["bn_t"] = stats.unbind(0)
        meta["num_valid"] = nvalid
        return z2

    @staticmethod
    def backward(ctx, dz2):
        hc, x, batch, rootindex, w2, stats, a_x, tree_count, nvalid = ctx.saved_tensors
        dev = hc.device
        N, B, F = int(hc.size(0)), int(rootindex.numel()), int(x.size(1))
        dz2 = _rows16(dz2)
        f32 = dict(dtype=torch.float32, device=dev)
        dh1, dw2 = torch.empty(N, 64, **f32), torch.empty(64, 64 + F, **f32)
        dgb = torch.empty(2, 64 + F, **f32)
        a = _lib.Conv2LinTrainBwdArgs()
        a.dz2, a.lddz, a.h1, a.ldh, a.x, a.ldx = dz2.data_ptr(), dz2.stride(0), hc.data_ptr(), hc.stride(0), \
            x.data_ptr(), x.stride(0)
        a.batch, a.rootindex = batch.data_ptr(), rootindex.data_ptr()
        a.num_nodes, a.num_graphs, a.in_feats, a.hid = N, B, F, 64
        a.w2, a.eps = w2.data_ptr(), ctx.eps
        a.batch_mean, a.batch_var, a.bn_g, a.bn_t = (stats[k].data_ptr() for k in range(4))
        a.a_x, a.tree_count, a.num_valid = a_x.data_ptr(), tree_count.data_ptr(), nvalid.data_ptr()
        a.dh1, a.ldd, a.dw2, a.dgamma, a.dbeta = dh1.data_ptr(), 64, dw2.data_ptr(), dgb[0].data_ptr(), dgb[1].data_ptr()
        L = _lib.lib()
        ws = workspace(L.bgcn_ebgcn_conv2_lin_train_workspace_size(N, B, F), dev)
        check(L.bgcn_ebgcn_conv2_lin_train_bwd(ctypes.addressof(a), ws.data_ptr(), ws.numel(), stream_handle()))
        # (the passes share their intermediates: all four are always computed)
        grads = tuple(g.to(dt) if need else None
                      for g, dt, need in zip((dh1, dw2, dgb[0], dgb[1]), ctx.in_dtypes, ctx.needs_input_grad[1:5]))
        return (None,) + grads + (None, None, None)


def ebgcn_conv2_lin_train(h1: torch.Tensor, x: torch.Tensor, batch: torch.Tensor, rootindex: torch.Tensor,
                          weight: torch.Tensor, bn1: torch.nn.Module,
                          status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """conv2's lin of the EBGCN direction in TRAINING mode (``EBGCN.py:72-84``): ``relu(bn1(cat(h1,
    x[root of the node's tree]))) W2^T`` [N, 64] with bn1 on batch statistics, as one autograd function
    on ``bgcn_ebgcn_conv2_lin_train_fwd`` / ``_bwd``.  The [N, 64 + F] concat is never formed: the
    root columns' statistics, product and gradients are taken over the B root rows weighted by tree
    size; the largest arrays are [B, F] and [N, 64].

    Gradients reach ``h1``, ``weight``, ``bn1.weight`` and ``bn1.bias``; ``x`` is data
    (``x.requires_grad`` raises ``ValueError``).  bn1's running statistics and ``num_batches_tracked``
    are updated as ``torch.nn.BatchNorm1d`` does in training (``momentum=None``: the cumulative
    average; ``track_running_stats=False``: nothing to update).  A node whose tree id is outside
    [0, B) or whose tree's rootindex is outside [0, N) is left out of the statistics, gets a zero row
    and a zero gradient and sets ``status`` (int32 [1], optional) to 1; a batch with fewer than two
    valid nodes gives zeros and blends nothing (decided on the device, no sync)."""
    if bn1 is None or bn1.weight is None or bn1.bias is None:
        raise ValueError("ebgcn_conv2_lin_train needs an affine BatchNorm")
    _dev_check(h1, x, batch, rootindex, weight, bn1.weight)
    if x.requires_grad:
        raise ValueError("ebgcn_conv2_lin_train: x is data and gets no gradient (x.requires_grad is set)")
    if h1.dim() != 2 or x.dim() != 2 or h1.size(1) != 64:
        raise ValueError("ebgcn_conv2_lin_train: h1 must be [N, 64] and x [N, F]")
    N, F, B = int(h1.size(0)), int(x.size(1)), int(rootindex.numel())
    if x.size(0) != N or batch.numel() != N or weight.shape != (64, 64 + F) or bn1.weight.numel() != 64 + F:
        raise ValueError("ebgcn_conv2_lin_train: shapes do not match (h1 [N, 64], x [N, F], batch [N], "
                         "W2 [64, 64 + F], bn1 over 64 + F)")
    if N == 0 or B == 0 or F == 0 or F % 4:
        raise ValueError("ebgcn_conv2_lin_train needs N > 0, B > 0 and F a positive multiple of 4")
    x = _rows16(x)
    batch, rootindex = batch.to(torch.int64).contiguous(), rootindex.to(torch.int64).contiguous()
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=h1.device)
    meta = {"eps": float(bn1.eps), "status": status}
    z2 = _Conv2LinTrainFn.apply(meta, h1, weight, bn1.weight, bn1.bias, x, batch, rootindex)
    if bn1.track_running_stats and bn1.running_mean is not None:
        with torch.no_grad():
            # fewer than two valid nodes: no statistics, nothing blended (decided on the device, no sync)
            nv = meta["num_valid"]
            some = nv >= 2
            rm, rv = bn1.running_mean, bn1.running_var
            if bn1.num_batches_tracked is not None:
                bn1.num_batches_tracked += some.to(bn1.num_batches_tracked.dtype).view(())
            if bn1.momentum is None:   # cumulative average over the batches tracked so far
                f = some.to(rm.dtype) / bn1.num_batches_tracked.clamp(min=1).to(rm.dtype)
            else:
                f = some.to(rm.dtype) * float(bn1.momentum)
            n = nv.to(rv.dtype)
            unbiased = meta["batch_var"].to(rv.dtype) * (n / (n - 1).clamp(min=1))
            rm.add_(f * (meta["batch_mean"].to(rm.dtype) - rm))
            rv.add_(f * (unbiased - rv))
    return z2


# ----------------------------------------------------------------------------- explain
SEGMENT_RANK_LDS = _lib.BGCN_SEGMENT_RANK_LDS   # longest segment the ranking sorts in LDS
# the reference's stage keys (explain_PHEME.py:91-242), in its order
STAGES_BIGCN = ("conv1_output_sum", "conv1_output_cat_x_sum", "conv2_input_sum", "conv2_output_sum",
                "scatter_mean_input_sum")
STAGES_EBGCN = STAGES_BIGCN[:2] + ("conv1_output_cat_x_bn1_sum",) + STAGES_BIGCN[2:]


def explain_sums(h1: torch.Tensor, h2: torch.Tensor, x: torch.Tensor, batch: torch.Tensor, rootindex: torch.Tensor,
                 bn1: Optional[torch.nn.Module] = None, want_x_sum: bool = True, validate: bool = False,
                 status: Optional[torch.Tensor] = None):
    """``(sums [S, N], x_sum [N] or None)``: the per-node stage sums of one direction
    (``bgcn_explain_sums``; ``explain_PHEME.py:91-242``) from conv1's output ``h1`` [N, 64], conv2's
    output before its relu ``h2`` [N, 64] and the features ``x`` [N, F].  ``bn1=None`` gives the
    BiGCN stage list (:data:`STAGES_BIGCN`, S = 5), a ``BatchNorm1d(64 + F)`` the EBGCN one
    (:data:`STAGES_EBGCN`, S = 6).  ``x_sum`` is the row sum of ``x`` (``want_x_sum=False`` skips
    that pass over X).  A rootindex outside [0, N) or a batch id outside [0, B) contributes zeros
    and sets ``status`` (int32 [1], optional) to 1; ``validate=True`` syncs and raises IndexError."""
    _dev_check(h1, h2, x, batch, rootindex)
    h1, h2, x = _f32c(h1), _f32c(h2), _f32c(x)
    batch, rootindex = batch.to(torch.int64).contiguous(), rootindex.to(torch.int64).contiguous()
    N, H = h1.shape
    F, B = int(x.size(1)), int(rootindex.numel())
    if h2.shape != (N, H) or x.size(0) != N or batch.numel() != N:
        raise ValueError("explain_sums: shapes do not match (h1, h2 [N, 64], x [N, F], batch [N])")
    g, t = bn_fold(bn1) if bn1 is not None else (None, None)
    if g is not None and g.numel() != H + F:
        raise ValueError("bn1 must cover the [hidden + input] concat")
    S = len(STAGES_BIGCN if g is None else STAGES_EBGCN)
    sums = torch.empty(S, N, dtype=torch.float32, device=h1.device)
    x_sum = torch.empty(N, dtype=torch.float32, device=h1.device) if want_x_sum else None
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=h1.device)
    L = _lib.lib()
    ws = workspace(L.bgcn_explain_sums_workspace_size(B), h1.device)
    check(L.bgcn_explain_sums(ptr(h1), h1.stride(0), ptr(h2), h2.stride(0), ptr(x), x.stride(0), ptr(batch),
                              ptr(rootindex), N, B, F, H, ptr(g), ptr(t), ptr(sums), N, ptr(x_sum), ptr(status),
                              ptr(ws), ws.numel(), stream_handle()))
    if validate and int(status.item()) & 1:
        raise IndexError("rootindex / batch contains an index out of range")
    return sums, x_sum


def _segment_rank(values: torch.Tensor, batch: torch.Tensor, num_graphs: int, status: torch.Tensor):
    _dev_check(values, batch)
    if values.dim() == 1:
        values = values.unsqueeze(0)
    if values.dim() != 2 or values.size(1) != batch.numel():
        raise ValueError("segment_rank: values must be [S, N] (or [N]) with batch [N]")
    if values.dtype != torch.float32 or values.stride(1) != 1 or values.requires_grad:
        values = _f32c(values)
    batch = batch.to(torch.int64).contiguous()
    S, N = values.shape
    ld = values.stride(0) if S > 1 else max(N, 1)
    order = torch.empty(S, N, dtype=torch.int32, device=values.device)
    srt = torch.empty(S, N, dtype=torch.float32, device=values.device)
    L = _lib.lib()
    ws = workspace(L.bgcn_segment_rank_workspace_size(int(num_graphs)), values.device)
    check(L.bgcn_segment_rank(ptr(values), ld, S, ptr(batch), N, int(num_graphs), ptr(order), ptr(srt), ptr(status),
                              ptr(ws), ws.numel(), stream_handle()))
    return order, srt


def segment_rank(values: torch.Tensor, batch: torch.Tensor, num_graphs: int):
    """``(order int32 [S, N], sorted fp32 [S, N])``: ``torch.topk(values[s, tree], k = n)`` for
    every row ``s`` of ``values`` [S, N] and every tree of the PyG batch vector ``batch`` [N]
    (``bgcn_segment_rank``).  Inside tree t's node range ``order`` holds the tree's local node
    indices (node id minus the tree's first node) by descending value and ``sorted`` the values in
    that order.  Equal values rank by ascending node index (-0.0 equals +0.0); NaN ranks above
    +inf, NaNs among themselves by ascending index.  ``values`` may have any row stride.  One host
    sync at the end: a ``batch`` that decreases, or holds an id outside [0, num_graphs), raises
    IndexError."""
    status = torch.zeros(1, dtype=torch.int32, device=values.device)
    order, srt = _segment_rank(values, batch, num_graphs, status)
    if int(status.item()) & 1:
        raise IndexError("segment_rank: batch must be non-decreasing with ids in [0, num_graphs)")
    return order, srt


# ----------------------------------------------------------------------------- compare
TREE_CENTRALITY_LDS = _lib.BGCN_TREE_CENTRALITY_LDS   # longest tree the centrality kernel keeps in LDS
RANK_SIMILARITY_MAX = _lib.BGCN_RANK_SIMILARITY_MAX   # most rankings, and the largest k, of rank_similarity
# the reference's names (compare_similarity.py:41-43), in its order
CENTRALITY_NAMES = ("out_degree", "betweenness", "closeness")
METRIC_NAMES = ("pearsonr", "spearmanr", "kendalltau", "somersd", "jaccard")


def _raise_on_compare_status(s: int) -> None:
    """The Python errors of the status word bgcn_tree_centrality / bgcn_rank_similarity leave."""
    if s & _lib.BGCN_STATUS_TWO_PARENTS:
        raise ValueError("tree_centrality: a node has more than one incoming edge (not a tree)")
    if s & _lib.BGCN_STATUS_CROSS_TREE:
        raise ValueError("tree_centrality: an edge joins two trees of the batch")
    if s & _lib.BGCN_STATUS_CYCLE:
        raise ValueError("tree_centrality: the edges of a tree hold a cycle")
    if s & 1:
        raise IndexError("an edge endpoint is out of range, or batch is not non-decreasing with ids in "
                         "[0, num_graphs)")
    if s & 2:
        raise ValueError("rank_similarity: a list repeats a node index (or holds one outside its tree) inside its "
                         "first k entries: not a ranking")


def _num_graphs_of(batch: torch.Tensor, num_graphs: Optional[int]) -> int:
    if num_graphs is not None:
        return int(num_graphs)
    return int(batch[-1].item()) + 1 if batch.numel() else 0   # (a host sync: pass num_graphs to avoid it)


def _tree_centrality(edge_index: torch.Tensor, batch: torch.Tensor, num_graphs: int, status: torch.Tensor):
    _dev_check(edge_index, batch)
    if edge_index.dim() != 2 or edge_index.size(0) != 2:
        raise ValueError("tree_centrality: edge_index must be [2, E]")
    edge_index, batch = edge_index.to(torch.int64).contiguous(), batch.to(torch.int64).contiguous()
    N, E = batch.numel(), edge_index.size(1)
    cent = torch.zeros(3, N, dtype=torch.float32, device=batch.device)
    L = _lib.lib()
    ws = workspace(L.bgcn_tree_centrality_workspace_size(N, num_graphs), batch.device)
    check(L.bgcn_tree_centrality(ptr(edge_index), E, ptr(batch), N, num_graphs, ptr(cent), max(N, 1), ptr(status),
                                 ptr(ws), ws.numel(), stream_handle()))
    return cent


def tree_centrality(edge_index: torch.Tensor, batch: torch.Tensor, num_graphs: Optional[int] = None,
                    validate: bool = False, status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``[3, N]`` fp32, rows :data:`CENTRALITY_NAMES`: networkx's ``out_degree_centrality``,
    ``betweenness_centrality`` and ``closeness_centrality`` (default arguments) of every tree of the
    batch, from the top-down ``edge_index`` [2, E] (parent -> child, any edge order) and the PyG
    ``batch`` vector (``bgcn_tree_centrality``).  Nodes of a tree with equal child count, depth and
    subtree size get bit-equal values.  A DropEdge'd forest is accepted.  A node with two parents, an
    edge across trees, a cycle, an endpoint out of range or a bad ``batch`` sets ``status`` (int32
    [1], optional) and leaves the tree's values zero; ``validate=True`` syncs and raises ValueError /
    IndexError.  ``num_graphs=None`` reads it from ``batch`` (a host sync)."""
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=batch.device)
    cent = _tree_centrality(edge_index, batch, _num_graphs_of(batch, num_graphs), status)
    if validate:
        _raise_on_compare_status(int(status.item()))
    return cent


def _rank_similarity(orders: torch.Tensor, batch: torch.Tensor, k: int, num_graphs: int, status: torch.Tensor):
    _dev_check(orders, batch)
    if orders.dim() == 1:
        orders = orders.unsqueeze(0)
    if orders.dim() != 2 or orders.size(1) != batch.numel():
        raise ValueError("rank_similarity: orders must be [V, N] (or [N]) with batch [N]")
    orders, batch = orders.to(torch.int32).contiguous(), batch.to(torch.int64).contiguous()
    V, N = orders.shape
    sim = torch.zeros(num_graphs, len(METRIC_NAMES), V, V, dtype=torch.float64, device=orders.device)
    valid = torch.zeros(num_graphs, dtype=torch.int32, device=orders.device)
    L = _lib.lib()
    ws = workspace(L.bgcn_rank_similarity_workspace_size(num_graphs), orders.device)
    check(L.bgcn_rank_similarity(ptr(orders), max(N, 1), V, ptr(batch), N, num_graphs, int(k), ptr(sim), ptr(valid),
                                 ptr(status), ptr(ws), ws.numel(), stream_handle()))
    return sim, valid


def rank_similarity(orders: torch.Tensor, batch: torch.Tensor, k: int = 10, num_graphs: Optional[int] = None):
    """``(sim [B, 5, V, V] float64, valid [B] bool)``: the body of ``compute_metrics``
    (``compare_similarity.py:88-171``) for every tree of a batch (``bgcn_rank_similarity``).
    ``orders`` [V, N] int32 are V rankings as :func:`segment_rank` gives them; for every tree of more
    than ``k`` nodes and every pair of rankings the five statistics :data:`METRIC_NAMES` over their
    first ``k`` entries.  A tree of at most ``k`` nodes gets zeros and ``valid`` False (the
    reference skips it).  ``k`` in [2, 32], V in [1, 32].  One host sync at the end: a list that
    repeats an index inside its first ``k`` raises ValueError, a bad ``batch`` IndexError."""
    status = torch.zeros(1, dtype=torch.int32, device=orders.device)
    sim, valid = _rank_similarity(orders, batch, k, _num_graphs_of(batch, num_graphs), status)
    _raise_on_compare_status(int(status.item()))
    return sim, valid.bool()


# ----------------------------------------------------------------------------- fused encoder
_PARAM_ORDER = ("td_w1", "td_b1", "td_w2", "td_b2", "bu_w1", "bu_b1", "bu_w2", "bu_b2")


_FEAT_MODES = {"auto": _lib.BGCN_FEAT_AUTO, "sparse": _lib.BGCN_FEAT_AUTO, "dense": _lib.BGCN_FEAT_DENSE}


def feat_path(feat_mode: str, data) -> int:
    """C-ABI feature path for a batch: "auto" becomes BGCN_FEAT_SPARSE (no dense fallback
    launched) when the batch's host-side hints say its rows fit the sparse path - every row
    within the ELL cap, or the entries past it within the spill pool (``collate`` /
    ``synth_batch`` set them, bound to x's identity and version); "sparse" forces it (in
    the fused step a batch that does not fit -> check_status raises)."""
    if feat_mode == "sparse":
        return _lib.BGCN_FEAT_SPARSE
    if feat_mode == "auto" and int(data.x.size(1)) <= 5120:
        hint = data.x_nnz_hint() if hasattr(data, "x_nnz_hint") else None
        if hint is not None and int(hint) <= _lib.BGCN_SPARSE_CAP:
            return _lib.BGCN_FEAT_SPARSE
        spill = data.x_spill_hint() if hasattr(data, "x_spill_hint") else None
        if spill is not None and int(spill) <= int(data.x.size(0)) * _lib.BGCN_SPARSE_SPILL_PER_ROW:
            return _lib.BGCN_FEAT_SPARSE
    return _FEAT_MODES[feat_mode]


def _feat_code(feat_mode) -> int:
    return feat_mode if isinstance(feat_mode, int) else _FEAT_MODES[feat_mode]


def check_param_shapes(params, F: int) -> None:
    """The 8 encoder parameters (reference order) have the shapes of in_feats = F."""
    want = [(HID, F), (HID,), (HID, HID + F), (HID,)] * 2
    for p, shp in zip(params, want):
        if tuple(p.shape) != shp:
            raise ValueError(f"parameter of shape {tuple(p.shape)}, expected {shp} for in_feats={F}")


def check_encoder_shapes(x: torch.Tensor, batch: torch.Tensor, rootindex: torch.Tensor, params) -> None:
    """Host-side shape contract of the fused encoder (the kernels trust it)."""
    if x.dim() != 2:
        raise ValueError("x must be [N, F]")
    N, F = x.shape
    check_param_shapes(params, F)
    if batch.numel() != N:
        raise ValueError("batch must have one entry per node")
    if rootindex.dim() != 1:
        raise ValueError("rootindex must be 1-D")


def features(x: torch.Tensor) -> torch.Tensor:
    """Node features as the fused path reads them: bf16 stays bf16 (the bf16
    configuration: bag-of-words counts are exact), anything else becomes fp32;
    contiguous rows."""
    if x.dtype != torch.bfloat16 and x.dtype != torch.float32:
        x = x.float()
    return x.contiguous()


def x_dtype_code(x) -> int:
    """BGCN_DTYPE_* of a feature tensor (or of its dtype)."""
    dtype = x if isinstance(x, torch.dtype) else x.dtype
    return _lib.BGCN_DTYPE_BF16 if dtype == torch.bfloat16 else _lib.BGCN_DTYPE_F32


def dense_batch_desc(data):
    """``(bgcn_batch, tensors)`` of a collated batch with a dense ``x``: the descriptor's
    features, sizes, index vectors and edge lists (no DropEdge), and the tensors its
    pointers point into - ``(x, td_ei, bu_ei, batch, rootindex)`` as the kernels read them
    (:func:`features`, int64, contiguous), to be kept alive while the descriptor is used."""
    x = features(data.x)
    td_ei, bu_ei = _check_ei(data.edge_index), _check_ei(data.BU_edge_index)
    batch, root = _i64c(data.batch), _i64c(data.rootindex)
    d = BatchDesc()
    d.x, d.ldx, d.num_nodes, d.num_graphs = ptr(x), x.stride(0), x.size(0), root.numel()
    d.x_dtype = x_dtype_code(x)
    d.batch, d.rootindex = ptr(batch), ptr(root)
    d.td_edge_index, d.td_num_edges = ptr(td_ei), td_ei.size(1)
    d.bu_edge_index, d.bu_num_edges = ptr(bu_ei), bu_ei.size(1)
    return d, (x, td_ei, bu_ei, batch, root)


_GRAD_ORDER = tuple(n.replace("_w", "_dw").replace("_b", "_db") for n in _PARAM_ORDER)


def _fill_args(a: BiGCNArgs, x, batch, rootindex, graphs, B, training, seed, keep, feat_mode, xs, params):
    """``graphs``: the batch's ``(td, bu)`` :class:`Graph` pair, or its :class:`PreparedBatch`
    (bgcn_bigcn_args.prepared: graphs, tree pointers and the ELL of X come from its buffer)."""
    N, F = x.shape
    a.x, a.ldx, a.num_nodes, a.num_graphs, a.in_feats, a.hid = x.data_ptr(), x.stride(0), N, B, F, HID
    a.x_dtype = x_dtype_code(x)
    a.batch, a.rootindex = batch.data_ptr(), rootindex.data_ptr()
    if isinstance(graphs, PreparedBatch):
        a.prepared, a.prepared_bytes = graphs.buf.data_ptr(), graphs.buf.numel()
        a.td_num_edges, a.bu_num_edges = graphs.td_num_edges, graphs.bu_num_edges
    else:
        a.td, a.bu = graphs[0].view(), graphs[1].view()
    a.td_w1, a.td_b1, a.td_w2, a.td_b2, a.bu_w1, a.bu_b1, a.bu_w2, a.bu_b2 = (p.data_ptr() for p in params)
    a.training, a.seed = int(bool(training)), int(seed) & (2**64 - 1)
    a.keep_words = ptr(keep)
    a.feat_mode = feat_mode
    if xs is not None:
        a.x_flags, a.x_nnz, a.x_cols, a.x_vals = (t.data_ptr() for t in xs)


_ENC_SAVED = 11   # tensors of _encoder_forward's `saved` before the parameters


def _encoder_forward(ctx, x, batch, rootindex, td: Graph, bu: Graph, B, training, seed, keep_words,
                     feat_mode, params, stream, prep=None):
    """The encoder's native forward; returns (head [B, 256], tensors for backward) and
    keeps the rest of the forward -> backward state on ``ctx`` (``_encoder_backward``).
    ``prep`` (a ``PreparedBatch`` of this batch, ``td`` / ``bu`` then None): the graphs,
    tree pointers, items and ELL / CSC of X come from it (bgcn_bigcn_args.prepared)."""
    x = features(x)
    N, F = x.shape
    dev = x.device
    L = _lib.lib()
    xs = tree_ptr = None
    if prep is not None:
        prep.check_matches(x, batch, rootindex, B, feat_mode)
    else:
        if feat_mode != _lib.BGCN_FEAT_DENSE:
            cap = _lib.BGCN_SPARSE_CAP
            xs = (torch.empty(8, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev),
                  torch.empty(N * cap, dtype=torch.int32, device=dev),
                  torch.empty(N * cap, dtype=torch.float32, device=dev))
        tree_ptr = torch.empty(B + 1, dtype=torch.int32, device=dev)
    a = BiGCNArgs()
    _fill_args(a, x, batch, rootindex, (td, bu) if prep is None else prep, B, training, seed, keep_words,
               feat_mode, xs, params)
    h1 = torch.empty(N, 2 * HID, dtype=torch.float32, device=dev)
    h2 = torch.empty(N, 2 * HID, dtype=torch.float32, device=dev)
    head = torch.empty(B, 4 * HID, dtype=torch.float32, device=dev)
    a.tree_ptr, a.h1, a.h2, a.head_in = ptr(tree_ptr), h1.data_ptr(), h2.data_ptr(), head.data_ptr()
    a.save_for_backward = 1 if any(ctx.needs_input_grad) else 0
    if prep is not None:
        prep.wait()                                # its preparation ordered before this forward
    ws = workspace(L.bgcn_bigcn_workspace_size(N, B, F, HID), dev)
    check(L.bgcn_bigcn_forward(ctypes.byref(a), ws.data_ptr(), ws.numel(), stream))
    ctx.ws = ws if a.save_for_backward else None   # forward -> backward state (bgcn.h)
    ctx.args = a                                   # the backward reuses the filled struct
    ctx.graphs = (td, bu) if prep is None else (prep,)   # (a prepared buffer lives until the backward)
    ctx.meta = (B, N, params[0].device)
    ctx.has_keep = keep_words is not None
    empty = x.new_empty(0)
    # saved for autograd's version checks and lifetime (the struct holds their pointers); a
    # prepared batch has no tree_ptr / ELL tensors of its own: empty placeholders
    saved = (x, batch, rootindex, keep_words if keep_words is not None else empty,
             tree_ptr if tree_ptr is not None else empty, h1, h2, *(xs if xs is not None else (empty,) * 4))
    assert len(saved) == _ENC_SAVED
    return head, saved + tuple(params)


class PreparedBatch:
    """A batch's weight-independent state built ahead of its forward (``prepare_batch``:
    K1 gcn_norm + CSR of both directions with their aggregation plans, tree pointers and
    work items, the ELL / spill pool / CSC of X - bgcn_prepare_batch) in a caller-side
    buffer, plus the event that ends its preparation.  The drop-in model's forward takes it
    from ``data._bgcn_prep`` (``prepare_ahead`` attaches it) and then runs no K1 and no pass
    over X of its own (bgcn_bigcn_args.prepared)."""

    def __init__(self, buf, N, B, F, td_edges, bu_edges, degree_on, dense, key, keep, event):
        self.buf, self.num_nodes, self.num_graphs, self.in_feats = buf, N, B, F
        self.td_num_edges, self.bu_num_edges = td_edges, bu_edges
        self.degree_on, self.dense, self.key, self._keep, self.event = degree_on, dense, key, keep, event
        self._waited = False
        # (slot, generation) when the buffer is one of a pipeline's reused slots
        # (prepare_ahead): the slot's counter moves on when a later batch is prepared into
        # it, and this preparation then no longer matches
        self._slot = None

    def current(self) -> bool:
        """Whether the buffer still holds this preparation (a reused slot may have taken a
        later batch since)."""
        return self._slot is None or self._slot[0][0] == self._slot[1]

    def matches(self, data, degree_on: str, feat_mode: int) -> bool:
        """Whether this preparation is of ``data`` as it is now (same tensors, unmodified,
        its buffer not reused) for that degree convention and feature path."""
        return (self.current() and self.degree_on == degree_on
                and self.dense == (feat_mode == _lib.BGCN_FEAT_DENSE) and self.key == _prep_key(data))

    def check_matches(self, x, batch, rootindex, B, feat_mode) -> None:
        if (x.size(0), B, x.size(1)) != (self.num_nodes, self.num_graphs, self.in_feats) or \
                self.dense != (feat_mode == _lib.BGCN_FEAT_DENSE):
            raise ValueError("prepared batch does not match the forward's inputs")

    def wait(self) -> None:
        """The current stream waits for the preparation (once) and is recorded as a user of
        the buffer (it may have been allocated on the preparing stream)."""
        if not self._waited:
            s = torch.cuda.current_stream(self.buf.device)
            if self.event is not None:
                s.wait_event(self.event)
            self.buf.record_stream(s)
        self._waited = True


def _prep_key(data):
    x = data.x
    return (x.data_ptr(), x._version, tuple(x.shape), data.edge_index.data_ptr(), data.edge_index._version,
            int(data.edge_index.size(1)), data.BU_edge_index.data_ptr(), data.BU_edge_index._version,
            int(data.BU_edge_index.size(1)), data.batch.data_ptr(), data.batch._version,
            data.rootindex.data_ptr(), data.rootindex._version)


def prepare_batch(data, degree_on: str = "col", feat_mode: str = "auto", buf: Optional[torch.Tensor] = None,
                  stream: Optional[torch.cuda.Stream] = None) -> PreparedBatch:
    """bgcn_prepare_batch of a collated device batch (its edge lists as they are: the
    reference's DropEdge happened in the dataset) on ``stream`` (default: the current
    one), into ``buf`` when it is large enough.  The returned object's event marks the end
    of the preparation; the batch's tensors must be ready on ``stream`` when it runs."""
    d, keep = dense_batch_desc(data)
    _dev_check(*keep)
    x = keep[0]
    N, F = x.shape
    B = int(d.num_graphs)
    code = _feat_code(feat_path(feat_mode, data) if isinstance(feat_mode, str) else feat_mode)
    L = _lib.lib()
    n = L.bgcn_prepare_workspace_size(N, B, F, d.td_num_edges, d.bu_num_edges)
    if buf is None or buf.numel() < n:
        buf = workspace(n, x.device)
    s = stream if stream is not None else torch.cuda.current_stream(x.device)
    check(L.bgcn_prepare_batch(ctypes.byref(d), F, degree_code(degree_on), code, buf.data_ptr(), buf.numel(),
                               s.cuda_stream))
    ev = torch.cuda.Event()
    ev.record(s)
    return PreparedBatch(buf, N, B, F, int(d.td_num_edges), int(d.bu_num_edges), degree_on,
                         code == _lib.BGCN_FEAT_DENSE, _prep_key(data), keep, ev)


def _encoder_backward(ctx, saved, dhead, stream):
    """Gradients of the 8 encoder parameters (reference order) from dhead [B, 256]."""
    params = saved[_ENC_SAVED:_ENC_SAVED + 8]
    L = _lib.lib()
    a = ctx.args
    a.dhead_in = dhead.data_ptr()
    grads = [torch.empty_like(p) for p in params]
    for name, gt in zip(_GRAD_ORDER, grads):
        setattr(a, name, gt.data_ptr())
    ws = ctx.ws
    ctx.ws = None
    if ws is None:
        raise RuntimeError("bigcn_encoder: backward called twice or without a saved forward")
    for g in ctx.graphs:
        if isinstance(g, PreparedBatch) and not g.current():
            raise RuntimeError("bigcn_encoder: the forward's prepared batch buffer was reused by a later "
                               "batch (prepare_ahead) before this backward")
    check(L.bgcn_bigcn_backward(ctypes.byref(a), ws.data_ptr(), ws.numel(), stream))
    return grads


class _BiGCNEncoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, batch, rootindex, td: Graph, bu: Graph, B, training, seed, keep_words,
                feat_mode, prep, *params):
        head, saved = _encoder_forward(ctx, x, batch, rootindex, td, bu, B, training, seed, keep_words,
                                       feat_mode, params, stream_handle(), prep)
        ctx.save_for_backward(*saved)
        return head

    @staticmethod
    def backward(ctx, dhead):
        saved = ctx.saved_tensors
        dhead = dhead.contiguous().float()
        return (None,) * 11 + tuple(_encoder_backward(ctx, saved, dhead, stream_handle()))


class _BiGCNNetFn(torch.autograd.Function):
    """encoder -> fc -> log_softmax (``BiGCN.forward``, BiGCN_Twitter.py:126-130) as one
    autograd node: the encoder's native forward / backward plus the K9 head
    (``bgcn_head_forward`` / ``bgcn_head_backward``) - no library GEMM, log_softmax or
    their backward kernels, and one node for the autograd engine to run."""

    @staticmethod
    def forward(ctx, x, batch, rootindex, td: Graph, bu: Graph, B, training, seed, keep_words,
                feat_mode, prep, fc_w, fc_b, *params):
        s = stream_handle()
        head, saved = _encoder_forward(ctx, x, batch, rootindex, td, bu, B, training, seed, keep_words,
                                       feat_mode, params, s, prep)
        C = fc_w.size(0)
        logp = torch.empty(B, C, dtype=torch.float32, device=head.device)
        check(_lib.lib().bgcn_head_forward(head.data_ptr(), fc_w.data_ptr(), fc_b.data_ptr(), B, C,
                                           logp.data_ptr(), s))
        ctx.save_for_backward(*saved, head, logp, fc_w, fc_b)
        return logp

    @staticmethod
    def backward(ctx, dlogp):
        saved = ctx.saved_tensors
        head, logp, fc_w, fc_b = saved[-4:]
        dlogp = dlogp.contiguous().float()
        B, C = logp.shape
        s = stream_handle()
        dhead = torch.empty_like(head)
        dfc_w, dfc_b = torch.empty_like(fc_w), torch.empty_like(fc_b)
        check(_lib.lib().bgcn_head_backward(head.data_ptr(), logp.data_ptr(), dlogp.data_ptr(), fc_w.data_ptr(),
                                            B, C, dhead.data_ptr(), dfc_w.data_ptr(), dfc_b.data_ptr(), s))
        grads = _encoder_backward(ctx, saved, dhead, s)
        return (None,) * 11 + (dfc_w, dfc_b) + tuple(grads)


def _encoder_inputs(x, batch, rootindex, params, keep_words):
    _dev_check(x, batch, rootindex, keep_words, *params)
    for p in params:
        if p.dtype != torch.float32 or not p.is_contiguous():
            raise ValueError("parameters must be contiguous fp32")
    check_encoder_shapes(x, batch, rootindex, params)
    return _i64c(batch), _i64c(rootindex), (keep_words.contiguous() if keep_words is not None else None)


def bigcn_encoder(x: torch.Tensor, batch: torch.Tensor, rootindex: torch.Tensor, td: Graph, bu: Graph,
                  num_graphs: int, params, training: bool = False, seed: int = 0,
                  keep_words: Optional[torch.Tensor] = None, feat_mode: str = "auto",
                  prep: Optional["PreparedBatch"] = None) -> torch.Tensor:
    """cat(BU_x, TD_x) [B, 256] of ``BiGCN.forward`` (``BiGCN_Twitter.py:126-128``).

    ``params`` = (td_w1, td_b1, td_w2, td_b2, bu_w1, bu_b1, bu_w2, bu_b2) in the
    reference layout (``convN.lin.weight [out, in]``, ``convN.bias``).  ``keep_words``
    optionally injects the dropout draw as packed bits [2, N, ceil((64+F)/32)] int32.
    ``feat_mode``: "auto" (sparse feature path, dense MFMA fallback decided on the
    device), "dense" (always the dense MFMA kernels) or a C-ABI code (``feat_path``:
    BGCN_FEAT_SPARSE when the batch's hints say its rows fit)."""
    batch, rootindex, keep_words = _encoder_inputs(x, batch, rootindex, params, keep_words)
    return _BiGCNEncoderFn.apply(x, batch, rootindex, td, bu, int(num_graphs), bool(training), int(seed),
                                 keep_words, _feat_code(feat_mode), prep, *params)


def head_fits(fc: torch.nn.Module) -> bool:
    """Whether ``fc`` is a head the K9 kernels take in place of ``fc(...)``: exactly a
    ``torch.nn.Linear(256, C <= 16)`` (not a subclass with its own forward) with a bias,
    no forward hooks (their side effects would be skipped), contiguous fp32 weights on
    16-byte boundaries (``bgcn_head_forward``'s alignment contract).  Anything else runs
    through ``fc`` itself and torch's log_softmax."""
    w, b = getattr(fc, "weight", None), getattr(fc, "bias", None)
    return (type(fc) is torch.nn.Linear and w is not None and b is not None and w.dim() == 2
            and not fc._forward_hooks and not fc._forward_pre_hooks
            and not torch.nn.modules.module._global_forward_hooks
            and not torch.nn.modules.module._global_forward_pre_hooks
            and w.size(1) == 4 * HID and 0 < w.size(0) <= 16 and w.dtype == torch.float32
            and b.dtype == torch.float32 and w.is_contiguous() and b.is_contiguous()
            and w.data_ptr() % 16 == 0 and b.data_ptr() % 4 == 0)


def bigcn_net(x: torch.Tensor, batch: torch.Tensor, rootindex: torch.Tensor, td: Graph, bu: Graph,
              num_graphs: int, params, fc_w: torch.Tensor, fc_b: torch.Tensor, training: bool = False,
              seed: int = 0, keep_words: Optional[torch.Tensor] = None, feat_mode: str = "auto",
              prep: Optional["PreparedBatch"] = None) -> torch.Tensor:
    """``log_softmax(fc(bigcn_encoder(...)), dim=1)`` [B, C] (``BiGCN_Twitter.py:126-130``)
    as one autograd node: the encoder plus the K9 head kernels.  ``fc_w`` [C, 256] and
    ``fc_b`` [C] are the ``fc`` Linear's parameters (C <= 16)."""
    batch, rootindex, keep_words = _encoder_inputs(x, batch, rootindex, params, keep_words)
    _dev_check(fc_w, fc_b)
    if (fc_w.dim() != 2 or fc_w.size(1) != 4 * HID or not 0 < fc_w.size(0) <= 16 or fc_b.shape != (fc_w.size(0),)
            or fc_w.dtype != torch.float32 or fc_b.dtype != torch.float32
            or not fc_w.is_contiguous() or not fc_b.is_contiguous()):
        raise ValueError("fc must be a contiguous fp32 Linear(256, C <= 16) with a bias")
    return _BiGCNNetFn.apply(x, batch, rootindex, td, bu, int(num_graphs), bool(training), int(seed), keep_words,
                             _feat_code(feat_mode), prep, fc_w, fc_b, *params)


def keep_words(seed: int, num_nodes: int, in_feats: int, device) -> torch.Tensor:
    """Materialise the in-kernel dropout keep bits [2, N, nw] (int32 view of uint32)."""
    nw = (HID + in_feats + 31) // 32
    w = torch.empty(2, num_nodes, nw, dtype=torch.int32, device=device)
    check(_lib.lib().bgcn_keep_words(int(seed) & (2**64 - 1), num_nodes, nw, ptr(w), stream_handle()))
    return w


def unpack_keep(words: torch.Tensor, width: int) -> torch.Tensor:
    """[..., nw] packed keep words -> [..., width] bool (bit j of word w = column 32w+j)."""
    w = words.to(torch.int64) & 0xFFFFFFFF
    bits = torch.arange(32, device=w.device, dtype=torch.int64)
    m = ((w.unsqueeze(-1) >> bits) & 1).bool()
    return m.reshape(*words.shape[:-1], -1)[..., :width]


def pack_keep(mask: torch.Tensor) -> torch.Tensor:
    """[..., width] bool -> [..., ceil(width/32)] int32 words."""
    width = mask.size(-1)
    nw = (width + 31) // 32
    pad = nw * 32 - width
    m = torch.nn.functional.pad(mask.to(torch.int64), (0, pad)).reshape(*mask.shape[:-1], nw, 32)
    w = (m << torch.arange(32, dtype=torch.int64, device=mask.device)).sum(-1)
    w = torch.where(w >= 2**31, w - 2**32, w)
    return w.to(torch.int32)


def set_kernel_timing(enable, classes=None) -> None:
    """Enable (all classes, or the iterable ``classes``) / disable the kernel-timing hook."""
    mask = 0
    if enable:
        mask = 0xFF if classes is None else sum(1 << int(c) for c in classes)
    check(_lib.lib().bgcn_set_kernel_timing(mask))


def kernel_timing(kernel_class: int):
    """(total_ms, launches) of a kernel class since set_kernel_timing(True) (syncs)."""
    ms = ctypes.c_float(0.0)
    n = ctypes.c_int64(0)
    check(_lib.lib().bgcn_kernel_timing(kernel_class, ctypes.byref(ms), ctypes.byref(n)))
    return float(ms.value), int(n.value)


def kernel_span(kernel_class: int):
    """(total_ms, launches) of a stamped kernel class's device-side spans since
    set_kernel_timing(True) (the kernel's own first-block-start to last-block-end; syncs)."""
    ms = ctypes.c_float(0.0)
    n = ctypes.c_int64(0)
    check(_lib.lib().bgcn_kernel_span(kernel_class, ctypes.byref(ms), ctypes.byref(n)))
    return float(ms.value), int(n.value)
