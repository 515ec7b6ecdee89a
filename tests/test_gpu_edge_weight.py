"""Exact and edge-shape tests of the weighted graph build and of d edge_weight (bgcn_graph.hip:
the weighted steps of bgcn_build_graph, bgcn_graph_dinv, bgcn_edge_weight_grad = k_ew_nodes +
k_ew_edges), through the C ABI and through gcn_conv / gcn_aggregate.

The inputs and the float64 reference come from tests/edge_weight_ref.py.  On its EXACT class
(degrees 4^k, integer weights and features) every product and partial sum is an fp32 number, so
the kernels must return the fp64 result cast to fp32 bit for bit (torch.equal) whatever their
summation order; tests/test_edge_weight_ref.py shows on the CPU that a wrong degree key, a
dropped term or a feature loop that stops at column 64 changes that result on these very inputs.
The GENERAL class (random weights and features) is compared with the project's elementwise rule.

Every operand of bgcn_edge_weight_grad lives inside a larger allocation whose other elements
(the columns from F to ld, a guard after the last row) hold NaN; the workspaces hold 0xFF bytes;
d_edge_weight is followed by a sentinel that must survive.

Which kernel and branch each case enters:
* test_build_exact: the weighted steps k_count -> k_scan_blocks / _top / _write -> k_fill ->
  k_fill_rank -> k_nodes -> k_normalize.  A tree's target rows hold one edge each, so in the td
  lists the target orientation keeps the grouped placement (flags[3]) in every order unless
  flags[2] is set, and the source orientation is grouped in `reference` order, general (atomic
  slot + rank) when `shuffled`; the bu (flipped) lists swap the two.  A loop `inside` its node's
  run sets flags[2]: both orientations general.  A loop `between` runs of other nodes or at the
  `tail` leaves both grouped (the run starts after it).  The stars' root rows (255, 1023, 2999
  entries) are the long rows of the aggregation plans and, where the root is the key, the
  degree-heavy node (256, 1024, 4096).
* test_build_two_loops_on_one_node: the atomicMax of loop_eid ("last loop wins"), forward only.
* test_build_general_shuffled: general placement in both orientations, distinct random weights.
* test_edge_weight_grad_exact: k_ew_nodes and k_ew_edges with F4 = F: F = 4, 12, 60 one trip of
  the feature loop with 15, 13 and 1 idle lanes; 64 one trip, all lanes; 68 a second trip for lane
  0 alone; 128 two full trips; 132 and 200 three and four trips, the last one partial; ld = F + 4
  rows with a gap.  The `inside` / `between` / `tail` graphs take the loop-edge branch of
  k_ew_edges (dw = lgrad[src]); N = 365 and E = 357 / 358 leave the last block partial.
* test_out_of_range_edge: the invalid-edge branch of k_ew_edges (dw = 0), flags[2] in the build.
* test_zero_degree_node: dis = 0 in k_nodes (the masked inf) and the `dis > 0` select of k_ew_nodes.
* test_duplicate_edge: general placement in both orientations; two edges, one (s, d).
* test_no_edges: k_ew_nodes alone (no edge launch); the unweighted build (a null weight pointer).
* test_autograd_*: ops._aggregate_backward, F4 = _pad4(O): O = 10 -> 12 (one trip, zero-padded
  columns), 66 -> 68 (two trips), 128 (two trips).
"""
import ctypes

import numpy as np
import pytest
import torch

import edge_weight_ref as R
from oracle import bigcn_oracle as O
from test_gpu_gemm_exact import Dev, _ws
from test_gpu_kernels import _dump_errors, close, close_elem, dense_adj

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -777.25
GUARD = 64


def _api():
    from bigcn_amd import _lib
    return _lib.lib(), _lib.check, _lib.stream_handle()


class Built:
    """bgcn_build_graph through the C ABI: outputs pre-filled with sentinels, a 0xFF workspace
    that stays with the graph (it holds dinv)."""

    def __init__(self, ei, w, N, degree_on):
        L, check, stream = _api()
        ei = np.asarray(ei, np.int64).reshape(2, -1)
        self.N, self.E = N, ei.shape[1]
        self.cap = self.E + N
        self.ei = torch.from_numpy(np.ascontiguousarray(ei)).to(DEV)
        self.w = None if w is None else torch.from_numpy(np.asarray(w, np.float32)).to(DEV)
        self.code = {"col": 0, "row": 1}[degree_on]
        i32 = lambda n: torch.full((n,), -7, dtype=torch.int32, device=DEV)      # noqa: E731
        self.a = {"t_ptr": i32(N + 1), "t_row": i32(self.cap), "t_col": i32(self.cap),
                  "t_w": torch.full((self.cap,), SENT, device=DEV),
                  "s_ptr": i32(N + 1), "s_row": i32(self.cap), "s_col": i32(self.cap),
                  "s_w": torch.full((self.cap,), SENT, device=DEV)}
        self.status = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.ws = _ws(L.bgcn_graph_workspace_size(self.E, N))
        check(L.bgcn_build_graph(self.ei.data_ptr() if self.E else 0,
                                 self.w.data_ptr() if self.w is not None and self.E else 0, self.E, N, self.code,
                                 *(self.a[k].data_ptr() for k in ("t_ptr", "t_row", "t_col", "t_w",
                                                                  "s_ptr", "s_row", "s_col", "s_w")),
                                 self.status.data_ptr(), self.ws.data_ptr(), self.ws.numel(), stream))
        out = ctypes.c_void_p()
        check(L.bgcn_graph_dinv(self.ws.data_ptr(), self.ws.numel(), self.E, N, ctypes.byref(out)))
        off = int(out.value) - self.ws.data_ptr()
        assert 0 <= off and off + 4 * N <= self.ws.numel() and off % 4 == 0
        self.dinv = self.ws[off:off + 4 * N].view(torch.float32)

    def check(self, c, what=""):
        """Bit for bit what csr_ref describes: pointers, entries in edge order with the loop last,
        norms, the row -1 tail, and dinv."""
        N = self.N
        for o in ("t", "s"):
            n = int(c[o + "_ptr"][N])
            assert torch.equal(self.a[o + "_ptr"].cpu(), torch.from_numpy(c[o + "_ptr"]).int()), (what, o, "ptr")
            for k in ("_row", "_col"):
                assert torch.equal(self.a[o + k][:n].cpu(), torch.from_numpy(c[o + k]).int()), (what, o + k)
            assert torch.equal(self.a[o + "_w"][:n].cpu(), torch.from_numpy(c[o + "_w"]).float()), (what, o + "_w")
            assert bool((self.a[o + "_row"][n:] == -1).all()) and not bool(self.a[o + "_w"][n:].any()), (what, "tail")
        assert torch.equal(self.dinv.cpu(), torch.from_numpy(c["dis"]).float()), (what, "dinv")

    def spmm(self, x, out, transposed=False):
        """out = A x (A^T x) with bgcn_spmm; x and out are Dev matrices of one width."""
        L, check, stream = _api()
        o = "s" if transposed else "t"
        ws = _ws(L.bgcn_spmm_workspace_size(self.cap, x.width))
        check(L.bgcn_spmm(*(self.a[o + k].data_ptr() for k in ("_ptr", "_row", "_col", "_w")), self.N, self.cap,
                          x.ptr, x.ld, out.ptr, out.ld, x.width, 0, 0, ws.data_ptr(), ws.numel(), stream))


def check_nan_framed(d, want, what):
    """The Dev matrix equals `want` bit for bit and everything around it is still NaN."""
    got = d.buf.cpu()
    assert torch.equal(d.view(got), want), f"{what}: {int((d.view(got) != want).sum())} elements differ"
    assert int(torch.isnan(got).sum()) == got.numel() - d.rows * d.width, f"{what}: the frame changed"


def run_grad(ei, w, N, degree_on, h, dout, pad=0, parts=None, what=""):
    """bgcn_edge_weight_grad as ops._aggregate_backward feeds it (agg and dz from bgcn_spmm on the
    built graph), every operand NaN-framed with row stride F + pad.  Returns (dw [E] on the CPU,
    the build); with `parts` (the exact reference) agg and dz are checked bit for bit too."""
    L, check, stream = _api()
    F = h.shape[1]
    g = Built(ei, w, N, degree_on)
    E = g.E
    hd = Dev(N, F, F + pad, guard=GUARD, data=torch.from_numpy(h).float())
    dd = Dev(N, F, F + pad, guard=GUARD, data=torch.from_numpy(dout).float())
    agg, dz = Dev(N, F, F + pad, guard=GUARD), Dev(N, F, F + pad, guard=GUARD)
    g.spmm(hd, agg)
    g.spmm(dd, dz, transposed=True)
    if parts is not None:
        check_nan_framed(agg, torch.from_numpy(parts["agg"]).float(), what + " A h")
        check_nan_framed(dz, torch.from_numpy(parts["dz"]).float(), what + " A^T dout")
    dw = torch.full((E + 8,), SENT, device=DEV)
    ws = _ws(L.bgcn_edge_weight_grad_workspace_size(N))
    check(L.bgcn_edge_weight_grad(g.ei.data_ptr() if E else 0, E, N, g.code, g.dinv.data_ptr(), hd.ptr, agg.ptr,
                                  dd.ptr, dz.ptr, F + pad, F, dw.data_ptr() if E else 0, ws.data_ptr(), ws.numel(),
                                  stream))
    dw = dw.cpu()
    assert bool((dw[E:] == SENT).all()), what + ": the sentinel after d_edge_weight"
    for d in (hd, dd, agg, dz):        # inputs: unchanged frames
        assert int(torch.isnan(d.buf).sum()) == d.buf.numel() - N * F, what
    return dw[:E], g


def f32(a):
    return torch.from_numpy(np.asarray(a)).float()


def worst_ratio(got, want, floor, rtol=1e-4):
    """The largest |got - want| over close_elem's bound rtol (|want| + floor max|want|)."""
    a, b = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(want).detach().double().cpu()
    return float(((a - b).abs() / (rtol * (b.abs() + floor * float(b.abs().max())))).max())


# ------------------------------------------------------------------------- the weighted build
@pytest.mark.parametrize("bu", [False, True], ids=["td", "bu"])
@pytest.mark.parametrize("order", R.BUILD_ORDERS)
@pytest.mark.parametrize("degree_on", ["col", "row"])
def test_build_exact(degree_on, order, bu):
    ran = 0
    for sizes, star in R.BUILD_GRAPHS:
        case = R.exact_build_case(sizes, star, degree_on, order, bu)
        if case is None:                      # a single star has no run of another node
            continue
        ei, w, N = case
        c = R.csr_ref(ei, w, N, degree_on)
        for k in ("t_w", "s_w", "dis"):       # the class: every norm is an fp32 number
            assert np.array_equal(c[k].astype(np.float32).astype(np.float64), c[k])
        g = Built(ei, w, N, degree_on)
        g.check(c, f"{sizes}")
        assert int(g.status) == 0
        ran += 1
    assert ran >= 1 + 3 * (order != "between")


def test_build_two_loops_on_one_node():
    """Node 1 carries the input loops 5 and then 13: the later one is its loop weight.  With the 3
    that arrives at it ('col') or leaves it ('row') its degree is 16, every other degree 1 or 4:
    the exact class again.  Forward only."""
    ei = np.array([[0, 1, 1, 1, 2], [1, 1, 2, 1, 3]])
    w = np.array([3.0, 5.0, 3.0, 13.0, 3.0])
    for degree_on in ("col", "row"):
        n = R.gcn_norm_ref(ei, w, 4, degree_on)
        assert n["lw"].tolist() == [1.0, 13.0, 1.0, 1.0] and n["deg"][1] == 16.0
        g = Built(ei, w, 4, degree_on)
        g.check(R.csr_ref(ei, w, 4, degree_on), degree_on)
        last = int(g.a["t_ptr"][2]) - 1                         # row 1's last entry: its loop
        assert int(g.a["t_col"][last]) == 1 and float(g.a["t_w"][last]) == 13.0 / 16.0


@pytest.mark.parametrize("degree_on", ["col", "row"])
def test_build_general_shuffled(degree_on):
    rng = np.random.default_rng(21)
    ei, w, N, _, _ = R.general_case(rng, [1, 2, 7, 40, 300], 4)
    perm = rng.permutation(ei.shape[1])
    ei, w = ei[:, perm], w[perm]
    g = Built(ei, w, N, degree_on)
    e, nw = O.gcn_norm(torch.from_numpy(ei), torch.from_numpy(w), N, degree_on, dtype=torch.float64)
    ref = torch.zeros(N, N, dtype=torch.float64)
    ref.index_put_((e[1], e[0]), nw, accumulate=True)
    close(dense_adj(*[g.a[k].cpu() for k in ("t_ptr", "t_row", "t_col", "t_w")], N), ref, 1e-6, "t-csr")
    close(dense_adj(*[g.a[k].cpu() for k in ("s_ptr", "s_row", "s_col", "s_w")], N), ref.t(), 1e-6, "s-csr")
    # distinct weights: every entry sits in its own slot, in edge order, the loop last
    c = R.csr_ref(ei, w, N, degree_on)
    n = int(c["t_ptr"][N])
    assert n == N + ei.shape[1] - 1          # the input loop is gone
    for o in ("t", "s"):
        assert torch.equal(g.a[o + "_ptr"].cpu(), torch.from_numpy(c[o + "_ptr"]).int())
        assert torch.equal(g.a[o + "_col"][:n].cpu(), torch.from_numpy(c[o + "_col"]).int())
        close(g.a[o + "_w"][:n], torch.from_numpy(c[o + "_w"]), 1e-6, o + "_w")
    close(g.dinv, torch.from_numpy(c["dis"]), 1e-6, "dinv")


# --------------------------------------------------- bgcn_edge_weight_grad, the exact class
@pytest.mark.parametrize("degree_on", ["col", "row"])
@pytest.mark.parametrize("pad", [0, 4], ids=["tight", "ld+4"])
@pytest.mark.parametrize("F", R.GPU_WIDTHS)
def test_edge_weight_grad_exact(F, pad, degree_on):
    for loop in R.GPU_LOOPS:
        ei, w, N, h, dout, p = R.gpu_exact_case(degree_on, F, loop)
        assert N % 16 and ei.shape[1] % 16
        what = f"F {F} pad {pad} {degree_on} loop {loop}"
        dw, g = run_grad(ei, w, N, degree_on, h, dout, pad, p, what)
        assert torch.equal(g.dinv.cpu(), f32(p["dis"])), what
        want = f32(p["dw"])
        assert torch.equal(dw, want), f"{what}: {int((dw != want).sum())} of {want.numel()} differ"
        assert int(g.status) == 0
    # the same edges in another order: the same gradient per edge
    ei, w, N, h, dout, p = R.gpu_exact_case(degree_on, F, None)
    perm = np.random.default_rng(F).permutation(ei.shape[1])
    dw, _ = run_grad(ei[:, perm], w[perm], N, degree_on, h, dout, pad, p, "shuffled")
    assert torch.equal(dw, f32(p["dw"][perm]))


# ------------------------------------------------------------------ the edges of the contract
@pytest.mark.parametrize("N", [1, 5])
def test_no_edges(N):
    rng = np.random.default_rng(N)
    ei, w = np.zeros((2, 0), np.int64), np.zeros(0)
    h, dout = R.exact_features(rng, N, 12)
    dw, g = run_grad(ei, w, N, "col", h, dout, 4, R.ew_parts_ref(ei, w, N, "col", h, dout), f"N {N}")
    assert dw.numel() == 0 and int(g.status) == 0
    assert torch.equal(g.dinv.cpu(), torch.ones(N))
    from bigcn_amd.ops import gcn_aggregate
    z = f32(h).to(DEV).requires_grad_(True)
    ew = torch.empty(0, device=DEV, requires_grad=True)
    out = gcn_aggregate(z, torch.from_numpy(ei).to(DEV), None, ew)
    out.backward(f32(dout).to(DEV))
    assert torch.equal(out.detach().cpu(), f32(h)) and torch.equal(z.grad.cpu(), f32(dout))
    assert ew.grad is not None and ew.grad.shape == (0,)


@pytest.mark.parametrize("degree_on", ["col", "row"])
@pytest.mark.parametrize("bad", [(-1, 2), (3, 10 ** 12), (365, 365)], ids=["src<0", "dst>>N", "loop=N"])
def test_out_of_range_edge(bad, degree_on):
    ei, w, N, h, dout, p = R.gpu_exact_case(degree_on, 68, "tail")
    at = ei.shape[1] // 3
    ei2, w2 = np.insert(ei, at, bad, axis=1), np.insert(w, at, 7.0)
    dw, g = run_grad(ei2, w2, N, degree_on, h, dout, 0, p, "with the bad edge")
    assert int(g.status) & 1
    assert float(dw[at]) == 0.0
    assert torch.equal(torch.cat([dw[:at], dw[at + 1:]]), f32(p["dw"]))          # the list without it
    assert torch.equal(dw, f32(R.ew_grad_ref(ei2, w2, N, degree_on, h, dout)))
    g.check(R.csr_ref(ei2, w2, N, degree_on), "build")


@pytest.mark.parametrize("degree_on", ["col", "row"])
def test_zero_degree_node(degree_on):
    """An edge of weight -1 against the loop's 1: the key node's degree is 0, its dis the masked
    inf.  (Autograd gives NaN here; the kernel documents 0 - tests/test_edge_weight_ref.py.)"""
    ei, w, N, h, dout, _ = R.gpu_exact_case(degree_on, 132, None)
    key = ei[1] if degree_on == "col" else ei[0]
    k = int(np.flatnonzero(np.bincount(key, minlength=N) == 1)[0])        # one edge at its key side
    w = w.copy()
    w[key == k] = -1.0
    p = R.ew_parts_ref(ei, w, N, degree_on, h, dout, exact=True)          # still the exact class
    assert p["deg"][k] == 0 and p["dis"][k] == 0 and not p["agg"][k].any()
    dw, g = run_grad(ei, w, N, degree_on, h, dout, 4, p, "zero degree")
    assert float(g.dinv[k]) == 0.0 and torch.equal(g.dinv.cpu(), f32(p["dis"]))
    assert bool(torch.isfinite(dw).all())
    assert torch.equal(dw, f32(p["dw"]))
    # the same through the operator: the dead node's forward row is 0
    from bigcn_amd.ops import gcn_aggregate
    ew = f32(w).to(DEV).requires_grad_(True)
    out = gcn_aggregate(f32(h).to(DEV), torch.from_numpy(ei).to(DEV), None, ew, degree_on=degree_on)
    out.backward(f32(dout).to(DEV))
    assert not bool(out[k].any()) and torch.equal(out.detach().cpu(), f32(p["agg"]))
    assert torch.equal(ew.grad.cpu(), f32(p["dw"]))


@pytest.mark.parametrize("degree_on", ["col", "row"])
def test_duplicate_edge(degree_on):
    """One edge of weight 3 or more split into two copies of different weights (1 and the rest),
    the second at the end of the list: the degrees stay, each copy gets its own gradient."""
    ei, w, N, h, dout, _ = R.gpu_exact_case(degree_on, 60, None)
    e = int(np.flatnonzero(w >= 3)[0])
    ei2 = np.concatenate([ei, ei[:, e:e + 1]], 1)
    w2 = np.concatenate([w, [w[e] - 1.0]])
    w2[e] = 1.0
    p = R.ew_parts_ref(ei2, w2, N, degree_on, h, dout, exact=True)
    dw, g = run_grad(ei2, w2, N, degree_on, h, dout, 0, p, "duplicate")
    g.check(R.csr_ref(ei2, w2, N, degree_on), "build")
    assert torch.equal(dw, f32(p["dw"]))
    assert float(dw[e]) != 0.0 and float(dw[-1]) != 0.0


def test_two_runs_give_equal_bits():
    ei, w, N, h, dout = R.general_case(np.random.default_rng(8), R.GPU_SIZES, 200, star=True)
    a, _ = run_grad(ei, w, N, "col", h, dout, 4)
    b, _ = run_grad(ei, w, N, "col", h, dout, 4)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    ref = R.ew_grad_ref(ei, w, N, "col", h, dout)
    close_elem(a, torch.from_numpy(ref), "d edge_weight (C ABI, general class)", floor=1e-2)


# -------------------------------------------------------------------------- through autograd
K_IN = 20


@pytest.mark.parametrize("degree_on", ["col", "row"])
@pytest.mark.parametrize("Oc", [10, 66, 128])
def test_autograd_general(Oc, degree_on):
    """gcn_conv and gcn_aggregate with a learned weight against fp64 autograd of the oracle: the
    project's elementwise rule (rtol 1e-4, floor 1e-3; d edge_weight floor 1e-2: its two terms
    nearly cancel, as test_gcnconv_learned_edge_weight explains)."""
    from bigcn_amd.ops import gcn_aggregate, gcn_conv
    rng = np.random.default_rng(100 + Oc)
    ei, w, N, x, _ = R.general_case(rng, [1, 2, 7, 40, 300, 13], K_IN, star=(Oc == 66))
    gout = rng.standard_normal((N, Oc))
    eit = torch.from_numpy(ei)
    W = torch.from_numpy(rng.standard_normal((Oc, K_IN)) / np.sqrt(K_IN)).requires_grad_(True)
    b = torch.from_numpy(rng.uniform(-0.1, 0.1, Oc)).requires_grad_(True)
    xr = torch.from_numpy(x).requires_grad_(True)
    wr = torch.from_numpy(w).requires_grad_(True)
    ref = O.gcn_conv(xr, eit, W, b, edge_weight=wr, degree_on=degree_on)
    ref.backward(torch.from_numpy(gout))

    xd = f32(x).to(DEV).requires_grad_(True)
    Wd = W.detach().float().to(DEV).requires_grad_(True)
    bd = b.detach().float().to(DEV).requires_grad_(True)
    wd = f32(w).to(DEV).requires_grad_(True)
    out = gcn_conv(xd, eit.to(DEV), Wd, bd, wd, degree_on=degree_on)
    out.backward(f32(gout).to(DEV))
    pairs = {"out": (out, ref), "dx": (xd.grad, xr.grad), "dW": (Wd.grad, W.grad), "db": (bd.grad, b.grad),
             "d edge_weight": (wd.grad, wr.grad)}

    # the aggregation half alone, on z = x W^T taken in fp64
    z = (xr.detach() @ W.detach().t())
    zr = z.clone().requires_grad_(True)
    wr2 = torch.from_numpy(w).requires_grad_(True)
    b2 = b.detach().clone().requires_grad_(True)
    ref2 = O.gcn_conv(zr, eit, torch.eye(Oc, dtype=torch.float64), b2, edge_weight=wr2, degree_on=degree_on)
    ref2.backward(torch.from_numpy(gout))
    zd = z.float().to(DEV).requires_grad_(True)
    b2d = b.detach().float().to(DEV).requires_grad_(True)
    wd2 = f32(w).to(DEV).requires_grad_(True)
    out2 = gcn_aggregate(zd, eit.to(DEV), b2d, wd2, degree_on=degree_on)
    out2.backward(f32(gout).to(DEV))
    pairs.update({"agg out": (out2, ref2), "agg dz": (zd.grad, zr.grad), "agg db": (b2d.grad, b2.grad),
                  "agg d edge_weight": (wd2.grad, wr2.grad)})

    floors = {"d edge_weight": 1e-2, "agg d edge_weight": 1e-2}
    _dump_errors(f"edge_weight_autograd_{degree_on}_{Oc}", pairs, floors=floors)
    for k, (got, want) in pairs.items():
        print(f"{k}: {worst_ratio(got, want, floors.get(k, 1e-3)):.3f} of the bound")
    for k, (got, want) in pairs.items():
        close_elem(got, want, what=k, floor=floors.get(k, 1e-3))


@pytest.mark.parametrize("degree_on", ["col", "row"])
@pytest.mark.parametrize("Oc", [10, 66, 128])
def test_autograd_exact(Oc, degree_on):
    """The same calls on the exact class with an identity weight: out, dx and d edge_weight bit for
    bit - the case the 1e-2 floor cannot hide."""
    from bigcn_amd.ops import gcn_aggregate, gcn_conv
    for loop in (None, "inside"):
        ei, w, N, h, dout, p = R.exact_case(np.random.default_rng(Oc + (degree_on == "row")), R.GPU_SIZES,
                                            degree_on, Oc, loop)
        eid = torch.from_numpy(ei).to(DEV)
        for op in ("conv", "aggregate"):
            x = f32(h).to(DEV).requires_grad_(True)
            ew = f32(w).to(DEV).requires_grad_(True)
            if op == "conv":
                out = gcn_conv(x, eid, torch.eye(Oc, device=DEV), None, ew, degree_on=degree_on)
            else:
                out = gcn_aggregate(x, eid, None, ew, degree_on=degree_on)
            out.backward(f32(dout).to(DEV))
            what = f"{op} O {Oc} {degree_on} loop {loop}"
            assert torch.equal(out.detach().cpu(), f32(p["agg"])), what
            assert torch.equal(x.grad.cpu(), f32(p["dz"])), what
            assert torch.equal(ew.grad.cpu(), f32(p["dw"])), what
