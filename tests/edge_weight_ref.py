"""A float64 restatement of the weighted gcn_norm and of its gradient w.r.t. edge_weight
(the closed formula above EwArgs in bgcn_graph.hip), and the inputs to test them with.
TEST INFRASTRUCTURE: tests/test_edge_weight_ref.py checks the restatement against autograd and
the input classes on the CPU, tests/test_gpu_edge_weight.py compares the kernels with them.

The formula, for edges e = (s, d) of weight w_e over N nodes, `key` = d ('col') or s ('row'):
  valid    s and d inside [0, N); an input self loop (s == d) is removed, its weight becomes the
           node's loop weight lw (the LAST loop of a node wins), else lw = 1
  deg[k]   = lw[k] + sum of w_e over the kept edges with key_e == k
  dis[k]   = deg[k]^-1/2, 0 where deg[k] == 0 (the masked inf)
  norm_e   = dis[s] w_e dis[d], the loop of k: dis[k]^2 lw[k]
  A        the N x N matrix A[d, s] += norm_e, A[k, k] += loop norm
  S[k]     = <dout[k], (A h)[k]> + <h[k], (A^T dout)[k]>
  dldeg[k] = -1/2 dis[k]^2 S[k], 0 where dis[k] == 0
  dw_e     = <dout[d], h[s]> dis[s] dis[d] + dldeg[key_e]        (a kept edge)
  dw_e     = <dout[k], h[k]> dis[k]^2 + dldeg[k]                 (an input self loop at k)
  dw_e     = 0                                                   (an edge out of range)
The self-loop line IS the kept-edge line at s = d = k: telling them apart is not possible, what
can go wrong for a loop is that it is given 0 (it is "removed") or the degree term alone.

EXACT class: trees whose every degree is a power of four, integer weights, integer h and dout.
  'col': every non-root node has one incoming edge, of weight 3 or 15 (degree 4 or 16); a
         zero-weight edge leaves its target at degree 1, as a root.
  'row': the weights of an inner node's children sum to 4^k - 1 (3 or 15 for up to 15
         children), a leaf has degree 1; one child may weigh 0.
  A weighted input self loop at k replaces the loop's 1 by w_l = 4^k - (the other weights at k).
Then dis is 1, 1/2, 1/4, ..., every norm a small integer times a power of two, and with
|h|, |dout| <= VMAX every term of every sum of the formula is a multiple of some power of two u
(per sum) while the absolute values of the terms add up to at most 2^24 u.  Every partial sum,
in any order and grouping, is then a multiple of u below 2^24 u: an fp32 number.  The fp64
result cast to fp32 is THE result.  `ew_parts_ref(..., exact=True)` asserts that bound for every
sum it takes (the aggregations, the three row dots, S, the loop and the edge gradients), so the
generator asserts it at the width it is called with; the widest any test uses is F_MAX.

GENERAL class: random forests in reference (parent, child) order, distinct weights in
[0.05, 2], normal h and dout.
"""
import numpy as np
import torch

VMAX = 2          # |h|, |dout| of the exact class
F_MAX = 200       # the widest feature width of the GPU tests
MUTANTS = ("no_ddeg", "swap_key", "half_S", "loop_as_edge", "loop_zero", "loop_ddeg_only", "cols_lt_64")
_Q = 40           # every term of the exact class is a multiple of 2^-40 (asserted)


def _np(a, dtype=None):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=dtype)


# ------------------------------------------------------------------------------ exactness
def _units(terms):
    """(|t| 2^Q as int64, the largest power of two dividing it; 2^38 for t == 0)."""
    t = np.abs(terms) * 2.0 ** _Q
    ti = t.astype(np.int64)
    assert t.size == 0 or (float(t.max()) < 2.0 ** 50 and bool((ti == t).all())), "no multiple of 2^-40"
    low = np.where(ti == 0, np.int64(1) << 38, np.minimum(ti & -ti, np.int64(1) << 38))
    return ti, low


def assert_sum_exact(terms, index=None, n=None, what=""):
    """Every partial sum of `terms` along the last axis - or, given `index` [T] and n, of the rows
    of terms [T, F] scattered to n rows - is an fp32 number: sum |t| <= 2^24 u, u the largest
    power of two dividing every term."""
    ti, low = _units(terms)
    if index is None:
        tot, u = ti.sum(-1), low.min(-1) if ti.shape[-1] else np.int64(1) << 38
    else:
        tot = np.zeros((n,) + ti.shape[1:], np.int64)
        u = np.full((n,) + ti.shape[1:], np.int64(1) << 38)
        np.add.at(tot, index, ti)
        np.minimum.at(u, index, low)
    assert bool((tot <= u * (1 << 24)).all()), f"{what}: a partial sum may not be an fp32 number"


# --------------------------------------------------------------------------- the formula
def gcn_norm_ref(ei, w, N, degree_on):
    """dict: src, dst, valid, loop, kept (masks over the edges), lw, deg, dis [N], norm [E] (0 off
    the kept edges), loop_norm [N]; float64."""
    assert degree_on in ("col", "row")
    ei = _np(ei, np.int64).reshape(2, -1)
    E = ei.shape[1]
    w = np.ones(E) if w is None else _np(w, np.float64)
    src, dst = ei[0], ei[1]
    valid = (src >= 0) & (src < N) & (dst >= 0) & (dst < N)
    loop = valid & (src == dst)
    kept = valid & ~loop
    lw = np.ones(N)
    for e in np.flatnonzero(loop):          # in edge order: the last loop of a node wins
        lw[src[e]] = w[e]
    key = dst if degree_on == "col" else src
    deg = np.zeros(N)
    np.add.at(deg, key[kept], w[kept])
    deg = deg + lw                          # the edges in order, then the loop
    with np.errstate(divide="ignore"):
        dis = np.where(deg == 0, 0.0, 1.0 / np.sqrt(deg))
    s, d = np.where(kept, src, 0), np.where(kept, dst, 0)
    norm = np.where(kept, dis[s] * w * dis[d], 0.0)
    return dict(src=src, dst=dst, valid=valid, loop=loop, kept=kept, key=key, w=w, lw=lw, deg=deg,
                dis=dis, norm=norm, loop_norm=dis * dis * lw)


def csr_ref(ei, w, N, degree_on):
    """What bgcn_build_graph must leave: per orientation (ptr, col, w) with the entries of a row in
    edge order and its self loop last, as float64 / int64, and dis."""
    g = gcn_norm_ref(ei, w, N, degree_on)
    out = {"dis": g["dis"]}
    ke = np.flatnonzero(g["kept"])
    for name, rows, cols in (("t", g["dst"], g["src"]), ("s", g["src"], g["dst"])):
        r = np.concatenate([rows[ke], np.arange(N)])
        order = np.argsort(r, kind="stable")                 # edge order inside a row, the loop last
        cnt = np.bincount(r, minlength=N)
        out[name + "_ptr"] = np.concatenate([[0], np.cumsum(cnt)])
        out[name + "_row"] = r[order]
        out[name + "_col"] = np.concatenate([cols[ke], np.arange(N)])[order]
        out[name + "_w"] = np.concatenate([g["norm"][ke], g["loop_norm"]])[order]
    return out


def _rowdot(a, b, dtype, order, exact, what, cols=None):
    """sum_c a[:, c] b[:, c] over the columns in `order`, accumulated one column at a time."""
    if cols is not None:
        order = [c for c in order if c < cols]
    if exact:
        assert_sum_exact(a[:, order].astype(np.float64) * b[:, order].astype(np.float64), what=what)
    acc = np.zeros(a.shape[0], dtype)
    for c in order:
        acc = acc + a[:, c] * b[:, c]
    return acc


def ew_parts_ref(ei, w, N, degree_on, h, dout, dtype=np.float64, rng=None, exact=False, mutant=None):
    """The formula of the module docstring: dict(dw [E], agg = A h, dz = A^T dout [N, F], dis, ...).
    dtype: the arithmetic of every product and sum (the graph's norm is always taken in fp64 and
    cast).  rng: take every sum in an order drawn from it (columns, and the edges of a row).
    exact: assert that every sum is exact in fp32 (the exact class).  mutant: one of MUTANTS."""
    assert mutant is None or mutant in MUTANTS
    g = gcn_norm_ref(ei, w, N, degree_on)
    h, dout = _np(h, dtype), _np(dout, dtype)
    F = h.shape[1]
    E = g["src"].size
    dis, norm, lnorm = g["dis"].astype(dtype), g["norm"].astype(dtype), g["loop_norm"].astype(dtype)
    cols = list(range(F)) if rng is None else [int(c) for c in rng.permutation(F)]
    ke = np.flatnonzero(g["kept"])
    if rng is not None:
        ke = rng.permutation(ke)
    s, d = g["src"][ke], g["dst"][ke]
    # A h and A^T dout: the loop, then the kept edges one at a time (np.add.at does not buffer)
    t_agg, t_dz = norm[ke, None] * h[s], norm[ke, None] * dout[d]
    if exact:
        assert_sum_exact(np.concatenate([t_agg, lnorm[:, None] * h]).astype(np.float64),
                         np.concatenate([d, np.arange(N)]), N, "A h")
        assert_sum_exact(np.concatenate([t_dz, lnorm[:, None] * dout]).astype(np.float64),
                         np.concatenate([s, np.arange(N)]), N, "A^T dout")
    agg, dz = lnorm[:, None] * h, lnorm[:, None] * dout
    np.add.at(agg, d, t_agg)
    np.add.at(dz, s, t_dz)
    lim = 64 if mutant == "cols_lt_64" else None
    s1 = _rowdot(dout, agg, dtype, cols, exact, "<dout, A h>", lim)
    s2 = _rowdot(h, dz, dtype, cols, exact, "<h, A^T dout>", lim)
    s3 = _rowdot(dout, h, dtype, cols, exact, "<dout, h>", lim)
    if mutant == "half_S":
        s2 = np.zeros_like(s2)
    if exact:
        assert_sum_exact(np.stack([s1, s2], -1).astype(np.float64), what="S")
    half = np.asarray(-0.5, dtype)
    dld = np.where(dis > 0, half * dis * dis * (s1 + s2), np.zeros((), dtype)).astype(dtype)
    if mutant == "no_ddeg":
        dld = np.zeros_like(dld)
    direct = s3 * dis * dis
    if exact:
        assert_sum_exact(np.stack([direct, dld], -1).astype(np.float64), what="the loop gradient")
    lgrad = direct + dld
    key = g["key"]
    if mutant == "swap_key":
        key = g["src"] if degree_on == "col" else g["dst"]
    dw = np.zeros(E, dtype)
    ke = np.flatnonzero(g["kept"])
    s, d = g["src"][ke], g["dst"][ke]
    ge = _rowdot(dout[d], h[s], dtype, cols, exact, "g_e", lim) * dis[s] * dis[d]
    if exact:
        assert_sum_exact(np.stack([ge, dld[key[ke]]], -1).astype(np.float64), what="dw")
    dw[ke] = ge + dld[key[ke]]
    le = np.flatnonzero(g["loop"])
    k = g["src"][le]
    if mutant == "loop_as_edge":       # the kept-edge line at s = d = k
        dw[le] = _rowdot(dout[k], h[k], dtype, cols, False, "", lim) * dis[k] * dis[k] + dld[key[le]]
    elif mutant == "loop_zero":
        dw[le] = 0
    elif mutant == "loop_ddeg_only":
        dw[le] = dld[k]
    else:
        dw[le] = lgrad[k]
    return dict(g, dw=dw, agg=agg, dz=dz, dldeg=dld, lgrad=lgrad)


def ew_grad_ref(ei, w, N, degree_on, h, dout, **kw):
    """d L / d edge_weight [E] in float64 for L = <dout, A_hat(edge_index, edge_weight) h>."""
    return ew_parts_ref(ei, w, N, degree_on, h, dout, **kw)["dw"]


# ------------------------------------------------------------------------------- inputs
def forest(rng, sizes, star=False, max_children=None):
    """([2, E] int64 edges (parent, child) in reference order - sorted by parent, then child -, N):
    trees of the given sizes, the nodes of a tree numbered in a row, its root first; node k hangs
    under the root (always for `star`, else half of the time) or under a random earlier node.  No
    node gets more than max_children children."""
    rows, cols, off = [], [], 0
    for n in sizes:
        nch = np.zeros(n, np.int64)
        for k in range(1, n):
            p = 0 if (star or k == 1 or rng.random() < 0.5) else int(rng.integers(1, k))
            if max_children is not None and nch[p] >= max_children:
                p = int(np.flatnonzero(nch[:k] < max_children)[0])
            nch[p] += 1
            rows.append(off + p)
            cols.append(off + k)
        off += n
    ei = np.array([rows, cols], np.int64).reshape(2, -1)
    return ei[:, np.lexsort((ei[1], ei[0]))], off


def _pow4_above(s):
    """The smallest power of four >= s + 1 (> 1)."""
    p = 4
    while p < s + 1:
        p *= 4
    return p


def _composition(rng, total, parts):
    """`parts` positive integers that sum to `total`."""
    cuts = np.sort(rng.choice(np.arange(1, total), parts - 1, replace=False)) if parts > 1 else np.array([], int)
    return np.diff(np.concatenate([[0], cuts, [total]])).astype(np.float64)


def exact_weights(rng, ei, N, degree_on, zero_weight=True, unit=False):
    """Integer weights [E] that make every degree of the tree edges `ei` a power of four.
    zero_weight: one edge weighs 0 (and the class stays exact).  unit: weights of 1 wherever a
    node's children number 4^k - 1 ('row': the stars of 255 and 1023)."""
    E = ei.shape[1]
    w = np.zeros(E)
    if degree_on == "col":
        w[:] = rng.choice([3.0, 15.0], E)
        if zero_weight and E > 2:
            w[E // 2] = 0.0
    else:
        zero_done = not zero_weight
        for p in np.unique(ei[0]):
            idx = np.flatnonzero(ei[0] == p)
            c = idx.size
            if unit and _pow4_above(c) == c + 1:
                w[idx] = 1.0
                continue
            live = idx
            if not zero_done and c >= 2:
                live, zero_done = idx[idx != idx[c // 2]], True
            total = _pow4_above(live.size) - 1
            if total == 3 and rng.random() < 0.5:
                total = 15
            w[live] = _composition(rng, total, live.size)
    return w


def exact_graph(rng, sizes, degree_on, star=False, max_children=15, zero_weight=True, unit=False):
    """(ei, w, N) of the exact class in reference order."""
    ei, N = forest(rng, sizes, star, max_children)
    return ei, exact_weights(rng, ei, N, degree_on, zero_weight, unit), N


def loop_node(ei, w, N, degree_on, max_other=3, between=True):
    """A node fit to carry the weighted input loop of `with_loop`: at least two children, the other
    weights at its key side sum to at most max_other (3: its degree stays at most 16), and
    (`between`) a run of another node that does not touch it starts somewhere past the first edge."""
    key = ei[1] if degree_on == "col" else ei[0]
    for k in np.unique(ei[0]):
        if (ei[0] == k).sum() >= 2 and w[key == k].sum() <= max_other and \
                (not between or _between_slot(ei, k) is not None):
            return int(k)
    raise AssertionError("no node fits")


def _between_slot(ei, k):
    """An index i >= 1 where a run of sources starts whose edge does not touch k, nor does the edge
    before it: a loop of k put there sits between runs of other nodes."""
    for i in range(1, ei.shape[1]):
        if ei[0, i] != ei[0, i - 1] and k not in (ei[0, i], ei[1, i], ei[0, i - 1], ei[1, i - 1]):
            return i
    return None


def with_loop(ei, w, N, degree_on, k, where):
    """(ei, w) with the input self loop (k, k) added `where`: 'inside' the run of k's own edges
    (after the first), 'between' two runs of other nodes, or at the 'tail'.  Its weight is
    4^j - (the other weights at k's key side), never 1: the degree stays a power of four."""
    key = ei[1] if degree_on == "col" else ei[0]
    other = w[key == k].sum()
    wl = _pow4_above(other + 1) - other
    assert wl > 1
    at = {"inside": int(np.flatnonzero(ei[0] == k)[0]) + 1, "between": _between_slot(ei, k),
          "tail": ei.shape[1]}[where]
    return np.insert(ei, at, k, axis=1), np.insert(w, at, wl)


def exact_features(rng, N, F):
    """Integer h and dout [N, F] in [-VMAX, VMAX], float64."""
    return (rng.integers(-VMAX, VMAX + 1, (N, F)).astype(np.float64),
            rng.integers(-VMAX, VMAX + 1, (N, F)).astype(np.float64))


def exact_case(rng, sizes, degree_on, F, loop=None, **kw):
    """(ei, w, N, h, dout, parts): an exact graph (with a weighted input loop `loop` = 'inside' /
    'between' / 'tail'), features of width F and the reference, which asserts the class's bound."""
    ei, w, N = exact_graph(rng, sizes, degree_on, **kw)
    h, dout = exact_features(rng, N, F)
    if loop:
        k = loop_node(ei, w, N, degree_on)
        ei, w = with_loop(ei, w, N, degree_on, k, loop)
        while True:     # the loop's gradient and both of its terms must show (they may not at F = 4)
            p = ew_parts_ref(ei, w, N, degree_on, h, dout)
            if h[k] @ dout[k] != 0 and p["dldeg"][k] != 0 and p["lgrad"][k] != 0:
                break
            h[k] = exact_features(rng, 1, F)[0]
    return ei, w, N, h, dout, ew_parts_ref(ei, w, N, degree_on, h, dout, exact=True)


def general_case(rng, sizes, F, star=False, loop=True, duplicate=True):
    """(ei, w, N, h, dout) of the general class; `loop` appends one input self loop, `duplicate` a
    second copy of the first edge (with a weight of its own)."""
    ei, N = forest(rng, sizes, star)
    if duplicate:
        ei = np.concatenate([ei, ei[:, :1]], 1)
    if loop:
        ei = np.concatenate([ei, [[N // 2], [N // 2]]], 1)
    E = ei.shape[1]
    w = rng.permutation(np.linspace(0.05, 2.0, E))          # distinct
    return ei, w, N, rng.standard_normal((N, F)), rng.standard_normal((N, F))


# ------------------------------------------------- the cases of tests/test_gpu_edge_weight.py
# eight trees: single nodes (isolated: no edge at all) among them; N = 365 and E = 357 (358 with
# a loop) are no multiples of 16, and 16 N / 256 = 23 blocks of node groups, the last one partial
GPU_SIZES = (1, 2, 7, 1, 40, 300, 1, 13)
GPU_WIDTHS = (4, 12, 60, 64, 68, 128, 132, 200)
GPU_LOOPS = (None, "inside", "between", "tail")
_cases = {}


def gpu_exact_case(degree_on, F, loop=None):
    """The exact case (exact_case's tuple) the GPU test of width F runs; computed once."""
    key = (degree_on, F, loop)
    if key not in _cases:
        seed = 1000 * F + 10 * GPU_LOOPS.index(loop) + (degree_on == "row")
        _cases[key] = exact_case(np.random.default_rng(seed), GPU_SIZES, degree_on, F, loop)
        ei, _, N = _cases[key][:3]
        assert N % 16 and ei.shape[1] % 16
    return _cases[key]


BUILD_ORDERS = ("reference", "shuffled", "inside", "between", "tail")
# (sizes, star): a forest with a root of about 150 children, and stars; 255 and 1023 children of
# unit weight give the root the degrees 256 and 1024 under 'row'
BUILD_GRAPHS = (((1, 2, 7, 40, 300), False), ((256,), True), ((1024,), True), ((3000,), True))


def exact_build_case(sizes, star, degree_on, order, bu):
    """(ei, w, N) of the exact class for the build test, or None where the graph has no place for
    the loop (`between` in a single star).  order: BUILD_ORDERS, the last three put one weighted
    input self loop there.  bu: the flipped (child, parent) list, the degrees taken so that the
    flipped graph is the exact one."""
    rng = np.random.default_rng(sizes[-1] + 7 * BUILD_ORDERS.index(order) + 2 * bu + (degree_on == "row"))
    on = degree_on if not bu else ("row" if degree_on == "col" else "col")
    ei, w, N = exact_graph(rng, sizes, on, star=star, max_children=None, unit=True)
    if order in ("inside", "between", "tail"):
        if star and order == "between":
            return None
        k = loop_node(ei, w, N, on, max_other=2 ** 20 if star else 3, between=not star)
        ei, w = with_loop(ei, w, N, on, k, order)
    if order == "shuffled":
        perm = rng.permutation(ei.shape[1])
        ei, w = ei[:, perm], w[perm]
    return (ei[::-1].copy() if bu else ei), w, N
