"""Numpy restatement of what bigcn_amd.compare computes (the reference's compare_similarity.py
:38-214 plus the tree centralities its missing generator wrote), in this project's own words.
TEST INFRASTRUCTURE: the exact oracle of tests/test_gpu_compare.py; tests/test_compare.py pins it
to fixtures that networkx and scipy produced (tools/gen_compare_golden.py).

* centralities: the closed forms of networkx's out_degree / betweenness / closeness centrality on
  a forest, from a parent walk: integers c (children), d (depth), s (subtree size), n (the tree's
  node count), then ONE fp64 division rounded once to fp32;
* the five statistics by integer sums over the k distinct entries of two lists (no ties), then one
  fp64 division (after one sqrt for Pearson and Spearman);
* summarise: sum over trees / count_nonzero.
Ranking goes through tests/explain_ref.segment_rank.
"""
import numpy as np

import explain_ref as X

CENTRALITY_NAMES = ("out_degree", "betweenness", "closeness")
METRIC_NAMES = ("pearsonr", "spearmanr", "kendalltau", "somersd", "jaccard")
# compare_similarity.py:43-45, the eleven names that are not BERT's
REFERENCE_NAMES = ("out_degree", "betweenness", "closeness",
                   "bigcn_td_conv1", "bigcn_td_conv2", "bigcn_bu_conv1", "bigcn_bu_conv2",
                   "ebgcn_td_conv1", "ebgcn_td_conv2", "ebgcn_bu_conv1", "ebgcn_bu_conv2")


# ---- fixtures (tests/golden/compare_*.npz) and the bars the CPU and GPU tests share
ULP2 = 2.4e-7      # two fp32 ulps, relative


def cases_of(z):
    """(k, V, sim, valid, summary) of every case a fixture holds."""
    if "cases" not in z.files:
        return [(int(z["k"]), z["orders"].shape[0], z["sim"], z["valid"], z["summary"])]
    return [(int(k), int(v), z[f"sim_{k}_{v}"], z[f"valid_{k}_{v}"], z[f"summary_{k}_{v}"]) for k, v in z["cases"]]


def similarity_bar(z):
    """Pearson / Spearman against scipy: 16x the restatement's own distance from scipy, measured on
    the CPU when the fixture was written; the floor is 32 terms of fp64 rounding with a wide margin."""
    return max(16.0 * float(z["restatement_err"]), 1e-12)


def tree_integers(edge_index: np.ndarray, batch: np.ndarray, B: int):
    """(c, d, s, n) int64 [N] each: children, depth, subtree size (itself included) inside the
    node's component, and the node's tree's node count.  The edges must form a forest."""
    N = len(batch)
    par = np.full(N, -1, dtype=np.int64)
    c = np.zeros(N, dtype=np.int64)
    for s_, d_ in zip(edge_index[0].tolist(), edge_index[1].tolist()):
        assert par[d_] == -1 and batch[s_] == batch[d_]
        par[d_] = s_
        c[s_] += 1
    d = np.zeros(N, dtype=np.int64)
    s = np.zeros(N, dtype=np.int64)
    for v in range(N):
        u, steps = v, 0
        s[u] += 1
        while par[u] >= 0:
            u = par[u]
            steps += 1
            assert steps < N, "cycle"
            s[u] += 1
        d[v] = steps
    n = np.bincount(batch, minlength=B)[batch].astype(np.int64)
    return c, d, s, n


def centrality(edge_index: np.ndarray, batch: np.ndarray, B: int) -> np.ndarray:
    """[3, N] float32, rows CENTRALITY_NAMES."""
    c, d, s, n = tree_integers(np.asarray(edge_index), np.asarray(batch), B)
    out = np.zeros((3, len(batch)), dtype=np.float64)
    m = n > 1
    out[0] = 1.0
    out[0, m] = c[m].astype(np.float64) / (n[m] - 1).astype(np.float64)
    m = n > 2
    out[1, m] = (d[m] * (s[m] - 1)).astype(np.float64) / ((n[m] - 1) * (n[m] - 2)).astype(np.float64)
    m = d > 0
    out[2, m] = (2 * d[m]).astype(np.float64) / ((d[m] + 1) * (n[m] - 1)).astype(np.float64)
    return out.astype(np.float32)


def centrality_orders(cent: np.ndarray, batch: np.ndarray, B: int) -> np.ndarray:
    return X.segment_rank(cent, batch, B)[0]


def _pair_sums(x, y):
    """(sum over a < b of (x_a - x_b)(y_a - y_b), of sign(x_a - x_b) sign(y_a - y_b)) as ints."""
    x, y = np.asarray(x, dtype=np.int64), np.asarray(y, dtype=np.int64)
    dx, dy = x[:, None] - x[None, :], y[:, None] - y[None, :]
    upper = np.triu(np.ones((len(x), len(x)), dtype=bool), 1)
    return int((dx * dy)[upper].sum()), int((np.sign(dx) * np.sign(dy))[upper].sum())


def _ranks(x):
    x = np.asarray(x)
    return (x[None, :] < x[:, None]).sum(1)


def pair_metrics(x, y) -> np.ndarray:
    """The five statistics of two lists of k distinct integers."""
    k = len(x)
    assert len(y) == k and len(set(x)) == k and len(set(y)) == k
    cxy, conc = _pair_sums(x, y)
    cxx, cyy = _pair_sums(x, x)[0], _pair_sums(y, y)[0]
    rx, ry = _ranks(x), _ranks(y)
    rxy, rxx, ryy = _pair_sums(rx, ry)[0], _pair_sums(rx, rx)[0], _pair_sums(ry, ry)[0]
    m = len(set(x) & set(y))
    f = np.float64
    tau = f(conc) / f(k * (k - 1) // 2)
    return np.array([f(cxy) / np.sqrt(f(cxx) * f(cyy)), f(rxy) / np.sqrt(f(rxx) * f(ryy)), tau, tau,
                     f(m) / f(2 * k - m)], dtype=np.float64)


def rank_similarity(orders: np.ndarray, batch: np.ndarray, B: int, k: int):
    """(sim float64 [B, 5, V, V], valid bool [B]) of the V rankings ``orders`` [V, N]."""
    orders = np.asarray(orders)
    V = orders.shape[0]
    p = X.tree_ptr(np.asarray(batch), B)
    sim = np.zeros((B, 5, V, V), dtype=np.float64)
    valid = np.zeros(B, dtype=bool)
    for t in range(B):
        a, b = int(p[t]), int(p[t + 1])
        if b - a <= k:
            continue
        valid[t] = True
        lists = [orders[v, a:a + k].tolist() for v in range(V)]
        for i in range(V):
            for j in range(i, V):
                sim[t, :, i, j] = sim[t, :, j, i] = pair_metrics(lists[i], lists[j])
    return sim, valid


def summarise(mat: np.ndarray) -> np.ndarray:
    """compare_similarity.py:205 for every entry: NaN where no tree has a nonzero value."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return mat.sum(0) / np.count_nonzero(mat, axis=0)
