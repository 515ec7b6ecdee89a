"""Write tests/golden/compare_*.npz: tree centralities as networkx computes them and rank-similarity
matrices as scipy computes them, for the batches tests/test_compare.py and tests/test_gpu_compare.py
check bigcn_amd.compare against.  CPU only; needs networkx and scipy; the test suite only reads the
files.

The reference (compare_similarity.py:38-183) reads a centrality file per tree that a script outside
it wrote; the definition taken here is networkx's out_degree_centrality, betweenness_centrality and
closeness_centrality on the DiGraph of a tree's top-down edges with default arguments.  Its
statistics are scipy.stats.pearsonr / spearmanr / kendalltau / somersd and a set Jaccard, called
here the way its loop calls them (scipy_matrix; `--time` times that loop for tools/compare_bench.py).

Each file holds arrays only: the batch (edge_index, batch, num_graphs), `nx_centrality` [3, N] fp64,
`order` [3, N] int32 (the ranking of the CLOSED-FORM centralities: networkx's accumulation does not
give equal floats to nodes with equal integer keys, so ties are only defined there), `orders`
[V, N] int32 (the compared lists), `restatement_err` (the largest |tests/compare_ref - scipy| over
the file) and per case `sim` [B, 5, V, V], `valid` [B], `summary` [5, V, V] (+ `k`); the sweep file
compare_lists.npz holds `cases` [(k, V)] with `sim_<k>_<V>` ... computed from `orders[:V]`.

    python tools/gen_compare_golden.py
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import compare_ref as C   # noqa: E402
import explain_ref as X   # noqa: E402

LDS = 2048   # BGCN_TREE_CENTRALITY_LDS (tests/test_compare.py checks the fixture against the header)
SWEEP = ((2, 15), (5, 15), (10, 15), (32, 15), (5, 1), (2, 32), (32, 32))


# ------------------------------------------------------------------ trees: local (parent, child) lists
def chain(n, root_last=False):
    e = [(i, i + 1) for i in range(n - 1)]
    return [(n - 1 - a, n - 1 - b) for a, b in e] if root_last else e


def star(leaves):
    return [(0, i) for i in range(1, leaves + 1)]


def random_tree(n, rng, root_first=False):
    """A uniformly attached random tree whose labels are shuffled (the root is not node 0)."""
    e = [(int(rng.integers(0, i)), i) for i in range(1, n)]
    perm = rng.permutation(n)
    if root_first:
        perm = np.arange(n)
    elif perm[0] == 0:
        perm[[0, 1 % n]] = perm[[1 % n, 0]]
    return [(int(perm[a]), int(perm[b])) for a, b in e]


def make_batch(trees, rng):
    """trees: (n_nodes, edges) per tree id (n_nodes = 0: an id without nodes).  Edges shuffled."""
    src, dst, batch, first = [], [], [], 0
    for t, (n, edges) in enumerate(trees):
        batch += [t] * n
        src += [first + a for a, _ in edges]
        dst += [first + b for _, b in edges]
        first += n
    order = rng.permutation(len(src))
    ei = np.array([src, dst], dtype=np.int64).reshape(2, -1)[:, order]
    return ei, np.array(batch, dtype=np.int64), len(trees)


# ------------------------------------------------------------------ networkx / scipy
def nx_centrality(ei, batch, B):
    import networkx as nx
    out = np.zeros((3, len(batch)), dtype=np.float64)
    p = X.tree_ptr(batch, B)
    for t in range(B):
        a, b = int(p[t]), int(p[t + 1])
        if a == b:
            continue
        g = nx.DiGraph()
        g.add_nodes_from(range(a, b))
        g.add_edges_from((int(s), int(d)) for s, d in ei.T if a <= s < b)
        for r, f in enumerate((nx.out_degree_centrality, nx.betweenness_centrality, nx.closeness_centrality)):
            c = f(g)
            out[r, a:b] = [c[v] for v in range(a, b)]
    return out


def _jaccard(a, b):
    a, b = set(a), set(b)
    return len(a & b) / len(a | b)


def scipy_tree(lists):
    """One tree's [5, V, V] block the way the reference's loop fills it (:147-169): four scipy
    statistics, each called per ordered pair and read through [0] or .statistic, then Jaccard."""
    import scipy.stats as st
    V = len(lists)
    out = np.zeros((5, V, V))
    for m, f in enumerate((st.pearsonr, st.spearmanr, st.kendalltau, st.somersd)):
        for i in range(V):
            for j in range(V):
                r = f(lists[i], lists[j])
                try:
                    out[m, i, j] = r[0]
                except TypeError:
                    out[m, i, j] = r.statistic
    for i in range(V):
        for j in range(V):
            out[4, i, j] = _jaccard(lists[i], lists[j])
    return out


def scipy_matrix(orders, batch, B, k, trees=None):
    p = X.tree_ptr(batch, B)
    V = orders.shape[0]
    sim = np.zeros((B, 5, V, V))
    valid = np.zeros(B, dtype=bool)
    for t in (range(B) if trees is None else trees):
        a, b = int(p[t]), int(p[t + 1])
        if b - a <= k:      # the reference's `continue`
            continue
        valid[t] = True
        sim[t] = scipy_tree([orders[v, a:a + k].tolist() for v in range(V)])
    return sim, valid


# ------------------------------------------------------------------ the files
def lists_for(order, batch, B, V, rng):
    """V lists [V, N]: the three centrality orders, a copy of the first, its full reverse (disjoint
    top-k sets on a tree of 2 k nodes or more), the first with its first 2 / 5 / 10 / 32 entries
    reversed (a reversed top-k list), random permutations after that."""
    p = X.tree_ptr(batch, B)
    rows = [order[0], order[1], order[2], order[0].copy()]
    rev = order[0].copy()
    for t in range(B):
        rev[p[t]:p[t + 1]] = rev[p[t]:p[t + 1]][::-1]
    rows.append(rev)
    for k in (2, 5, 10, 32):
        r = order[0].copy()
        for t in range(B):
            a, b = int(p[t]), int(p[t + 1])
            m = min(k, b - a)
            r[a:a + m] = r[a:a + m][::-1]
        rows.append(r)
    while len(rows) < V:
        r = np.zeros(len(batch), dtype=np.int32)
        for t in range(B):
            r[p[t]:p[t + 1]] = rng.permutation(int(p[t + 1] - p[t]))
        rows.append(r)
    return np.stack(rows[:V]).astype(np.int32)


def case_arrays(orders, batch, B, k):
    sim, valid = scipy_matrix(orders, batch, B, k)
    mine, mine_valid = C.rank_similarity(orders, batch, B, k)
    assert np.array_equal(valid, mine_valid)
    return sim, valid, C.summarise(sim), float(np.abs(mine - sim).max())


def write(name, ei, batch, B, V, rng, k=10, sweep=None):
    nxc = nx_centrality(ei, batch, B)
    cent = C.centrality(ei, batch, B)
    rel = np.abs(cent.astype(np.float64) - nxc) / np.maximum(np.abs(nxc), 1e-300)
    assert float(np.where(nxc == 0, np.abs(cent), rel).max()) <= 2.4e-7, "closed form vs networkx"
    order = C.centrality_orders(cent, batch, B)
    orders = lists_for(order, batch, B, V, rng)
    out = {"edge_index": ei, "batch": batch, "num_graphs": np.int64(B), "nx_centrality": nxc, "order": order,
           "orders": orders}
    err = 0.0
    if sweep is None:
        sim, valid, summary, err = case_arrays(orders, batch, B, k)
        out.update(sim=sim, valid=valid, summary=summary, k=np.int64(k))
    else:
        out["cases"] = np.array(sweep, dtype=np.int64)
        for kk, vv in sweep:
            sim, valid, summary, e = case_arrays(orders[:vv], batch, B, kk)
            out.update({f"sim_{kk}_{vv}": sim, f"valid_{kk}_{vv}": valid, f"summary_{kk}_{vv}": summary})
            err = max(err, e)
    out["restatement_err"] = np.float64(err)
    path = os.path.join(ROOT, "tests", "golden", f"compare_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"{name}: N {len(batch)}, B {B}, V {V}, restatement_err {err:.3e}, {os.path.getsize(path)} bytes")


def mixed_trees(rng):
    return [(1, []), (2, chain(2)), (3, chain(3)), (0, []), (41, star(40)), (70, chain(70)),
            (33, random_tree(33, rng))]


def time_loop(B=128, mean=256, V=11, k=10, trees=8, seed=0):
    """Seconds per tree of the reference-style scipy loop on a Twitter15-shaped batch."""
    rng = np.random.default_rng(seed)
    sizes = np.maximum(k + 1, rng.poisson(mean, size=B))
    ei, batch, B = make_batch([(int(n), random_tree(int(n), rng, root_first=True)) for n in sizes], rng)
    order = C.centrality_orders(C.centrality(ei, batch, B), batch, B)
    orders = lists_for(order, batch, B, V, rng)
    t0 = time.perf_counter()
    scipy_matrix(orders, batch, B, k, trees=range(trees))
    return (time.perf_counter() - t0) / trees


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true", help="only time the scipy loop")
    args = ap.parse_args()
    if args.time:
        print(f"scipy loop, V = 11, k = 10: {time_loop():.3f} s per tree")
        return
    rng = np.random.default_rng(20)
    write("mixed", *make_batch(mixed_trees(rng), rng), 5, rng)
    long_trees = [(LDS + 5, chain(LDS + 5, root_last=True)), (12, random_tree(12, rng)),
                  (LDS + 5, random_tree(LDS + 5, rng))]
    write("long", *make_batch(long_trees, rng), 4, rng)
    ei, batch, B = make_batch(mixed_trees(np.random.default_rng(21)), rng)
    keep = np.sort(rng.choice(ei.shape[1], size=int(ei.shape[1] * (1 - 0.4)), replace=False))
    write("forest", ei[:, keep], batch, B, 5, rng)
    sizes = (2, 3, 5, 6, 10, 11, 32, 33, 64, 1)
    write("lists", *make_batch([(n, random_tree(n, rng)) for n in sizes], rng), 32, rng, sweep=SWEEP)


if __name__ == "__main__":
    main()
