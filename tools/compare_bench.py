"""Time bigcn_amd.compare() on a twitter15-shaped batch, and the reference-style scipy loop on the
same batch's rankings on the same host.

    python tools/compare_bench.py [--trees 128 --mean 256 --feats 5000 --k 10 --iters 20 --out profiles/compare.txt]

The batch: ``--trees`` random trees of LogNormal sizes (bench.py's twitter15 shape: 128 trees of
mean 256 nodes), bag-of-words X [N, feats] fp32, a BiGCN and an EBGCN with their default init in
eval mode: V = 11 rankings (three centralities, four stages per model), the reference's list
without its BERT columns.  Every form is warmed up, then timed with device events over ``--iters``
calls in ``--blocks`` blocks; each block ends in a synchronise and must finish within ``--limit``
seconds.

Reported, ms per call (median and min-max of the blocks): explain() of the two models (not new);
compare() given their Explanations (centralities, their ranking, the similarity kernel, one host
sync); bgcn_tree_centrality and bgcn_rank_similarity alone.  Then the CPU: the reference's loop
(tools/gen_compare_golden.py scipy_matrix: 11 x 11 x 4 scipy calls and 121 set operations per tree)
over the first ``--cpu-trees`` trees of the same rankings, seconds per tree and scaled to the batch.
A run without a GPU fails: there is nothing to measure.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from explain_bench import timed_block   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trees", type=int, default=128)
    ap.add_argument("--mean", type=float, default=256.0)
    ap.add_argument("--feats", type=int, default=5000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--limit", type=float, default=60.0)
    ap.add_argument("--cpu-trees", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("compare_bench needs a ROCm GPU: nothing is measured without one")
    from bigcn_amd import EBGCN, BiGCN, compare, explain, ops
    from bigcn_amd.data import synth_batch, synth_tree_sizes

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(a.seed)
    sizes = synth_tree_sizes(rng, a.trees, a.mean)
    data = synth_batch(rng, sizes, a.feats, 4, device=dev, root_random=True)
    torch.manual_seed(a.seed)
    models = {"bigcn": BiGCN(a.feats, 64, 64, dev).eval().to(dev),
              "ebgcn": EBGCN(argparse.Namespace(input_features=a.feats, hidden_features=64, output_features=64,
                                                num_class=4, edge_num=2, edge_infer_td=True, edge_infer_bu=True,
                                                device=dev)).eval().to(dev)}
    N, B = data.x.size(0), a.trees

    with torch.no_grad():
        ex = {name: explain(m, data) for name, m in models.items()}
        sim = compare(data, ex, k=a.k)
        orders = torch.cat([sim.centrality_order] + [d.order[[d.stage_names.index(s) for s in
                                                              ("conv1_output_sum", "conv2_output_sum")]]
                                                     for e in ex.values() for d in (e.td, e.bu)]).contiguous()
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        forms = {
            "explain() x 2 models": lambda: [explain(m, data) for m in models.values()],
            "compare() given the Explanations": lambda: compare(data, ex, k=a.k),
            "bgcn_tree_centrality": lambda: ops._tree_centrality(data.edge_index, data.batch, B, status),
            "bgcn_rank_similarity": lambda: ops._rank_similarity(orders, data.batch, a.k, B, status),
        }
        times = {}
        for name, fn in forms.items():
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            times[name] = [timed_block(fn, a.iters, a.limit) for _ in range(a.blocks)]
        assert int(status.item()) == 0

    import gen_compare_golden as G
    o, bt = orders.cpu().numpy(), data.batch.cpu().numpy()
    kept = [t for t in range(B) if sizes[t] > a.k][:a.cpu_trees]
    t0 = time.perf_counter()
    ref, _ = G.scipy_matrix(o, bt, B, a.k, trees=kept)
    per_tree = (time.perf_counter() - t0) / len(kept)
    err = float(np.abs(sim.matrix.cpu().numpy()[kept] - ref[kept]).max())

    lines = [f"compare on the MI355X: {B} trees, {N} nodes (mean {N / B:.0f}), F = {a.feats}, V = {orders.size(0)} "
             f"rankings, k = {a.k}; {int(sim.valid.sum())} trees kept",
             f"(device-event time per call, {a.iters} calls per block, {a.blocks} blocks: median [min - max])"]
    for name, ts in times.items():
        lines.append(f"  {name:36s} {statistics.median(ts):8.4f} ms [{min(ts):.4f} - {max(ts):.4f}]")
    lines += [f"the reference-style scipy loop on this host's CPU, same rankings, {len(kept)} trees: "
              f"{per_tree:.3f} s per tree = {per_tree * int(sim.valid.sum()):.1f} s for the batch's kept trees",
              f"  max |compare - scipy| over those trees: {err:.3e}"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
