"""Time bigcn_amd.explain() on a twitter15-shaped batch against the same analysis written with
plain torch ops on the same GPU, and the pass over X of bgcn_explain_sums against HBM's peak.

    python tools/explain_bench.py [--trees 128 --mean 256 --feats 5000 --iters 20 --out profiles/explain.txt]

The batch: ``--trees`` random trees of LogNormal sizes (bench.py's twitter15 shape: 128 trees of
mean 256 nodes), bag-of-words X [N, feats] fp32, a BiGCN with its default init in eval mode.
The torch form is the reference's op sequence (explain_PHEME.py:91-162, :530-533) for the whole
batch - both concatenations materialised per direction - with gcn_norm / propagate as
index_add_ and the per-tree topk as two stable sorts (by value, then by tree).  Both forms are
warmed up, then timed with device events over ``--iters`` calls in alternating blocks; each
timed block ends in a synchronise and must finish within ``--limit`` seconds.

Reported: ms per call (median and min-max of the blocks); whether the two forms rank alike; the
X pass alone (ops.explain_sums with and without x_sum, the difference being the pass) as a
fraction of the HBM3E peak, 8.0 TB/s by specification and 6.29 TB/s measured for a float4 copy.
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

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12


def _gcn(x, ei, w, b):
    N = x.size(0)
    loops = torch.arange(N, device=x.device)
    row, col = torch.cat((ei[0], loops)), torch.cat((ei[1], loops))
    deg = torch.zeros(N, device=x.device).index_add_(0, col, torch.ones(col.numel(), device=x.device))
    dinv = deg.pow(-0.5)
    h = x @ w.t()
    return torch.zeros(N, w.size(0), device=x.device).index_add_(0, col, h[row] * (dinv[row] * dinv[col])[:, None]) + b


def _rank(values, batch, first):
    """Per-tree descending order with ties by ascending index: two stable sorts."""
    i1 = torch.argsort(values, dim=-1, descending=True, stable=True)
    i2 = torch.argsort(batch[i1], dim=-1, stable=True)
    order = torch.gather(i1, -1, i2)
    return order - first[batch], torch.gather(values, -1, order)


def torch_form(model, data, first):
    x, batch = data.x, data.batch
    root = data.rootindex[batch]
    out = [_rank(x.sum(-1), batch, first)]
    for mod, ei in ((model.TDrumorGCN, data.edge_index), (model.BUrumorGCN, data.BU_edge_index)):
        h1 = _gcn(x, ei, mod.conv1.lin.weight, mod.conv1.bias)
        cat = torch.cat((h1, x[root]), 1)
        c2in = torch.relu(cat)
        h2 = _gcn(c2in, ei, mod.conv2.lin.weight, mod.conv2.bias)
        smi = torch.cat((torch.relu(h2), h1[root]), 1)
        sums = torch.stack((h1.sum(-1), cat.sum(-1), c2in.sum(-1), h2.sum(-1), smi.sum(-1)))
        gcn_out = torch.zeros(first.numel(), 128, device=x.device).index_add_(0, batch, smi)
        out.append((sums,) + _rank(sums, batch, first) + (gcn_out,))
    return out


def timed_block(fn, iters, limit):
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.monotonic()
    beg.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    if time.monotonic() - t0 > limit:
        raise RuntimeError(f"a timed block took more than {limit} s")
    return beg.elapsed_time(end) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trees", type=int, default=128)
    ap.add_argument("--mean", type=float, default=256.0)
    ap.add_argument("--feats", type=int, default=5000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--limit", type=float, default=60.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("explain_bench needs a ROCm GPU: nothing is measured without one")
    from bigcn_amd import BiGCN, explain, ops
    from bigcn_amd.data import synth_batch, synth_tree_sizes

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(a.seed)
    sizes = synth_tree_sizes(rng, a.trees, a.mean)
    data = synth_batch(rng, sizes, a.feats, 4, device=dev, root_random=True)
    torch.manual_seed(a.seed)
    model = BiGCN(a.feats, 64, 64, dev).eval().to(dev)
    N = data.x.size(0)
    first = torch.searchsorted(data.batch, torch.arange(a.trees, device=dev))

    with torch.no_grad():
        k = lambda: explain(model, data)                 # noqa: E731
        t = lambda: torch_form(model, data, first)       # noqa: E731
        for _ in range(3):
            ex, ref = k(), t()
        torch.cuda.synchronize()
        same_x = bool(torch.equal(ex.x_order.long(), ref[0][0]))
        agree, err = [], 0.0
        for res, (sums, order, _, _) in ((ex.td, ref[1]), (ex.bu, ref[2])):
            agree.append(float((res.order.long() == order).float().mean()))
            err = max(err, float((res.sums - sums).abs().max()))
        kt, tt = [], []
        for _ in range(a.blocks):
            kt.append(timed_block(k, a.iters, a.limit))
            tt.append(timed_block(t, a.iters, a.limit))
        # the X pass: explain_sums with x_sum minus explain_sums without
        h = torch.randn(N, 64, device=dev)
        args = (h, h, data.x, data.batch, data.rootindex)
        w = lambda: ops.explain_sums(*args)                          # noqa: E731
        wo = lambda: ops.explain_sums(*args, want_x_sum=False)       # noqa: E731
        for _ in range(3):
            w(), wo()
        torch.cuda.synchronize()
        wt = statistics.median(timed_block(w, a.iters, a.limit) for _ in range(a.blocks))
        wot = statistics.median(timed_block(wo, a.iters, a.limit) for _ in range(a.blocks))
    km, tm = statistics.median(kt), statistics.median(tt)
    nbytes = N * a.feats * 4
    xpass = max(wt - wot, 1e-6) * 1e-3
    lines = [
        f"explain(), BiGCN, fp32, twitter15-shaped batch: trees={a.trees} N={N} F={a.feats} "
        f"device={torch.cuda.get_device_name(0)}",
        f"  timing: device events, {a.blocks} alternating blocks of {a.iters} calls, 3 warm-up calls each",
        f"  bigcn_amd.explain (both directions, x_sum, rankings, the model's forward): {km:.3f} ms/call "
        f"(min {min(kt):.3f}, max {max(kt):.3f})",
        f"  plain torch ops, same analysis (without the model's forward): {tm:.3f} ms/call "
        f"(min {min(tt):.3f}, max {max(tt):.3f})",
        f"  torch / explain: {tm / km:.2f}x",
        f"  agreement: x_sum ranking identical: {same_x}; stage ranks equal at {min(agree):.4f} of the slots "
        f"(sums differ by up to {err:.2e}: near-ties may swap)",
        f"  explain_sums with x_sum {wt:.4f} ms, without {wot:.4f} ms: the pass over X ({nbytes / 1e9:.3f} GB) "
        f"takes {xpass * 1e3:.4f} ms = {nbytes / xpass / 1e12:.2f} TB/s = {nbytes / xpass / HBM_SPEC:.2f} of the "
        f"8.0 TB/s specification, {nbytes / xpass / HBM_COPY:.2f} of the 6.29 TB/s a float4 copy reaches",
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
