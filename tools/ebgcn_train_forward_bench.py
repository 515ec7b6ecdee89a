"""Time EBGCN.train_forward + backward on a twitter15-shaped batch, and one direction's bn1 + conv2 block
alone, in two forms on the same GPU: the factored one (bigcn_amd.ebgcn_conv2_lin_train + gcn_aggregate:
no [N, 64 + F] array) and the dense composition it replaced (torch.cat, F.batch_norm, relu, gcn_conv over
the [N, 64 + F] concat), which is kept here as ``dense_block``.

    python tools/ebgcn_train_forward_bench.py [--trees 128 --mean 256 --feats 5000 --edge-num 2 --reps 20
                                               --out profiles/ebgcn_bn1_train_bench.json]

The batch is tools/ebgcn_bench.py's (``--trees`` random trees of LogNormal sizes, E = N - trees edges per
direction) with TF-IDF-like features x [N, F] (about 90 % zeros), fp32.

``step``: train_forward, then the backward of nll_loss + 0.2 (TD + BU edge loss) into every parameter.
``block``: from a given conv1 output h1 and edge_pred, bn1 + relu + conv2 (lin and aggregation), then the
backward of sum(up * h2) into h1, W2, b2, bn1's weight and bias and edge_pred.  After ``--warmup`` calls each
call is bracketed by its own pair of device events; the two forms alternate in blocks.  Reported per form:
median, 10th / 90th percentile, min and max of the per-call times, torch.cuda.max_memory_allocated over the
form's calls, the ratio of the medians, and the largest per-tensor difference between the two forms' block
results, max|a - b| / max|b|.  If the dense form runs out of memory the batch is halved (``--trees`` / 2)
for both forms and the JSON says so.  A run without a GPU fails: there is nothing to measure.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)


def stats(ms):
    a = np.sort(np.asarray(ms, dtype=np.float64))
    return {"median_ms": float(np.median(a)), "p10_ms": float(np.percentile(a, 10)), "p90_ms": float(np.percentile(a, 90)),
            "min_ms": float(a[0]), "max_ms": float(a[-1]), "calls": int(a.size)}


def timed(fn, reps):
    out = []
    for _ in range(reps):
        beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        beg.record()
        fn()
        end.record()
        end.synchronize()
        out.append(beg.elapsed_time(end))
    return out


def dense_block(d, h1, x, ei, batch, rootindex, edge_pred):
    """bn1 + relu + conv2 of one direction over the dense [N, 64 + F] concat: what
    ``_EdgeRumorGCN._train_encode`` did before ``ebgcn_conv2_lin_train``."""
    from bigcn_amd import gcn_conv
    cat = torch.cat((h1, x.index_select(0, rootindex[batch])), 1)
    bn = d.bn1
    bn.num_batches_tracked += 1
    factor = 1.0 / float(bn.num_batches_tracked) if bn.momentum is None else bn.momentum
    cat = torch.nn.functional.batch_norm(cat, bn.running_mean, bn.running_var, bn.weight, bn.bias, True, factor, bn.eps)
    return gcn_conv(torch.relu(cat), ei, d.conv2.lin.weight, d.conv2.bias, edge_weight=edge_pred,
                    degree_on=d.conv2.degree_on)


def factored_block(d, h1, x, ei, batch, rootindex, edge_pred):
    from bigcn_amd import ebgcn_conv2_lin_train, gcn_aggregate
    z2 = ebgcn_conv2_lin_train(h1, x, batch, rootindex, d.conv2.lin.weight, d.bn1)
    return gcn_aggregate(z2, ei, d.conv2.bias, edge_weight=edge_pred, degree_on=d.conv2.degree_on)


def dense_encode(d, data, noise, status):
    """``_train_encode`` with the dense block."""
    from bigcn_amd import edge_infer_train, gcn_conv, scatter_mean
    x, ei = data.x, getattr(data, d.edge_key)
    h1 = gcn_conv(x, ei, d.conv1.lin.weight, d.conv1.bias, degree_on=d.conv1.degree_on)
    loss, pred = edge_infer_train(h1, ei, d, noise=noise, status=status)
    h2 = dense_block(d, h1, x, ei, data.batch, data.rootindex, pred)
    h = torch.cat((torch.relu(h2), h1.detach().index_select(0, data.rootindex[data.batch])), 1)
    return scatter_mean(h, data.batch, dim=0, dim_size=int(data.rootindex.numel())), loss


def dense_train_forward(model, data, noise):
    status = torch.zeros(1, dtype=torch.int32, device=data.x.device)
    td_x, td_loss = dense_encode(model.TDrumorGCN, data, noise[0], status)
    bu_x, bu_loss = dense_encode(model.BUrumorGCN, data, noise[1], status)
    out = model.fc(torch.cat((bu_x, td_x), 1))
    return torch.nn.functional.log_softmax(out, dim=1), td_loss, bu_loss


def run(a, trees):
    from ebgcn_bench import make_edges
    from bigcn_amd import EBGCN

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(a.seed)
    N, ei = make_edges(rng, trees, a.mean)
    E, F_in = ei.shape[1], a.feats
    is_root = np.ones(N, dtype=bool)
    is_root[ei[1]] = False                       # a tree's nodes are contiguous, its first one the root
    batch = torch.from_numpy(np.cumsum(is_root) - 1).to(dev)
    rootindex = torch.from_numpy(np.flatnonzero(is_root)).to(dev)
    B = int(rootindex.numel())
    torch.manual_seed(a.seed)
    args = argparse.Namespace(input_features=F_in, hidden_features=64, output_features=64, num_class=4,
                              edge_num=a.edge_num, edge_infer_td=True, edge_infer_bu=True, device=dev)
    model = EBGCN(args).train()
    with torch.no_grad():   # away from the default init
        for name, mod in model.named_modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.normal_(0, 0.3)
            elif isinstance(mod, torch.nn.Conv1d):
                mod.weight.mul_(3.0)
    model = model.to(dev)
    x = torch.rand(N, F_in, device=dev) * (torch.rand(N, F_in, device=dev) < 0.1)
    tei = torch.from_numpy(ei).to(dev)
    data = argparse.Namespace(x=x, edge_index=tei, BU_edge_index=tei.flip(0).contiguous(), batch=batch,
                              rootindex=rootindex, y=torch.randint(0, 4, (B,), device=dev))
    noise = (torch.randn(E, 64, device=dev), torch.randn(E, 64, device=dev))
    params = [p for p in model.parameters()]
    d = model.TDrumorGCN
    h1 = (torch.randn(N, 64, device=dev) * 0.7).requires_grad_(True)
    pred = (torch.rand(E, device=dev) * 0.8 + 0.1).requires_grad_(True)
    up = torch.randn(N, 64, device=dev)
    wrt = [h1, d.conv2.lin.weight, d.conv2.bias, d.bn1.weight, d.bn1.bias, pred]
    last = {}

    def step(forward):
        def call():
            logp, td, bu = forward()
            loss = torch.nn.functional.nll_loss(logp, data.y) + 0.2 * (td + bu)
            torch.autograd.grad(loss, params, allow_unused=True)
        return call

    def block(form, name):
        def call():
            h2 = form(d, h1, x, tei, batch, rootindex, pred)
            last[name] = (h2,) + torch.autograd.grad((up * h2).sum(), wrt)
        return call

    forms = {
        "step": {"factored": step(lambda: model.train_forward(data, noise=noise)),
                 "dense": step(lambda: dense_train_forward(model, data, noise))},
        "block": {"factored": block(factored_block, "factored"), "dense": block(dense_block, "dense")},
    }
    res = {"what": "EBGCN train_forward + backward (step) and one direction's bn1 + conv2 block, fp32",
           "device": torch.cuda.get_device_name(0), "trees": trees, "N": N, "B": B, "E": E, "F": F_in,
           "edge_num": a.edge_num, "warmup_calls": a.warmup,
           "timer": "one pair of device events per call, forms alternating in blocks"}
    for what, pair in forms.items():
        times, peak = {"factored": [], "dense": []}, {"factored": 0, "dense": 0}
        for f in pair.values():
            for _ in range(a.warmup):
                f()
        torch.cuda.synchronize()
        for _ in range(a.blocks):                 # alternate the two forms
            for name, f in pair.items():
                torch.cuda.reset_peak_memory_stats()
                times[name] += timed(f, max(1, a.reps // a.blocks))
                peak[name] = max(peak[name], torch.cuda.max_memory_allocated())
        res[what] = {name: dict(stats(times[name]), max_memory_allocated_gib=peak[name] / 2**30) for name in pair}
        res[what]["dense_over_factored"] = res[what]["dense"]["median_ms"] / res[what]["factored"]["median_ms"]
    res["inputs_allocated_gib"] = (x.numel() * 4) / 2**30
    names = ["h2", "d_h1", "d_W2", "d_b2", "d_bn1_weight", "d_bn1_bias", "d_edge_pred"]
    res["block_max_rel_diff_factored_vs_dense"] = {
        n: float((p.detach() - q.detach()).abs().max()) / float(q.detach().abs().max())
        for n, p, q in zip(names, last["factored"], last["dense"])}
    res["requirement_block_factored_below_dense"] = bool(
        res["block"]["factored"]["median_ms"] < res["block"]["dense"]["median_ms"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trees", type=int, default=128)
    ap.add_argument("--mean", type=float, default=256.0)
    ap.add_argument("--feats", type=int, default=5000)
    ap.add_argument("--edge-num", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ebgcn_train_forward_bench needs a ROCm GPU: nothing is measured without one")
    trees = a.trees
    while True:
        try:
            res = run(a, trees)
            break
        except torch.cuda.OutOfMemoryError:
            torch.cuda.empty_cache()
            trees //= 2
            if trees == 0:
                raise
    res["batch_note"] = ("the full shape" if trees == a.trees else
                         f"out of memory at {a.trees} trees: both forms timed on {trees} trees")
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
