"""Time EBGCN's training-loop body (model/Twitter/EBGCN.py:300-312) two ways in one process:

  step    bigcn_amd.EBGCNTrainStep.step: the training forward, bgcn_ebgcn_train_loss, backward and
          MultiAdam (one launch for the 68 parameter tensors), no host sync
  parent  what a user composed before it: EBGCN.train_forward (which ends in a host read of its
          status word) + F.nll_loss + the edge-loss terms + backward + torch.optim.Adam over the same
          five groups + max / eq / sum for the accuracy

    python tools/ebgcn_step_bench.py [--trees 128 --mean 256 --feats 768 --edge-num 2 --iters 20 --blocks 7
                                      --out profiles/ebgcn_step_bench.json]

The batch: ``--trees`` random trees of LogNormal sizes (bench.py's twitter15 shape: 128 trees of mean
256 nodes), dense fp32 features of width ``--feats`` (the reference sets args.input_features = 768), one
fixed pair of noise draws for both forms.  Both models start from the same state.  After ``--warmup``
calls of each, ``--blocks`` blocks of ``--iters`` iterations alternate between the two forms; a block is
timed on the host clock from its first call to the end of a final synchronise (the loop body is host and
device work together), and must finish within ``--limit`` seconds.  Reported: the median, minimum and
maximum of the blocks' milliseconds per iteration, and the two losses of the last iteration.
A run without a GPU fails: there is nothing to measure.  Exit status 1 when the step's median is above
the parent's.
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed_block(fn, iters, limit):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        out = fn()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if dt > limit:
        raise RuntimeError(f"a timed block took more than {limit} s")
    return 1e3 * dt / iters, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trees", type=int, default=128)
    ap.add_argument("--mean", type=float, default=256.0)
    ap.add_argument("--feats", type=int, default=768)
    ap.add_argument("--edge-num", type=int, default=2)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=float, default=60.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ebgcn_step_bench needs a ROCm GPU: nothing is measured without one")
    from bigcn_amd import EBGCN, EBGCNTrainStep
    from bigcn_amd.data import synth_batch, synth_tree_sizes

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(a.seed)
    sizes = synth_tree_sizes(rng, a.trees, a.mean)
    data = synth_batch(rng, sizes, a.feats, 4, 0.0, 0.0, device=dev)
    N, E = int(data.x.size(0)), int(data.edge_index.size(1))
    args = argparse.Namespace(input_features=a.feats, hidden_features=64, output_features=64, num_class=4,
                              edge_num=a.edge_num, edge_infer_td=True, edge_infer_bu=True, device=dev, lr=5e-4,
                              lr_scale_bu=5, lr_scale_td=1, l2=1e-4, edge_loss_td=0.2, edge_loss_bu=0.2)
    torch.manual_seed(a.seed)
    new_model = EBGCN(args).to(dev).train()
    old_model = copy.deepcopy(new_model)
    noise = (torch.randn(E, 64, device=dev), torch.randn(int(data.BU_edge_index.size(1)), 64, device=dev))

    step = EBGCNTrainStep(new_model, args=args)

    def new():
        return step.step(data, noise=noise)

    td, bu = old_model.TDrumorGCN, old_model.BUrumorGCN
    ids = {id(p) for c in (td.conv1, td.conv2, bu.conv1, bu.conv2) for p in c.parameters()}
    opt = torch.optim.Adam([
        {"params": [p for p in old_model.parameters() if id(p) not in ids]},
        {"params": bu.conv1.parameters(), "lr": args.lr / args.lr_scale_bu},
        {"params": bu.conv2.parameters(), "lr": args.lr / args.lr_scale_bu},
        {"params": td.conv1.parameters(), "lr": args.lr / args.lr_scale_td},
        {"params": td.conv2.parameters(), "lr": args.lr / args.lr_scale_td},
    ], lr=args.lr, weight_decay=args.l2)

    def old():
        logp, td_loss, bu_loss = old_model.train_forward(data, noise=noise)
        loss = F.nll_loss(logp, data.y)
        if td_loss is not None:
            loss = loss + args.edge_loss_td * td_loss
        if bu_loss is not None:
            loss = loss + args.edge_loss_bu * bu_loss
        opt.zero_grad()
        loss.backward()
        opt.step()
        _, pred = logp.max(dim=-1)
        return loss, pred.eq(data.y).sum()

    for _ in range(a.warmup):
        new()
        old()
    torch.cuda.synchronize()
    step.check_status()
    nt, ot = [], []
    for _ in range(a.blocks):   # alternate the two forms
        t, nout = timed_block(new, a.iters, a.limit)
        nt.append(t)
        t, oout = timed_block(old, a.iters, a.limit)
        ot.append(t)
    step.check_status()
    res = {
        "what": "EBGCN training-loop body, ms per iteration (host clock, each block ends in a synchronise)",
        "device": torch.cuda.get_device_name(0), "trees": a.trees, "num_nodes": N, "num_edges": E, "in_feats": a.feats,
        "edge_num": a.edge_num, "warmup": a.warmup, "blocks": a.blocks, "iters_per_block": a.iters,
        "step_ms": {"median": statistics.median(nt), "min": min(nt), "max": max(nt)},
        "parent_ms": {"median": statistics.median(ot), "min": min(ot), "max": max(ot)},
        "parent_over_step": statistics.median(ot) / statistics.median(nt),
        "last_loss": {"step": float(nout[0]), "parent": float(oout[0].detach())},
    }
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    if res["step_ms"]["median"] > res["parent_ms"]["median"]:
        raise SystemExit("the step's median is above the parent composition's")


if __name__ == "__main__":
    main()
