#!/usr/bin/env python
"""Times the EBGCN evaluation epoch two ways over the same synthetic PHEME-shaped batches:

  loop      what a user wrote by hand before ``EBGCN.validate`` existed: ``model(data)`` (one host
            sync inside), ``F.nll_loss``, ``max``, ``eq().sum().item()`` (a second sync) and the
            confusion counts per batch
  validate  ``model.validate(batches)`` + the epoch's one ``result()`` read

Shapes: F = 768 with 24 trees per batch and F = 5000 with 128 trees per batch, 8 batches each
(``bigcn_amd.data.synth_batch``).  Rounds are interleaved (loop, validate, loop, ...), the first
``--warmup`` rounds are dropped, and the medians over the rest are reported; an epoch is bracketed
by device synchronisations and its per-batch time is the epoch's wall time / 8.  Kernel launches
per batch are counted with torch's profiler (every device kernel of the process, the library's
included) over one extra epoch of each path.

Writes profiles/ebgcn_eval_step.json.  Not part of bench.py.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (("pheme768", 768, 24), ("pheme5000", 5000, 128))
BATCHES = 8


def make_batches(feats, trees, dev, seed):
    from bigcn_amd.data import synth_batch
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(BATCHES):
        sizes = np.clip(rng.lognormal(3.2, 0.9, size=trees).astype(np.int64), 2, 400)   # ~35 nodes per tree
        b = synth_batch(rng, sizes, feats, 4, 0.0, 0.0, device=dev)
        b.y = torch.as_tensor(rng.integers(0, 4, size=trees), device=dev)
        out.append(b)
    return out


def loop_epoch(model, batches):
    from bigcn_amd.metrics import confusion
    total, losses = 0, []
    counts = torch.zeros(4, 4, dtype=torch.int32, device=batches[0].x.device)
    for b in batches:
        out, _, _ = model(b)
        losses.append(F.nll_loss(out, b.y))
        _, pred = out.max(dim=1)
        total += pred.eq(b.y).sum().item()
        confusion(pred, b.y, 4, out=counts, accumulate=True)
    return total, float(torch.stack(losses).mean()), counts.cpu()


def validate_epoch(model, batches):
    r = model.validate(batches).result()
    return int(r.correct.sum()), r.loss, r.confusion


def timed(fn, *a):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(*a)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def launches(fn, *a):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn(*a)
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")
                and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
        return round(n / BATCHES, 1) if n else None
    except Exception as exc:      # a torch build without the device tracer
        print("launch count unavailable:", exc)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ebgcn_eval_step.json"))
    args = ap.parse_args()
    from bigcn_amd import EBGCN
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "batches": BATCHES, "rounds": args.rounds,
              "warmup": args.warmup, "unit": "ms per batch (epoch wall time / 8)", "shapes": {}}
    for name, feats, trees in SHAPES:
        torch.manual_seed(1)
        model = EBGCN(argparse.Namespace(input_features=feats, hidden_features=64, output_features=64, num_class=4,
                                         edge_num=2, edge_infer_td=True, edge_infer_bu=True, device=dev)).to(dev).eval()
        batches = make_batches(feats, trees, dev, seed=feats)
        t_loop, t_val = [], []
        for r in range(args.warmup + args.rounds):
            a, ra = timed(loop_epoch, model, batches)
            b, rb = timed(validate_epoch, model, batches)
            if r == 0:
                assert ra[0] == rb[0] and np.array_equal(ra[2].numpy(), rb[2]), "the two paths disagree"
                model.check_status()
            if r >= args.warmup:
                t_loop.append(a / BATCHES)
                t_val.append(b / BATCHES)
        entry = {
            "in_feats": feats, "trees_per_batch": trees,
            "nodes_per_batch": [int(b.x.size(0)) for b in batches],
            "loop_ms": t_loop, "validate_ms": t_val,
            "loop_median_ms": statistics.median(t_loop), "validate_median_ms": statistics.median(t_val),
            "loop_launches_per_batch": launches(loop_epoch, model, batches),
            "validate_launches_per_batch": launches(validate_epoch, model, batches),
        }
        entry["validate_over_loop"] = entry["validate_median_ms"] / entry["loop_median_ms"]
        result["shapes"][name] = entry
        print(name, {k: v for k, v in entry.items() if not isinstance(v, list)})
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
