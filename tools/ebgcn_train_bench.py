"""Time bigcn_amd.edge_infer_train (forward + backward) on a twitter15-shaped batch against the
fp32 restatement (tests/ebgcn_train_ref.py) run eagerly by PyTorch on the same GPU.

    python tools/ebgcn_train_bench.py [--trees 128 --mean 256 --edge-num 2 --reps 50 --eager-reps 10
                                       --hub 0 --fp64-check --out profiles/ebgcn_train_bench.json]

The batch is tools/ebgcn_bench.py's: ``--trees`` random trees of LogNormal sizes (128 trees of mean
256 nodes), E = N - trees edges, h [N, 64] random, fp32.  ``--hub L`` appends one star of L leaves
(a node with L edge ends: the case the ordered dh sum is slowest on).

One call = the forward, then the backward of sum(c * edge_pred) + g * edge_loss into h, the sim
network's five parameters and fc1 - the same for both forms, allocations included.  After
``--warmup`` calls each call is bracketed by its own pair of device events; the two forms alternate
in blocks.  Reported per form: the median, the 10th / 90th percentile, min and max of the per-call
times, the HIP form's forward and backward separately, the ratio of the medians, and the largest
per-tensor difference between the two forms' results, max|a - b| / max|b| (``--fp64-check``: each
form's against the restatement in fp64 on the same inputs, one untimed call).  The eager form
materialises [E, 64, 64] tensors (about 0.5 GB each at the default shape, several per network kept
for autograd); if it runs out of memory the edge list is halved until it fits and the JSON says so.
A run without a GPU fails: there is nothing to measure.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)


def stats(ms):
    a = np.sort(np.asarray(ms, dtype=np.float64))
    return {"median_ms": float(np.median(a)), "p10_ms": float(np.percentile(a, 10)), "p90_ms": float(np.percentile(a, 90)),
            "min_ms": float(a[0]), "max_ms": float(a[-1]), "calls": int(a.size)}


def timed(fn, reps):
    """Per-call device times of ``fn`` (which may return a list of mid-call events to split at)."""
    out = []
    for _ in range(reps):
        beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        beg.record()
        mid = fn()
        end.record()
        end.synchronize()
        out.append((beg.elapsed_time(end), beg.elapsed_time(mid) if mid is not None else None))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trees", type=int, default=128)
    ap.add_argument("--mean", type=float, default=256.0)
    ap.add_argument("--edge-num", type=int, default=2)
    ap.add_argument("--hub", type=int, default=0)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--eager-reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=2)
    ap.add_argument("--skip-eager", action="store_true")
    ap.add_argument("--fp64-check", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ebgcn_train_bench needs a ROCm GPU: nothing is measured without one")
    import ebgcn_train_ref as T
    from ebgcn_bench import make_edges
    from bigcn_amd import edge_infer_train
    from bigcn_amd.ebgcn import TDrumorGCN

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(a.seed)
    N, ei = make_edges(rng, a.trees, a.mean)
    if a.hub:
        star = np.stack([np.full(a.hub, N, dtype=np.int64), N + 1 + np.arange(a.hub, dtype=np.int64)])
        ei, N = np.concatenate([ei, star], 1), N + 1 + a.hub
    E = ei.shape[1]
    torch.manual_seed(a.seed)
    args = argparse.Namespace(input_features=64, hidden_features=64, output_features=64, edge_num=a.edge_num,
                              edge_infer_td=True, edge_infer_bu=True, device=dev)
    m = TDrumorGCN(args).train()
    with torch.no_grad():   # away from the default init, where every output is ~0.5
        for name, mod in m.named_modules():
            if isinstance(mod, torch.nn.BatchNorm1d) and "norm0" in name:
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.normal_(0, 0.3)
            elif isinstance(mod, torch.nn.Conv1d):
                mod.weight.mul_(3.0)
        m.fc1.weight.mul_(4.0)
        m.fc2.weight.mul_(4.0)
    m = m.to(dev)
    h = (torch.randn(N, 64) * 0.7).to(dev).requires_grad_(True)
    ei = torch.from_numpy(ei).to(dev)
    noise, c, g = torch.randn(E, 64, device=dev), torch.randn(E, device=dev), torch.randn((), device=dev)
    params = dict(m.named_parameters())
    names = [k for k in params if k.startswith("sim_network.") or k == "fc1.weight"]
    wrt = [h] + [params[k] for k in names]
    last = {}

    def hip():
        loss, pred = edge_infer_train(h, ei, m, noise=noise)
        mid = torch.cuda.Event(enable_timing=True)
        mid.record()
        last["hip"] = (loss, pred) + torch.autograd.grad((c * pred).sum() + g * loss, wrt)
        return mid

    def eager_on(e_used):
        sd = {"TDrumorGCN." + k: v for k, v in list(m.named_parameters()) + list(m.named_buffers())}

        def eager():
            loss, pred = T.edge_infer_train(sd, "TDrumorGCN", h, ei[:, :e_used], noise[:e_used])
            last["eager"] = (loss, pred) + torch.autograd.grad((c[:e_used] * pred).sum() + g * loss, wrt)
        return eager

    for _ in range(a.warmup):
        hip()
    torch.cuda.synchronize()
    e_used, eager = E, None
    if not a.skip_eager:
        while eager is None:
            try:
                f = eager_on(e_used)
                for _ in range(a.warmup):
                    f()
                torch.cuda.synchronize()
                eager = f
            except torch.cuda.OutOfMemoryError:
                last.pop("eager", None)
                torch.cuda.empty_cache()
                e_used //= 2
                if e_used == 0:
                    raise
    ht, et = [], []
    for _ in range(a.blocks):                 # alternate the two forms
        ht += timed(hip, max(1, a.reps // a.blocks))
        if eager is not None:
            et += timed(eager, max(1, a.eager_reps // a.blocks))
    res = {"what": "edge_infer_train forward + backward, fp32", "device": torch.cuda.get_device_name(0),
           "trees": a.trees, "hub": a.hub, "N": N, "E": E, "edge_num": a.edge_num, "warmup_calls": a.warmup,
           "timer": "one pair of device events per call, forms alternating in blocks",
           "hip": stats([t for t, _ in ht]), "hip_forward": stats([f for _, f in ht]),
           "hip_backward": stats([t - f for t, f in ht])}
    if eager is not None:
        res["eager"] = stats([t for t, _ in et])
        res["eager_edges"] = e_used
        res["eager_note"] = ("the full shape" if e_used == E else
                             f"out of memory at E = {E}: timed on the first {e_used} edges; the ratio is NOT like for like")
        res["eager_over_hip"] = res["eager"]["median_ms"] / res["hip"]["median_ms"]
        if e_used == E:
            diff = 0.0
            for x, y in zip(last["hip"], last["eager"]):
                diff = max(diff, float((x.detach() - y.detach()).abs().max()) / float(y.detach().abs().max()))
            res["max_rel_diff_hip_vs_eager"] = diff
        res["eager_peak_gib"] = torch.cuda.max_memory_allocated() / 2**30
        if a.fp64_check and e_used == E:
            # both forms against the restatement in fp64 on the same inputs (one call, not timed)
            sd64 = {"TDrumorGCN." + k: v.detach().double() if v.is_floating_point() else v
                    for k, v in list(m.named_parameters()) + list(m.named_buffers())}
            w64 = [h.detach().double().requires_grad_(True)]
            for k in names:
                sd64["TDrumorGCN." + k] = sd64["TDrumorGCN." + k].requires_grad_(True)
                w64.append(sd64["TDrumorGCN." + k])
            loss, pred = T.edge_infer_train(sd64, "TDrumorGCN", w64[0], ei, noise.double())
            ref = (loss, pred) + torch.autograd.grad((c.double() * pred).sum() + g.double() * loss, w64)
            what = ["edge_loss", "edge_pred", "d_h"] + ["d_" + k for k in names]
            res["rel_err_vs_fp64"] = {
                form: {w: float((x.detach() - y).abs().max()) / float(y.abs().max())
                       for w, x, y in zip(what, last[form], ref)} for form in ("hip", "eager")}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
