"""Time the batched LSTM evaluation (bigcn_amd.LSTM.evaluate, one native call per batch) against the
reference's form on the same GPU, weights and batch: the per-tree Python loop of torch.nn.LSTM
(model/Twitter/LSTM_Twitter.py:146-173, with its rootindex.tolist() sync).

    python tools/lstm_bench.py --out profiles/lstm_eval.json

    python tools/lstm_bench.py --train --out profiles/lstm_train.json

--train times the training-loop body instead: bigcn_amd.LSTMTrainStep.step (one native call for
forward, loss and backward, one Adam launch) against the reference's own body on the same GPU,
weights and batch (LSTM_Twitter.py:96-126: nn.LSTM per tree, nll_loss, backward, torch.optim.Adam).

Two batches: the PHEME shape (B = 24, LSTM(768, 768, 4, 2), tree sizes from synth_tree_sizes at
mean 64) and B = 128 at the Twitter configuration (LSTM(5000, 64, 64, 2)).  Times are host clocks
around work that ends in a device synchronise, after a warm-up of every shape.  There is no
fallback: without a GPU the script fails."""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bigcn_amd import LSTM, LSTMTrainStep                    # noqa: E402
from bigcn_amd.data import synth_tree_sizes                  # noqa: E402
from bigcn_amd.lstm import max_sequence_len                  # noqa: E402


@torch.no_grad()
def reference_loop(lstm, fc, data, out_feats):
    """One batch of the reference's test loop, as written there (version 2)."""
    rootindices = data.rootindex.tolist()
    val_out = torch.zeros(data.y.shape[0], out_feats, device=data.cls.device)
    for k, r in enumerate(rootindices):
        sl = data.cls[r:] if k == len(rootindices) - 1 else data.cls[r:rootindices[k + 1]]
        _, (h_n, _) = lstm(sl)
        val_out[k] = F.log_softmax(fc(h_n.reshape(-1, fc.in_features)), dim=1)
    loss = F.nll_loss(val_out, data.y)
    pred = val_out.max(dim=1)[1]
    return val_out, loss.item(), pred.eq(data.y).sum().item()


def reference_train_body(lstm, fc, opt, data, out_feats):
    """One iteration of the reference's training loop, as written there (version 2)."""
    rootindices = data.rootindex.tolist()
    rows = []
    for k, r in enumerate(rootindices):
        sl = data.cls[r:] if k == len(rootindices) - 1 else data.cls[r:rootindices[k + 1]]
        _, (h_n, _) = lstm(sl)
        rows.append(F.log_softmax(fc(h_n.reshape(-1, fc.in_features)), dim=1))
    out = torch.cat(rows)
    loss = F.nll_loss(out, data.y)
    opt.zero_grad()
    loss.backward()
    opt.step()
    pred = out.max(dim=1)[1]
    return loss.item(), pred.eq(data.y).sum().item()


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def batch(cfg, B, seed):
    """The seeded batch and model of one shape: ``(data, N, max_len, model)``, the model in eval mode."""
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(seed)
    sizes = synth_tree_sizes(rng, B, 64)
    N = int(sizes.sum())
    g = torch.Generator().manual_seed(seed)
    cls = torch.randn(N, cfg[0], generator=g)
    root_cpu = torch.tensor(np.concatenate(([0], np.cumsum(sizes)[:-1])), dtype=torch.int64)
    max_len = max_sequence_len(root_cpu, N)                  # from the CPU batch, before the copy
    data = SimpleNamespace(cls=cls.to(dev), rootindex=root_cpu.to(dev),
                           y=torch.randint(0, cfg[2], (B,), generator=g).to(dev))
    torch.manual_seed(seed)
    return data, N, max_len, LSTM(*cfg, version=2).to(dev).eval()


def run(name, cfg, B, seed, warmup, iters, ref_iters):
    data, N, max_len, model = batch(cfg, B, seed)
    dev = data.cls.device
    logp = torch.empty(B, cfg[2], device=dev)
    ours = timed(lambda: model.evaluate(data, logp=logp, max_len=max_len), warmup, iters)
    model.check_status()
    ref = timed(lambda: reference_loop(model.lstm, model.fc, data, cfg[2]), 1, ref_iters)
    want, _, _ = reference_loop(model.lstm, model.fc, data, cfg[2])
    launches = cfg[3] * max_len
    return {"batch": name, "config": list(cfg), "B": B, "N": N, "max_len": max_len,
            "batched_ms_median": ours[0], "batched_ms_min": ours[1],
            "reference_loop_ms_median": ref[0], "reference_loop_ms_min": ref[1],
            "ratio_reference_over_batched": ref[0] / ours[0],
            "step_launches": launches,
            "batched_us_per_step_launch": 1e3 * ours[0] / launches,   # the whole call over its step launches
            "max_abs_logp_diff_vs_reference": float((logp - want).abs().max())}


def run_train(name, cfg, B, seed, warmup, iters, ref_iters):
    data, N, max_len, model = batch(cfg, B, seed)
    dev = data.cls.device
    model.train()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    step = LSTMTrainStep(model)
    first = float(step.step(data, max_len=max_len)[0])        # the first loss, on the initial weights
    ours = timed(lambda: step.step(data, max_len=max_len), warmup, iters)
    skipped = step.check_status()
    ref_model = LSTM(*cfg, version=2).to(dev).train()
    ref_model.load_state_dict(sd)
    opt = torch.optim.Adam(ref_model.parameters(), lr=5e-4, weight_decay=1e-4)
    ref_first, _ = reference_train_body(ref_model.lstm, ref_model.fc, opt, data, cfg[2])
    ref = timed(lambda: reference_train_body(ref_model.lstm, ref_model.fc, opt, data, cfg[2]), 1, ref_iters)
    launches = 2 * cfg[3] * max_len                            # forward and backward steps
    return {"batch": name, "config": list(cfg), "B": B, "N": N, "max_len": max_len,
            "train_step_ms_median": ours[0], "train_step_ms_min": ours[1],
            "reference_body_ms_median": ref[0], "reference_body_ms_min": ref[1],
            "ratio_reference_over_step": ref[0] / ours[0],
            "step_launches": launches,
            "train_step_us_per_step_launch": 1e3 * ours[0] / launches,
            "updates_skipped": skipped,
            "first_loss": first, "first_loss_reference": ref_first}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train", action="store_true", help="time the training-loop body (LSTMTrainStep.step)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--ref-iters", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lstm_bench needs a ROCm GPU (no fallback)")
    fn = run_train if a.train else run
    if a.out is None:
        a.out = os.path.join("profiles", "lstm_train.json" if a.train else "lstm_eval.json")
    res = {"device": torch.cuda.get_device_name(0), "mode": "train" if a.train else "eval", "batches": [
        fn("pheme", (768, 768, 4, 2), 24, 1, a.warmup, a.iters, a.ref_iters),
        fn("twitter", (5000, 64, 64, 2), 128, 2, a.warmup, a.iters, a.ref_iters)]}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
