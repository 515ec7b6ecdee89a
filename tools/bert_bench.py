"""Time the batched TreeBERT calls (bigcn_amd.TreeBERT, one native call per batch) against the
reference's form on the same GPU, weights and batch: the per-tree Python loop of the full 12-layer
encoder (model/Twitter/BERT_Twitter.py:127-150, with its rootindex.tolist() sync).

    python tools/bert_bench.py --out profiles/bert_eval.json

One batch at the PHEME shape: B = 24 trees (sizes from synth_tree_sizes at mean 64, capped at 512),
rows of T x 768 values pooled to 768, BERT-base sizes (12 layers, 768 wide, 12 heads, 3072
intermediate), random weights.  Timed: ``evaluate`` (the root-only form), the full-form call
(``forward_batch(..., return_hidden=True, return_sums=True)`` on the pooled rows) and the reference
loop - ``transformers``' BertModel where importable, else the fp32 torch restatement of
tests/bert_ref.py.  The root-only call is bound by the weight bytes it reads once per call; its
achieved fraction of the HBM peak is reported against them.  Times are host clocks around work that
ends in a device synchronise, after a warm-up.  There is no fallback: without a GPU the script fails.

    python tools/bert_bench.py --weights both

times ``evaluate`` on the fp32 parameters and on bf16 weight images (``TreeBERT.use_weight_images("bf16")``:
half the weight bytes, read by the split-K kernel of ``bgcn_bert_eval_w16``) in one process on the same
batch, and writes profiles/bert_eval_w16.json: medians, min / max, the weight bytes a call reads and their
share of the 8 TB/s HBM peak per leg.

    python tools/bert_bench.py --train --out profiles/bert_train.json

times one training step (``TreeBERTTrainStep.step``: root rows pooled, ``bgcn_bert_train_grad`` at
dropout 0.1 / 0.1, the Adam launches) on the same batch, in windows of ``--window`` steps with one
synchronise each, and ``grad_batch`` alone.  Beside the time stand the bytes a step cannot avoid
moving at B = 24: every weight the chain reads, twice (forward, and dX = dY W in the backward), every
dW written once, and Adam's traffic (gradient, parameter and both moments read, parameter and both
moments written) over all tensors that get a gradient; the activations ([24, width] rows) are left
out.  Their quotient by the HBM peak is the floor the step time is compared with.

    python tools/bert_bench.py --train --gemm both

times the same step and ``grad_batch`` on both GEMM paths (``gemm="tiled"``, the default path, and
``gemm="skinny"``, the split fp32 kernels of ``bgcn_bert_train_grad_skinny``) in one process on twin models
and the same batch, the windows of the two legs interleaved, and writes profiles/bert_train_skinny.json:
per leg the median and min / max, the bytes of ``train_bytes`` and the achieved GB/s.  The skinny leg counts
as a gain only when its median lies below the tiled leg's minimum."""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bigcn_amd import TreeBERT, TreeBERTTrainStep            # noqa: E402
from bigcn_amd.data import synth_tree_sizes                  # noqa: E402

HBM_PEAK_GBS = 8000.0   # MI355X: 8 TB/s


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
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "max_ms": float(np.max(ts))}


def reference(model):
    """``(which, encode)``: encode(rows [n, 768]) -> pooler_output [768] of one tree."""
    sd = {k: v for k, v in model.state_dict().items()}
    try:
        import transformers as tr
    except ImportError:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import bert_ref
        return "torch restatement (tests/bert_ref.py), fp32", lambda rows: torch.tanh(F.linear(
            bert_ref.encode(sd, rows, model.num_layers, model.heads)[0][0], sd["BERT.pooler.dense.weight"],
            sd["BERT.pooler.dense.bias"]))
    cfg = tr.BertConfig(vocab_size=sd["BERT.embeddings.word_embeddings.weight"].size(0), hidden_size=model.hidden,
                        num_hidden_layers=model.num_layers, num_attention_heads=model.heads,
                        intermediate_size=model.intermediate, max_position_embeddings=model.max_pos, is_decoder=True)
    bert = tr.BertModel(cfg).to(model.fc.weight.device).eval()
    bert.load_state_dict({k[5:]: v for k, v in sd.items() if k.startswith("BERT.")}, strict=False)
    return f"transformers {tr.__version__} BertModel(is_decoder=True), fp32", \
        lambda rows: bert(inputs_embeds=rows.unsqueeze(0)).pooler_output[0]


@torch.no_grad()
def reference_loop(model, encode, data, rows):
    """One batch of the reference's test loop, as written there (pooled rows given)."""
    rootindices = data.rootindex.tolist()
    out = torch.zeros(data.y.shape[0], model.num_classes, device=rows.device)
    for k, r in enumerate(rootindices):
        sl = rows[r:] if k == len(rootindices) - 1 else rows[r:rootindices[k + 1]]
        out[k] = F.log_softmax(model.fc(encode(sl)), dim=-1)
    loss = F.nll_loss(out, data.y)
    return out, loss.item(), out.max(dim=1)[1].eq(data.y).sum().item()


def timed_windows(fn, warmup, windows, steps):
    """ms per call of ``fn`` over windows of ``steps`` calls that end in one device synchronise."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3 / steps)
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "max_ms": float(np.max(ts)),
            "windows": windows, "steps_per_window": steps}


def timed_windows_interleaved(fns, warmup, windows, steps):
    """``timed_windows`` for several callables at once: window k of every one before window k + 1 of any."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) * 1e3 / steps)
    return {k: {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v)),
                "windows": windows, "steps_per_window": steps} for k, v in ts.items()}


def train_bytes(model):
    """The bytes one training step must move at a small B, from the shapes alone."""
    by_name = dict(model.named_parameters())
    names = model.names()
    chain = [n for n in names if ".query." not in n and ".key." not in n and "position_embeddings" not in n
             and "token_type" not in n]                      # read by the forward chain
    gemm = [n for n in chain if by_name[n].dim() == 2]       # read again by dX = dY W
    num = lambda ns: sum(by_name[n].numel() for n in ns)     # noqa: E731
    parts = {"weights_read_forward": 4 * num(chain), "weights_read_backward": 4 * num(gemm),
             "gradients_written": 4 * num(names),            # the q / k zeros and the embeddings' rows included
             "adam_read": 4 * 4 * num(names), "adam_written": 3 * 4 * num(names)}
    parts["total"] = sum(parts.values())
    return parts


def main_train(a, dev, data, model, B, N, sizes):
    step = TreeBERTTrainStep(model, drop_seed=1)
    rows = model._root_rows(data)
    st = timed_windows(lambda: step.step(data), a.warmup, a.iters, a.window)
    gb = timed_windows(lambda: model.grad_batch(rows, data.rootindex, data.y, drop_seed=1), a.warmup, a.iters, a.window)
    skipped = step.check_status()
    loss = float(step.step(data)[0])
    nbytes = train_bytes(model)
    floor_ms = nbytes["total"] / (HBM_PEAK_GBS * 1e9) * 1e3
    res = {"device": torch.cuda.get_device_name(0), "B": B, "N": N, "tokens_per_row": a.tokens,
           "longest_tree": int(sizes.max()), "hidden_dropout": model.hidden_dropout, "attn_dropout": model.attn_dropout,
           "train_step": st, "grad_batch_alone": gb, "steps_taken": step.step_count, "steps_skipped": skipped,
           "last_loss": loss, "bytes_per_step": nbytes, "hbm_peak_GBps": HBM_PEAK_GBS, "hbm_floor_ms": floor_ms,
           "step_GBps": nbytes["total"] / (st["median_ms"] * 1e-3) / 1e9,
           "step_time_over_hbm_floor": st["median_ms"] / floor_ms,
           "timing": "host clock around windows of steps ending in one device synchronise, after a warm-up"}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def main_train_gemms(a, dev, data, model, B, N, sizes):
    """``--train --gemm both``: the step and ``grad_batch`` on both GEMM paths, interleaved, on twin models."""
    legs = ("tiled", "skinny")
    twin = TreeBERT(256 * 768, 64, 64, dev, vocab=8).eval()
    twin.load_state_dict(model.state_dict())
    models = dict(zip(legs, (model, twin)))
    steps = {k: TreeBERTTrainStep(models[k], drop_seed=1, gemm=k) for k in legs}
    rows = model._root_rows(data)
    st = timed_windows_interleaved({k: (lambda k=k: steps[k].step(data)) for k in legs}, a.warmup, a.iters, a.window)
    gb = timed_windows_interleaved(
        {k: (lambda k=k: models[k].grad_batch(rows, data.rootindex, data.y, drop_seed=1, gemm=k)) for k in legs},
        a.warmup, a.iters, a.window)
    nbytes = train_bytes(model)
    res = {"device": torch.cuda.get_device_name(0), "B": B, "N": N, "tokens_per_row": a.tokens,
           "longest_tree": int(sizes.max()), "hidden_dropout": model.hidden_dropout, "attn_dropout": model.attn_dropout,
           "bytes_per_step": nbytes, "hbm_peak_GBps": HBM_PEAK_GBS,
           "hbm_floor_ms": nbytes["total"] / (HBM_PEAK_GBS * 1e9) * 1e3,
           "timing": "host clock around windows of steps ending in one device synchronise, after a warm-up; window k "
                     "of both legs before window k + 1 of either, one process, twin models, the same batch"}
    for k in legs:
        res[k] = {"train_step": dict(st[k], GBps=nbytes["total"] / (st[k]["median_ms"] * 1e-3) / 1e9),
                  "grad_batch_alone": gb[k], "steps_taken": steps[k].step_count, "steps_skipped": steps[k].check_status(),
                  "last_loss": float(steps[k].step(data)[0])}
    for what in ("train_step", "grad_batch_alone"):
        t, k = res["tiled"][what], res["skinny"][what]
        res[what + "_comparison"] = {"tiled_median_over_skinny_median": t["median_ms"] / k["median_ms"],
                                     "skinny_median_below_tiled_min": k["median_ms"] < t["min_ms"]}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def main_weights(a, dev, data, model, B, N, sizes):
    """``--weights bf16 / both``: ``evaluate`` on the fp32 parameters and on the bf16 weight images, in one
    process on the same batch; per leg the weight bytes one call reads and their share of the HBM peak."""
    by_name = dict(model.named_parameters())
    read = [n for n in model.names() if ".query." not in n and ".key." not in n
            and "position_embeddings" not in n and "token_type" not in n]
    imaged = {n for _, _, n in model._image_sources()}
    nbytes = {"fp32": 4 * sum(by_name[n].numel() for n in read),
              "bf16": sum((2 if n in imaged else 4) * by_name[n].numel() for n in read)}
    res = {"device": torch.cuda.get_device_name(0), "B": B, "N": N, "tokens_per_row": a.tokens,
           "longest_tree": int(sizes.max()), "hbm_peak_GBps": HBM_PEAK_GBS,
           "timing": "host clock around one evaluate() and a device synchronise, after a warm-up; both legs in one "
                     "process on the same batch"}
    logp = {}
    for leg in (("fp32", "bf16") if a.weights == "both" else (a.weights,)):
        model.use_weight_images(None if leg == "fp32" else "bf16")
        logp[leg] = torch.empty(B, 4, device=dev)
        t = timed(lambda: model.evaluate(data, logp=logp[leg]), a.warmup, a.iters)
        model.check_status()
        gbs = nbytes[leg] / (t["median_ms"] * 1e-3) / 1e9
        res["evaluate_" + leg] = dict(t, weight_bytes_per_call=nbytes[leg], GBps=gbs,
                                      fraction_of_hbm_peak=gbs / HBM_PEAK_GBS)
    if a.weights == "both":
        res["ratio_fp32_over_bf16"] = res["evaluate_fp32"]["median_ms"] / res["evaluate_bf16"]["median_ms"]
        res["max_abs_logp_diff_bf16_vs_fp32"] = float((logp["bf16"] - logp["fp32"]).abs().max())
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--weights", choices=("fp32", "bf16", "both"), default="fp32",
                    help="what evaluate() reads its GEMM weights from; bf16 / both time TreeBERT.use_weight_images "
                         "and write profiles/bert_eval_w16.json")
    ap.add_argument("--train", action="store_true", help="time the training step instead (profiles/bert_train.json)")
    ap.add_argument("--window", type=int, default=20, help="--train: steps per timed window")
    ap.add_argument("--gemm", choices=("tiled", "both"), default="tiled",
                    help="--train: both times gemm='tiled' and gemm='skinny' interleaved (profiles/bert_train_skinny.json)")
    ap.add_argument("--out", default=None, help="default profiles/bert_eval.json, or bert_train.json with --train")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--ref-iters", type=int, default=3)
    ap.add_argument("--tokens", type=int, default=4, help="T: values pooled per row are T x 768")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join("profiles", "bert_train_skinny.json" if a.train and a.gemm == "both" else
                             "bert_train.json" if a.train else
                             "bert_eval.json" if a.weights == "fp32" else "bert_eval_w16.json")
    if not torch.cuda.is_available():
        raise SystemExit("bert_bench needs a ROCm GPU (no fallback)")
    dev = torch.device("cuda:0")
    B, seed = 24, 1
    sizes = np.minimum(synth_tree_sizes(np.random.default_rng(seed), B, 64), 512)
    N = int(sizes.sum())
    g = torch.Generator().manual_seed(seed)
    data = SimpleNamespace(x=torch.randn(N, a.tokens * 768, generator=g).to(dev),
                           rootindex=torch.tensor(np.concatenate(([0], np.cumsum(sizes)[:-1])), dtype=torch.int64).to(dev),
                           y=torch.randint(0, 4, (B,), generator=g).to(dev))
    torch.manual_seed(seed)
    model = TreeBERT(256 * 768, 64, 64, dev, vocab=8).eval()
    if a.train:
        return (main_train_gemms if a.gemm == "both" else main_train)(a, dev, data, model, B, N, sizes)
    if a.weights != "fp32":
        return main_weights(a, dev, data, model, B, N, sizes)
    rows = model._pool(data.x.reshape(N, -1, 768))
    logp = torch.empty(B, 4, device=dev)

    ev = timed(lambda: model.evaluate(data, logp=logp), a.warmup, a.iters)
    full = timed(lambda: model.forward_batch(rows, data.rootindex, return_hidden=True, return_sums=True), a.warmup, a.iters)
    model.check_status()
    which, encode = reference(model)
    ref = timed(lambda: reference_loop(model, encode, data, rows), 1, a.ref_iters)
    want, _, _ = reference_loop(model, encode, data, rows)
    read = [n for n in model.names() if ".query." not in n and ".key." not in n
            and "position_embeddings" not in n and "token_type" not in n]
    by_name = dict(model.named_parameters())
    weight_bytes = 4 * sum(by_name[n].numel() for n in read)
    gbs = weight_bytes / (ev["median_ms"] * 1e-3) / 1e9
    res = {"device": torch.cuda.get_device_name(0), "B": B, "N": N, "tokens_per_row": a.tokens,
           "longest_tree": int(sizes.max()), "evaluate_root_only": ev, "full_form": full, "reference_loop": ref,
           "reference": which,
           "ratio_reference_over_evaluate": ref["median_ms"] / ev["median_ms"],
           "ratio_reference_over_full_form": ref["median_ms"] / full["median_ms"],
           "root_only_weight_bytes": weight_bytes, "root_only_GBps": gbs,
           "root_only_fraction_of_hbm_peak": gbs / HBM_PEAK_GBS, "hbm_peak_GBps": HBM_PEAK_GBS,
           "max_abs_logp_diff_vs_reference": float((logp - want).abs().max())}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
