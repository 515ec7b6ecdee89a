"""Time bigcn_amd.TweetEncoder.encode (bgcn_bert_encode) at BERT-base, T = 256 - the PHEME feature
extraction of one tree of n tweets - against the same computation in plain fp32 torch ops on the same GPU.

    python tools/bert_encode_bench.py [--seqs 1 8 24 64 --seq-len 256 --reps 10 --warmup 2 --blocks 2
                                       --out profiles/bert_encode_bench.json]

Forms, per n:
  native        encode(ids): the default call, the last layer on the [n, hidden] first rows only
  native_full   encode(ids, return_hidden=True): the last layer on every row (last_layer_full)
  unstaged      the default call with BGCN_BERT_ATTN_STAGE=0: every wave of the attention kernel reads its K / V
                tiles from global memory, nothing staged in LDS
  torch         embeddings, 12 layers and the pooler as torch.nn.functional ops in fp32 (what the reference's
                BertModel executes in eager mode; no attention mask), no host sync inside

Weights: BERT's initialisation times --weight-factor (default 3: attention away from uniform), random ids.
After --warmup calls of every form each call is bracketed by its own pair of device events; the forms
alternate in --blocks blocks.  Reported per form: median, 10th / 90th percentile, min and max of the per-call
times; the ratios of the medians; the model's FLOP count from the shapes and the rate it gives the native
call (a whole-call figure, not a kernel's share of peak); the largest difference between the native and the
torch results.  One JSON line goes to stdout (and, indented, to --out).  A run without a GPU fails.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

STAGE_KNOB = "BGCN_BERT_ATTN_STAGE"


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


def torch_encode(sd, ids, layers, heads):
    """(embeddings, pooler_output) as eager fp32 torch ops; every position attends to every other."""
    n, T = ids.shape
    e = "embeddings."
    emb = F.layer_norm(sd[e + "word_embeddings.weight"][ids] + sd[e + "token_type_embeddings.weight"][0]
                       + sd[e + "position_embeddings.weight"][:T], (sd[e + "LayerNorm.weight"].numel(),),
                       sd[e + "LayerNorm.weight"], sd[e + "LayerNorm.bias"], 1e-12)
    h, H = emb, emb.size(-1)

    def lin(v, name):
        return F.linear(v, sd[name + ".weight"], sd[name + ".bias"])

    def ln(v, name):
        return F.layer_norm(v, (H,), sd[name + ".weight"], sd[name + ".bias"], 1e-12)

    for i in range(layers):
        p = f"encoder.layer.{i}."
        q, k, v = (lin(h, p + "attention.self." + w).view(n, T, heads, 64).transpose(1, 2)
                   for w in ("query", "key", "value"))
        P = torch.softmax((q @ k.transpose(2, 3)) / 8.0, dim=-1)
        ctx = (P @ v).transpose(1, 2).reshape(n, T, H)
        a = ln(lin(ctx, p + "attention.output.dense") + h, p + "attention.output.LayerNorm")
        h = ln(lin(F.gelu(lin(a, p + "intermediate.dense")), p + "output.dense") + a, p + "output.LayerNorm")
    return emb, torch.tanh(lin(h[:, 0], "pooler.dense"))


def model_flops(n, T, H, I, L, heads):
    """Multiply-adds times two of the model as the reference runs it (every layer on every row)."""
    per_layer = 2 * n * T * (4 * H * H + 2 * H * I) + 2 * 2 * n * heads * T * T * 64
    return L * per_layer + 2 * n * H * H


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, nargs="+", default=[1, 8, 24, 64])
    ap.add_argument("--seq-len", type=int, default=256)
    ap.add_argument("--hidden", type=int, default=768)
    ap.add_argument("--intermediate", type=int, default=3072)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--vocab", type=int, default=30522)
    ap.add_argument("--weight-factor", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bert_encode_bench needs a ROCm GPU: nothing is measured without one")
    from bigcn_amd import TweetEncoder

    dev = torch.device("cuda:0")
    torch.manual_seed(a.seed)
    heads = a.hidden // 64
    m = TweetEncoder(hidden=a.hidden, heads=heads, intermediate=a.intermediate, num_layers=a.layers, max_pos=512,
                     vocab=a.vocab)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("LayerNorm.weight"):
                p.add_(0.1 * torch.randn_like(p))
            elif name.endswith(".bias"):
                p.normal_(0.0, 0.02)
            else:
                p.mul_(a.weight_factor)
    m = m.to(dev)
    sd = {k: v.detach() for k, v in m.state_dict().items()}
    os.environ.pop(STAGE_KNOB, None)
    res = {"what": "TweetEncoder.encode (bgcn_bert_encode), fp32", "device": torch.cuda.get_device_name(0),
           "hidden": a.hidden, "heads": heads, "intermediate": a.intermediate, "layers": a.layers, "seq_len": a.seq_len,
           "warmup_calls": a.warmup, "timer": "one pair of device events per call, forms alternating in blocks",
           "by_seqs": {}}
    for n in a.seqs:
        ids = torch.randint(0, a.vocab, (n, a.seq_len), device=dev)
        ids[:, a.seq_len * 2 // 3:] = 0   # the tokenizer's padding
        last = {}

        def native():
            last["native"] = m.encode(ids)

        def native_full():
            last["native_full"] = m.encode(ids, return_hidden=True)

        def unstaged():
            os.environ[STAGE_KNOB] = "0"
            try:
                last["unstaged"] = m.encode(ids)
            finally:
                os.environ.pop(STAGE_KNOB, None)

        def eager():
            with torch.no_grad():
                last["torch"] = torch_encode(sd, ids, a.layers, heads)

        forms = {"native": native, "native_full": native_full, "unstaged": unstaged, "torch": eager}
        for fn in forms.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        m.check_status()
        times = {k: [] for k in forms}
        for _ in range(a.blocks):
            for k, fn in forms.items():
                times[k] += timed(fn, max(1, a.reps // a.blocks))
        r = {k: stats(v) for k, v in times.items()}
        med = {k: r[k]["median_ms"] for k in forms}
        flops = model_flops(n, a.seq_len, a.hidden, a.intermediate, a.layers, heads)
        r.update(rows=n * a.seq_len, model_gflop=flops / 1e9,
                 native_tflops_of_model_work=flops / med["native"] / 1e9,
                 torch_over_native=med["torch"] / med["native"],
                 native_full_over_native=med["native_full"] / med["native"],
                 unstaged_over_native=med["unstaged"] / med["native"],
                 max_abs_diff_vs_torch={"embeddings": float((last["native"][0] - last["torch"][0]).abs().max()),
                                        "cls": float((last["native"][1] - last["torch"][1]).abs().max()),
                                        "cls_full": float((last["native_full"][1] - last["torch"][1]).abs().max())},
                 unstaged_equals_native=bool(torch.equal(last["native"][1], last["unstaged"][1])))
        res["by_seqs"][str(n)] = r
        last.clear()
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
