"""Diagnostic: where conv2's forward spends its time per block, alone and in the step, from a
-DBGCN_BLOCK_TRACE build of libbgcn (bgcn_trace.h; build line in tools/block_trace.py):

    BGCN_LIB=build/variants/libbgcn_bt.so python tools/conv2_blocks.py [--reps 4]

Per mode (chain alone: the prepared batch reused, nothing beside it; step: the next batch's
preparation - the pass over X - beside it) and per block that had work, pooled over --reps
recorded steps:
  start     the block's first wave start, relative to the launch's first wave on its XCD
            (per-XCD clock offsets are unknown) - dispatch queueing;
  fill      that start -> the B operand staged (mark 0, after the fill's barrier);
  rest      fill done -> the block's last wave end (products, root rounds, stores);
and the launch's span (first start -> last end, the longest XCD).  us of the device's
constant-rate clock (100 MHz).  Every recorded step is queued whole behind an ALU spin
(tools/libinterfere.so), as tools/trace_probe.py does."""
from __future__ import annotations

import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KID = 2   # conv2's forward (BT_END(2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="twitter15")
    ap.add_argument("--mhz", type=float, default=100.0)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--spin", type=int, default=60000)
    args = ap.parse_args()
    import bench
    from bigcn_amd import BiGCN, FusedTrainStep, Net, _lib
    from bigcn_amd.optim import bigcn_adam
    L = ctypes.CDLL(_lib.LIB_PATH)
    reader = L.bgcn_bt_read_sparse
    reader.restype = ctypes.c_int
    Li = ctypes.CDLL(os.path.join(ROOT, "tools", "libinterfere.so"))
    dev = torch.device("cuda", 0)
    wl = bench.WORKLOADS[args.workload]
    pool = bench.make_pool(wl, 0, 2, dev, (0.0, 0.0))
    model = (BiGCN if wl["classes"] == 4 else Net)(wl["feats"], 64, 64, dev).to(dev)
    model.train()
    fused = FusedTrainStep(model, bigcn_adam(model), tddroprate=wl["drop"][0], budroprate=wl["drop"][1], drop_seed=1)
    stream = torch.cuda.Stream(dev)
    sink = torch.zeros(4, device=dev)
    cap = 2 * 16 * (1 << 14)
    buf = np.zeros(cap * 4, dtype=np.uint64)
    us = 1.0 / args.mhz
    out = {"alone": [], "step": []}
    spans = {"alone": [], "step": []}
    with torch.cuda.stream(stream):
        for i in range(4):
            fused(pool[i % 2], next_data=pool[(i + 1) % 2])
        fused(pool[1], next_data=pool[0])
        pend = fused._pending
        for _ in range(3):
            fused._pending = pend
            fused(pool[0])
        torch.cuda.synchronize()
        for mode in ("alone", "step"):
            for _ in range(args.reps):
                reader(None, 0, 1)           # reset + enable
                fused._pending = pend
                Li.ifr_alu(1, args.spin, ctypes.c_void_p(sink.data_ptr()), ctypes.c_void_p(stream.cuda_stream))
                if mode == "step":
                    fused(pool[0], next_data=pool[1])
                    fused.discard_prefetch()
                else:
                    fused(pool[0])
                torch.cuda.synchronize()
                n = reader(buf.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong)), cap, 0)
                rec = buf[: 4 * n].reshape(-1, 4)
                mk = buf[4 * n: 8 * n].reshape(-1, 4)
                m = (rec[:, 1] != 0) & ((rec[:, 0] >> 48) == KID)
                rec, mk = rec[m], mk[m]
                blk = (rec[:, 0] & ((1 << 48) - 1)).astype(np.int64)        # (blockIdx.y, blockIdx.x)
                t0, t1 = rec[:, 1].astype(np.int64), rec[:, 2].astype(np.int64)
                xcc = ((rec[:, 3] >> 24) & 15).astype(int)
                fill = mk[:, 0].astype(np.int64)
                span = 0.0
                for x in sorted(set(xcc)):
                    mx = xcc == x
                    base = t0[mx].min()
                    span = max(span, (t1[mx].max() - base) * us)
                    for b in np.unique(blk[mx]):
                        mb = mx & (blk == b)
                        f = fill[mb]
                        f = f[f != 0]
                        if f.size == 0:
                            continue
                        s = t0[mb].min()
                        out[mode].append(((s - base) * us, (f.max() - s) * us, (t1[mb].max() - f.max()) * us))
                spans[mode].append(span)
    print(f"{args.workload}: conv2 forward per block, {args.reps} recorded steps per mode (us at {args.mhz:g} MHz)")
    for mode in ("alone", "step"):
        a = np.array(out[mode])
        print(f"{mode}: {len(a) // args.reps} blocks with work per launch; launch span (longest XCD) "
              + " ".join(f"{s:.1f}" for s in spans[mode]))
        for j, name in enumerate(("start", "fill", "rest")):
            v = a[:, j]
            print(f"  {name:6s} mean {v.mean():6.1f}  p10 {np.percentile(v, 10):6.1f}  p50 {np.percentile(v, 50):6.1f}  "
                  f"p90 {np.percentile(v, 90):6.1f}  max {v.max():6.1f}")
        life = a[:, 1] + a[:, 2]
        print(f"  block lifetime mean {life.mean():.1f} = fill {a[:, 1].mean():.1f} + rest {a[:, 2].mean():.1f}; "
              f"last block starts at {a[:, 0].max():.1f}")


if __name__ == "__main__":
    main()
