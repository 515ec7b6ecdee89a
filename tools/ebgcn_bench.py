"""Time the EBGCN edge-inference kernel (bgcn_edge_infer) on a twitter15-shaped batch against
the same arithmetic written with plain torch ops on the same GPU.

    python tools/ebgcn_bench.py [--trees 128 --mean 256 --edge-num 2 --iters 500 --out profiles/ebgcn_edge_infer.txt]

The batch: ``--trees`` random trees of LogNormal sizes (bench.py's twitter15 shape: 128 trees of
mean 256 nodes), E = N - trees edges, h [N, 64] random, fp32.  Both forms are warmed up, then
timed with device events over ``--iters`` calls, alternating blocks of the two; each timed
block ends in a synchronise and must finish within ``--limit`` seconds.

Reported: ms per call (median and min-max of the blocks), the kernel's share of the fp32 MFMA
peak = 524,288 E / t / 157.3e12 (the 64 x 64 x 64 product per edge is all it counts; the
epilogue's ~20k operations per edge are not), and max |kernel - torch| on the timed inputs.
The torch form materialises the [E, 64, 64] operand and its products (about 0.5 GB each).
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

FLOP_PER_EDGE = 2 * 64 * 64 * 64
MFMA_F32_PEAK = 157.3e12


def make_edges(rng, trees, mean):
    from bigcn_amd.data import synth_tree_sizes
    sizes = synth_tree_sizes(rng, trees, mean)
    rows, cols, off = [], [], 0
    for n in sizes:
        child = np.arange(1, n)
        rows.append(off + (rng.random(n - 1) * child).astype(np.int64))   # parent < child
        cols.append(off + child)
        off += int(n)
    return off, np.stack([np.concatenate(rows), np.concatenate(cols)])


def torch_form(h, ei, m):
    """edge_pred with library ops (the op sequence of the model's edge inference in eval mode)."""
    conv, norm, act, conv_out = m.sim_network
    D = (h[ei[0] - 1].unsqueeze(2) - h[ei[1] - 1].unsqueeze(1)).abs()          # [E, 64, 64]
    Y = torch.matmul(conv.weight[:, :, 0], D)
    Y = torch.nn.functional.batch_norm(Y, norm.running_mean, norm.running_var, norm.weight, norm.bias, False, 0.0,
                                       norm.eps)
    s = torch.matmul(conv_out.weight[0, :, 0], act(Y)) + conv_out.bias          # [E, 64]
    return torch.sigmoid(s @ m.fc1.weight.t()).mean(dim=1)


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
    ap.add_argument("--edge-num", type=int, default=2)
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--limit", type=float, default=60.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ebgcn_bench needs a ROCm GPU: nothing is measured without one")
    from bigcn_amd import edge_infer
    from bigcn_amd.ebgcn import TDrumorGCN

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(a.seed)
    N, ei = make_edges(rng, a.trees, a.mean)
    E = ei.shape[1]
    torch.manual_seed(a.seed)
    args = argparse.Namespace(input_features=64, hidden_features=64, output_features=64, edge_num=a.edge_num,
                              edge_infer_td=True, edge_infer_bu=True, device=dev)
    m = TDrumorGCN(args).eval()
    with torch.no_grad():   # away from the default init, where every output is ~0.5
        for mod in m.sim_network:
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.running_mean.normal_(0, 0.3)
                mod.running_var.uniform_(0.5, 2.0)
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.normal_(0, 0.3)
            elif isinstance(mod, torch.nn.Conv1d):
                mod.weight.mul_(3.0)
        m.fc1.weight.mul_(4.0)
    m = m.to(dev)
    h = (torch.randn(N, 64) * 0.7).to(dev)
    ei = torch.from_numpy(ei).to(dev)

    with torch.no_grad():
        k = lambda: edge_infer(h, ei, m)          # noqa: E731
        t = lambda: torch_form(h, ei, m)          # noqa: E731
        for _ in range(3):                        # warm-up: code objects, library algorithm choice
            pk, pt = k(), t()
        torch.cuda.synchronize()
        diff = float((pk - pt).abs().max())
        spread = (float(pt.min()), float(pt.max()))
        kt, tt = [], []
        for _ in range(a.blocks):                 # alternate the two forms
            kt.append(timed_block(k, a.iters, a.limit))
            tt.append(timed_block(t, max(1, a.iters // 10), a.limit))
    km, tm = statistics.median(kt), statistics.median(tt)
    lines = [
        f"edge_infer, fp32, twitter15-shaped batch: trees={a.trees} N={N} E={E} edge_num={a.edge_num} "
        f"device={torch.cuda.get_device_name(0)}",
        f"  timing: device events, {a.blocks} alternating blocks, kernel {a.iters} calls/block, torch "
        f"{max(1, a.iters // 10)} calls/block, 3 warm-up calls each",
        f"  HIP kernel (ops.edge_infer, incl. the BatchNorm fold launch): {km:.4f} ms/call "
        f"(min {min(kt):.4f}, max {max(kt):.4f})",
        f"    fraction of fp32 MFMA peak (524,288 E / t / 157.3e12): {FLOP_PER_EDGE * E / (km * 1e-3) / MFMA_F32_PEAK:.3f}",
        f"  plain torch ops, same arithmetic: {tm:.4f} ms/call (min {min(tt):.4f}, max {max(tt):.4f})",
        f"  torch / kernel: {tm / km:.1f}x",
        f"  max |kernel - torch| = {diff:.3e} on outputs in [{spread[0]:.3f}, {spread[1]:.3f}]",
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    if not km < tm:
        raise SystemExit("the kernel is not faster than the torch form")


if __name__ == "__main__":
    main()
