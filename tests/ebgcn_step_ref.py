"""The reference trajectory of EBGCN's training loop body (model/Twitter/EBGCN.py:249-260, :300-312) on the
model fixture, in this project's own words.  TEST INFRASTRUCTURE: tests/ebgcn_train_ref.py's forward in a
given dtype, the reference's loss composition, autograd, and torch.optim.Adam over the reference's five
parameter groups.  tests/test_ebgcn_step_ref.py bounds its fp32-vs-fp64 distance on the CPU;
tests/test_gpu_ebgcn_step.py compares EBGCNTrainStep with its fp64 run.
"""
import argparse
import os

import torch
import torch.nn.functional as F

import ebgcn_train_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_FIXTURE = os.path.join(ROOT, "tests", "golden", "train_ebgcn_model.npz")
# the issue's settings: lr 5e-4, lr scales 5 (BU) and 1 (TD), l2 1e-4, edge-loss weights 0.2
LR, LR_SCALE_BU, LR_SCALE_TD, L2, EDGE_LOSS_TD, EDGE_LOSS_BU = 5e-4, 5, 1, 1e-4, 0.2, 0.2
# The noise of the Bayesian branch.  With the fixture's own draw the fp64 trajectory puts one LeakyReLU
# argument of TDrumorGCN.sim_network at 1.2e-9 of the largest one in its third step: below fp32's resolution,
# so which slope that element's gradient takes is a coin toss in ANY fp32 evaluation, and the toss moves d
# TDrumorGCN.conv1.* by ~1.5e-4 of its maximum.  NOISE_SEED is the first seed (from 1 up) whose fp64
# trajectory keeps every sign decision that a gradient passes through (sign_margins) at least TIE_WINDOW away
# from zero in all three steps and whose fp32 run stays inside the bars (tests/test_ebgcn_step_ref.py).
NOISE_SEED = 1
TIE_WINDOW = 2.0 ** -23   # fp32's epsilon, relative to the largest argument of the same activation


def args_of(z, td=True, bu=True, device="cpu"):
    return argparse.Namespace(input_features=int(z["x"].shape[1]), hidden_features=64, output_features=64,
                              num_class=int(z["logp"].shape[1]), edge_num=int(z["edge_num"]), edge_infer_td=td,
                              edge_infer_bu=bu, device=device, lr=LR, lr_scale_bu=LR_SCALE_BU,
                              lr_scale_td=LR_SCALE_TD, l2=L2, edge_loss_td=EDGE_LOSS_TD, edge_loss_bu=EDGE_LOSS_BU)


def noise_of(z, seed=NOISE_SEED):
    """The pair (td, bu) of standard-normal draws [E, 64]; ``seed=None``: the fixture's own."""
    if seed is None:
        return z["noise_td"], z["noise_bu"]
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(z[k].shape, generator=g) for k in ("noise_td", "noise_bu"))


def sign_margins(z, sd, td=True, bu=True):
    """For a state ``sd`` (fp64): the smallest |argument| / max |argument| of every activation whose
    derivative is a sign decision on the gradient's way - per direction sim_network's LeakyReLU, the
    |a - b| of the edge features (rows that are not the same node), bn1's relu (conv1's columns) and
    conv2's relu."""
    from oracle import bigcn_oracle as O
    out = {}
    x = z["x"].to(torch.float64)
    for d, key, on in (("TDrumorGCN", "edge_index", td), ("BUrumorGCN", "BU_edge_index", bu)):
        ei = z[key]
        h1 = O.gcn_conv(x, ei, sd[d + ".conv1.lin.weight"], sd[d + ".conv1.bias"])
        N = h1.size(0)
        pred = None
        if on:
            a, b = (ei[0] - 1) % N, (ei[1] - 1) % N
            D = (h1[a][:, :, None] - h1[b][:, None, :])[a != b].abs()
            out[d + " |a - b|"] = float(D.min() / D.max())
            det = {}
            _, pred = T.edge_infer_train(sd, d, h1, ei, torch.zeros(ei.size(1), 64, dtype=torch.float64), {}, det)
            A = det["pre_activation"].abs()
            out[d + " LeakyReLU"] = float(A.min() / A.max())
        cat = T.bn_train(torch.cat((h1, x[z["rootindex"][z["batch"]]]), 1), sd, d + ".bn1", {})
        out[d + " bn1 relu"] = float(cat[:, :64].abs().min() / cat.abs().max())
        h2 = O.gcn_conv(F.relu(cat), ei, sd[d + ".conv2.lin.weight"], sd[d + ".conv2.bias"], edge_weight=pred)
        out[d + " conv2 relu"] = float(h2.abs().min() / h2.abs().max())
    return out


def _groups(sd):
    def conv(d, c):
        return [sd[f"{d}.{c}.lin.weight"], sd[f"{d}.{c}.bias"]]
    named = [conv("BUrumorGCN", "conv1"), conv("BUrumorGCN", "conv2"), conv("TDrumorGCN", "conv1"),
             conv("TDrumorGCN", "conv2")]
    taken = {id(p) for g in named for p in g}
    base = [v for v in sd.values() if v.requires_grad and id(v) not in taken]
    return [{"params": base},
            {"params": named[0], "lr": LR / LR_SCALE_BU}, {"params": named[1], "lr": LR / LR_SCALE_BU},
            {"params": named[2], "lr": LR / LR_SCALE_TD}, {"params": named[3], "lr": LR / LR_SCALE_TD}]


def trajectory(z, dtype, steps=3, td=True, bu=True, seed=NOISE_SEED, margins=False):
    """``[{"loss", "grads": {key: grad or None}, "params": {key: value after the update}}]`` per step, and the
    keys of the parameters that never get a gradient.  ``margins``: each step also carries ``sign_margins`` of
    the state its forward ran on."""
    sd = T.with_grad(T.group(z, "sd"), dtype)
    keys = [k for k, v in sd.items() if v.requires_grad]
    opt = torch.optim.Adam(_groups(sd), lr=LR, weight_decay=L2)
    x = z["x"].to(dtype)
    ntd, nbu = noise_of(z, seed)
    noise = (ntd.to(dtype) if td else None, nbu.to(dtype) if bu else None)
    out = []
    for _ in range(steps):
        new = {}
        marg = sign_margins(z, {k: v.detach() for k, v in sd.items()}, td, bu) if margins else None
        logp, ltd, lbu = T.forward_train(sd, x, z["edge_index"], z["BU_edge_index"], z["batch"], z["rootindex"],
                                         noise, infer_td=td, infer_bu=bu, new_buffers=new)
        loss = F.nll_loss(logp, z["y"])
        if ltd is not None:
            loss = loss + EDGE_LOSS_TD * ltd
        if lbu is not None:
            loss = loss + EDGE_LOSS_BU * lbu
        opt.zero_grad()
        loss.backward()
        grads = {k: (None if sd[k].grad is None else sd[k].grad.detach().clone()) for k in keys}
        opt.step()
        for k, v in new.items():   # the BatchNorms' buffers move on as the module's do
            sd[k] = v.detach().clone()
        pred = logp.detach().argmax(dim=1)
        out.append({"loss": loss.detach().clone(), "grads": grads, "margins": marg, "correct": int((pred == z["y"]).sum()),
                    "params": {k: sd[k].detach().clone() for k in keys}})
    return out, sorted(k for k in keys if all(s["grads"][k] is None for s in out))
