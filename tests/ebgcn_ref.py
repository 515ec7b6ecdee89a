"""Plain-torch restatement of EBGCN's eval-mode forward (model/Twitter/EBGCN.py:61-116, :215-230),
in this project's own words.  TEST INFRASTRUCTURE: the fp64 oracle of tests/test_gpu_ebgcn.py;
tests/test_ebgcn.py pins it (in fp32) to fixtures the reference's own classes produced
(tools/gen_ebgcn_golden.py).

Everything is a function of a state_dict keyed like the reference's and runs in the dtype of
its tensors.  The Bayesian branch of edge_infer (W_mean .. B_bias, fc2, th.normal) only feeds the
edge loss, which the evaluation loop discards, and is not restated.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import bigcn_oracle as O

BN_EPS = 1e-5          # torch.nn.BatchNorm1d's default, which the reference keeps
LEAKY_SLOPE = 0.01     # torch.nn.LeakyReLU's default


def bn_eval(v, sd, prefix, channel_dim=1):
    """Eval-mode BatchNorm1d over dimension ``channel_dim`` of ``v``."""
    shape = [1] * v.dim()
    shape[channel_dim] = -1
    mean, var = sd[prefix + ".running_mean"].view(shape), sd[prefix + ".running_var"].view(shape)
    w, b = sd[prefix + ".weight"].view(shape), sd[prefix + ".bias"].view(shape)
    return (v - mean) / torch.sqrt(var + BN_EPS) * w + b


def edge_pred(sd, d, h, edge_index):
    """``edge_pred`` [E] of direction ``d`` ('TDrumorGCN' / 'BUrumorGCN') from conv1's output
    ``h`` [N, 64] (EBGCN.py:95-102, :116).  Edge (r, c) reads the rows r - 1 and c - 1; index -1
    is the last node (the reference's indexing as written)."""
    N = h.size(0)
    a = h[(edge_index[0] - 1) % N]                       # [E, 64]  (c)
    b = h[(edge_index[1] - 1) % N]                       # [E, 64]  (l)
    D = (a[:, :, None] - b[:, None, :]).abs()            # [E, c, l]
    net = d + ".sim_network.sim_val"
    Y = torch.einsum("oc,ecl->eol", sd[net + "conv0.weight"][:, :, 0], D)
    Z = F.leaky_relu(bn_eval(Y, sd, net + "norm0"), LEAKY_SLOPE)
    s = torch.einsum("o,eol->el", sd[net + "conv_out.weight"][0, :, 0], Z) + sd[net + "conv_out.bias"]
    p = torch.sigmoid(s @ sd[d + ".fc1.weight"].t())     # [E, K]
    return p.mean(dim=1)


def direction(sd, d, x, edge_index, batch, rootindex, infer):
    """One direction's [B, 128] readout and its edge_pred (None when ``infer`` is off)."""
    h1 = O.gcn_conv(x, edge_index, sd[d + ".conv1.lin.weight"], sd[d + ".conv1.bias"])
    pred = edge_pred(sd, d, h1, edge_index) if infer else None
    root_of_node = rootindex[batch]
    cat = torch.cat((h1, x[root_of_node]), 1)
    if cat.size(0) != 1:                                  # EBGCN.py:80
        cat = bn_eval(cat, sd, d + ".bn1")
    cat = F.relu(cat)
    h2 = F.relu(O.gcn_conv(cat, edge_index, sd[d + ".conv2.lin.weight"], sd[d + ".conv2.bias"], edge_weight=pred))
    out = O.scatter_mean(torch.cat((h2, h1[root_of_node]), 1), batch, dim=0)
    return out, pred


def forward(sd, x, edge_index, bu_edge_index, batch, rootindex, infer_td=True, infer_bu=True):
    """(log_probs [B, C], td_edge_pred, bu_edge_pred)."""
    td, td_pred = direction(sd, "TDrumorGCN", x, edge_index, batch, rootindex, infer_td)
    bu, bu_pred = direction(sd, "BUrumorGCN", x, bu_edge_index, batch, rootindex, infer_bu)
    z = F.linear(torch.cat((bu, td), 1), sd["fc.weight"], sd["fc.bias"])
    return F.log_softmax(z, dim=1), td_pred, bu_pred


# ---- fixtures (tests/golden/ebgcn_*.npz)
def load_fixture(path, dtype=torch.float32):
    """(state_dict in ``dtype`` with integer buffers kept, batch dict, settings dict, expected dict)."""
    z = np.load(path)
    sd = {}
    for k in z.files:
        if k.startswith("sd/"):
            t = torch.from_numpy(z[k])
            sd[k[3:]] = t.to(dtype) if t.is_floating_point() else t
    b = {"x": torch.from_numpy(z["x"]).to(dtype)}
    for k in ("edge_index", "BU_edge_index", "batch", "rootindex"):
        b[k] = torch.from_numpy(z[k])
    cfg = {k: int(z[k]) for k in ("edge_num", "num_class", "edge_infer_td", "edge_infer_bu")}
    exp = {k: torch.from_numpy(z[k]) for k in ("logp", "td_edge_pred", "bu_edge_pred")}
    return sd, b, cfg, exp


def fixture_forward(sd, b, cfg):
    return forward(sd, b["x"], b["edge_index"], b["BU_edge_index"], b["batch"], b["rootindex"],
                   bool(cfg["edge_infer_td"]), bool(cfg["edge_infer_bu"]))
