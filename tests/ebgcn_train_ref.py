"""Plain-torch restatement of EBGCN's TRAINING forward (model/Twitter/EBGCN.py:61-116, :215-230), in
this project's own words.  TEST INFRASTRUCTURE: the fp64 oracle of tests/test_gpu_ebgcn_train.py;
tests/test_ebgcn_train.py pins it (in fp32) to fixtures the reference's own classes produced
(tools/gen_ebgcn_train_golden.py).

Everything is a function of a state_dict keyed like the reference's and runs in the dtype of its
tensors, with torch's autograd for the gradients: pass tensors that require grad and differentiate
the results.  The reference's ``th.normal(mean, std)`` is ``mean + std * noise`` for a given
standard-normal ``noise`` and carries no gradient.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import bigcn_oracle as O

BN_EPS = 1e-5          # torch.nn.BatchNorm1d's defaults, which the reference keeps
BN_MOMENTUM = 0.1
LEAKY_SLOPE = 0.01     # torch.nn.LeakyReLU's default
NETWORKS = (("sim_network", "sim_val"), ("W_mean", "W_mean"), ("W_bias", "W_bias"), ("B_mean", "B_mean"),
            ("B_bias", "B_bias"))


def bn_train(v, sd, prefix, new_buffers, channel_dim=1):
    """Training-mode BatchNorm1d over dimension ``channel_dim``: batch statistics (biased variance)
    normalise; the running statistics blended with the batch's (unbiased variance) and the
    incremented counter go into ``new_buffers``."""
    dims = [d for d in range(v.dim()) if d != channel_dim]
    shape = [1] * v.dim()
    shape[channel_dim] = -1
    n = v.numel() // v.size(channel_dim)
    mean = v.mean(dim=dims)
    var = ((v - mean.view(shape)) ** 2).mean(dim=dims)
    with torch.no_grad():
        m = BN_MOMENTUM
        new_buffers[prefix + ".running_mean"] = (1 - m) * sd[prefix + ".running_mean"] + m * mean
        new_buffers[prefix + ".running_var"] = (1 - m) * sd[prefix + ".running_var"] + m * var * n / max(n - 1, 1)
        new_buffers[prefix + ".num_batches_tracked"] = sd[prefix + ".num_batches_tracked"] + 1
    return (v - mean.view(shape)) / torch.sqrt(var.view(shape) + BN_EPS) * sd[prefix + ".weight"].view(shape) \
        + sd[prefix + ".bias"].view(shape)


def edge_infer_train(sd, d, h, edge_index, noise, new_buffers=None, details=None):
    """``(edge_loss, edge_pred [E])`` of direction ``d`` in training mode from conv1's output ``h``
    [N, 64] (EBGCN.py:95-116).  ``new_buffers`` (a dict) receives the five norms' updated buffers,
    ``details`` (a dict) the intermediate values the fixtures' conditions are stated on."""
    new_buffers = {} if new_buffers is None else new_buffers
    N = h.size(0)
    a = h[(edge_index[0] - 1) % N]                       # [E, 64]  (c)
    b = h[(edge_index[1] - 1) % N]                       # [E, 64]  (l)
    D = (a[:, :, None] - b[:, None, :]).abs()            # [E, c, l]
    out = {}
    for net, name in NETWORKS:
        pre = d + "." + net + "." + name
        Y = torch.einsum("oc,ecl->eol", sd[pre + "conv0.weight"][:, :, 0], D)
        A = bn_train(Y, sd, pre + "norm0", new_buffers)
        Z = F.leaky_relu(A, LEAKY_SLOPE)
        out[net] = torch.einsum("o,eol->el", sd[pre + "conv_out.weight"][0, :, 0], Z) + sd[pre + "conv_out.bias"]
        if details is not None and net == "sim_network":
            details["pre_activation"] = A.detach()
    s = out["sim_network"]
    p = torch.sigmoid(s @ sd[d + ".fc1.weight"].t())     # [E, K]
    with torch.no_grad():                                 # th.normal has no gradient
        mean = out["W_mean"] * s + out["B_mean"]
        std = torch.relu(torch.log(s ** 2 * torch.exp(out["W_bias"]) + torch.exp(out["B_bias"])))
        y = torch.sigmoid(mean + std * noise)
        p_y = F.softmax(y @ sd[d + ".fc2.weight"].t(), dim=-1)
    logp_x = F.log_softmax(p, dim=-1)
    loss = (torch.xlogy(p_y, p_y) - p_y * logp_x).sum() / p.size(0)     # KLDivLoss(reduction='batchmean')
    if details is not None:
        details.update(std=std, p_y=p_y, softmax_p=F.softmax(p.detach(), dim=-1))
    return loss, p.mean(dim=1)


def direction_train(sd, d, x, edge_index, batch, rootindex, infer, noise, new_buffers):
    """One direction's ``([B, 128] readout, edge_loss or None)`` in training mode (EBGCN.py:61-93)."""
    h1 = O.gcn_conv(x, edge_index, sd[d + ".conv1.lin.weight"], sd[d + ".conv1.bias"])
    loss = pred = None
    if infer:
        loss, pred = edge_infer_train(sd, d, h1, edge_index, noise, new_buffers)
    root_of_node = rootindex[batch]
    cat = torch.cat((h1, x[root_of_node]), 1)
    if cat.size(0) != 1:                                  # EBGCN.py:80
        cat = bn_train(cat, sd, d + ".bn1", new_buffers)
    cat = F.relu(cat)
    h2 = F.relu(O.gcn_conv(cat, edge_index, sd[d + ".conv2.lin.weight"], sd[d + ".conv2.bias"], edge_weight=pred))
    # the reference's x2 = copy.copy(x) (EBGCN.py:65) is a copy outside the autograd graph: no
    # gradient reaches conv1 through the root rows of the readout
    return O.scatter_mean(torch.cat((h2, h1.detach()[root_of_node]), 1), batch, dim=0), loss


def forward_train(sd, x, edge_index, bu_edge_index, batch, rootindex, noise, infer_td=True, infer_bu=True,
                  new_buffers=None):
    """``(log_probs [B, C], TD_edge_loss, BU_edge_loss)``; ``noise`` is the pair (td, bu)."""
    new_buffers = {} if new_buffers is None else new_buffers
    td, td_loss = direction_train(sd, "TDrumorGCN", x, edge_index, batch, rootindex, infer_td, noise[0], new_buffers)
    bu, bu_loss = direction_train(sd, "BUrumorGCN", x, bu_edge_index, batch, rootindex, infer_bu, noise[1], new_buffers)
    z = F.linear(torch.cat((bu, td), 1), sd["fc.weight"], sd["fc.bias"])
    return F.log_softmax(z, dim=1), td_loss, bu_loss


def with_grad(sd, dtype):
    """A copy of ``sd`` in ``dtype`` whose floating-point parameters (not the buffers) require grad."""
    out = {}
    for k, v in sd.items():
        if not v.is_floating_point():
            out[k] = v.clone()
        elif k.endswith("running_mean") or k.endswith("running_var"):
            out[k] = v.to(dtype).clone()
        else:
            out[k] = v.to(dtype).clone().requires_grad_(True)
    return out


def grads_of(value, sd, extra=()):
    """``({key: grad} for the parameters of ``sd`` that ``value`` depends on, the sorted keys of those it
    does not, [grads of ``extra``])``."""
    keys = [k for k, v in sd.items() if v.requires_grad]
    gs = torch.autograd.grad(value, [sd[k] for k in keys] + list(extra), allow_unused=True)
    have = {k: g for k, g in zip(keys, gs) if g is not None}
    return have, sorted(k for k, g in zip(keys, gs) if g is None), list(gs[len(keys):])


def load_npz(path):
    z = np.load(path)
    return {k: (list(z[k]) if z[k].dtype.kind == "U" else torch.from_numpy(np.asarray(z[k]))) for k in z.files}


def group(z, prefix):
    """The entries of a fixture whose key starts with ``prefix + '/'``, by the rest of the key."""
    return {k[len(prefix) + 1:]: v for k, v in z.items() if k.startswith(prefix + "/")}
