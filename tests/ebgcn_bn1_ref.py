"""Plain-torch restatement of EBGCN's training-mode bn1 + relu + conv2 lin (model/Twitter/EBGCN.py:72-84)
WITHOUT the dense concat, in any dtype.  TEST INFRASTRUCTURE: it documents the formulas of
``bgcn_ebgcn_conv2_lin_train_fwd`` / ``_bwd``; tests/test_ebgcn_bn1_train.py pins it in fp64 to the dense
composition (``ebgcn_train_ref.bn_train`` over the materialised concat, relu, ``F.linear``, autograd), which
is the oracle of tests/test_gpu_ebgcn_bn1_train.py.

The concat row of node i is c_i = [h1_i | x[rootindex[batch_i]]]: the F root columns hold only B distinct
rows, so their statistics, product and gradients are taken over the B root rows weighted by tree size n_b.
"""
import functools

import torch
import torch.nn.functional as F

import ebgcn_train_ref as T

H = 64
# (N, B, F) of the kernel tests: the smallest batch that uses bn1; one tree of a single node; a batch that
# crosses a 256-row reduction block; more trees than one block of the root-table reductions takes (32) and
# F no multiple of 64; one tree id without nodes and one rootindex that points into another tree
SHAPES = [(2, 1, 4), (5, 3, 4), (257, 3, 68), (1031, 130, 300), (64, 4, 8)]
MARGIN = 1e-3    # no pre-activation of a case lies within MARGIN * max|y| of relu's kink


# ----------------------------------------------------------------------------- the factored form
def forward(h1, x, batch, rootindex, W2, gamma, beta, eps=T.BN_EPS):
    """``(z2 [N, 64], saved)``: batch statistics, the fold, the folded forward."""
    N, B = h1.size(0), rootindex.numel()
    n = torch.bincount(batch, minlength=B).to(h1.dtype)                 # tree sizes; sum = N
    xr = x[rootindex.clamp(0, N - 1)]                                   # [B, F] (an empty tree has weight 0)
    mean_h = h1.mean(0)
    var_h = ((h1 - mean_h) ** 2).mean(0)
    mean_x = (n[:, None] * xr).sum(0) / N
    var_x = (n[:, None] * (xr - mean_x) ** 2).sum(0) / N
    mean, var = torch.cat((mean_h, mean_x)), torch.cat((var_h, var_x))  # biased variance
    g = gamma / torch.sqrt(var + eps)
    t = beta - mean * g
    y_h, y_x = g[:H] * h1 + t[:H], g[H:] * xr + t[H:]
    a_h, a_x = torch.relu(y_h), torch.relu(y_x)
    r = a_x @ W2[:, H:].t()                                             # [B, 64]: once per tree
    z2 = a_h @ W2[:, :H].t() + r[batch]
    saved = dict(h1=h1, xr=xr, batch=batch, n=n, W2=W2, mean=mean, var=var, g=g, eps=eps, y_h=y_h, y_x=y_x,
                 a_h=a_h, a_x=a_x)
    return z2, saved


def backward(saved, dz2):
    """``(dh1, dW2, dgamma, dbeta)`` in closed form."""
    s = saved
    N, B = s["h1"].size(0), s["n"].numel()
    rstd = 1.0 / torch.sqrt(s["var"] + s["eps"])
    dR = torch.zeros(B, H, dtype=dz2.dtype).index_add_(0, s["batch"], dz2)          # per-tree segment sum
    dW2 = torch.cat((dz2.t() @ s["a_h"], dR.t() @ s["a_x"]), 1)                      # x block: B rows, not N
    dY_h = (dz2 @ s["W2"][:, :H]) * (s["y_h"] > 0)
    dY_x = (dR @ s["W2"][:, H:]) * (s["y_x"] > 0)                                    # already summed over the tree
    ch_h = (s["h1"] - s["mean"][:H]) * rstd[:H]
    ch_x = (s["xr"] - s["mean"][H:]) * rstd[H:]
    dbeta = torch.cat((dY_h.sum(0), dY_x.sum(0)))
    dgamma = torch.cat(((dY_h * ch_h).sum(0), (dY_x * ch_x).sum(0)))                 # no n_b weight on the x side
    dh1 = s["g"][:H] * (dY_h - dbeta[:H] / N - ch_h * dgamma[:H] / N)
    return dh1, dW2, dgamma, dbeta


def blend(saved, running_mean, running_var, num_batches_tracked, momentum=T.BN_MOMENTUM):
    """The running buffers after the batch, as torch.nn.BatchNorm1d: momentum (``None``: the cumulative
    average), the unbiased variance, the counter + 1."""
    N = saved["h1"].size(0)
    nbt = num_batches_tracked + 1
    m = 1.0 / float(nbt) if momentum is None else momentum
    return ((1 - m) * running_mean + m * saved["mean"], (1 - m) * running_var + m * saved["var"] * N / max(N - 1, 1),
            nbt)


class Factored(torch.autograd.Function):
    """The factored block inside an autograd graph (x, batch and rootindex are data)."""

    @staticmethod
    def forward(ctx, h1, W2, gamma, beta, x, batch, rootindex, out):
        z2, ctx.s = forward(h1.detach(), x, batch, rootindex, W2.detach(), gamma.detach(), beta.detach())
        out.update(ctx.s)
        return z2

    @staticmethod
    def backward(ctx, dz2):
        return backward(ctx.s, dz2) + (None, None, None, None)


# ----------------------------------------------------------------------------- the dense oracle
def dense(h1, x, batch, rootindex, W2, gamma, beta, running_mean, running_var, num_batches_tracked):
    """``(z2, y [N, 64 + F] pre-activations, new buffers)`` of the materialised concat, differentiable."""
    sd = {"bn1.weight": gamma, "bn1.bias": beta, "bn1.running_mean": running_mean, "bn1.running_var": running_var,
          "bn1.num_batches_tracked": num_batches_tracked}
    new = {}
    y = T.bn_train(torch.cat((h1, x[rootindex[batch]]), 1), sd, "bn1", new)
    return F.linear(torch.relu(y), W2), y, new


def dense_reference(case, momentum=T.BN_MOMENTUM):
    """fp64 results of a case: z2, the gradients for the case's upstream weights, the new buffers, y."""
    c = {k: (v.double() if v.is_floating_point() else v) for k, v in case.items()}
    leaves = [c[k].clone().requires_grad_(True) for k in ("h1", "W2", "gamma", "beta")]
    z2, y, new = dense(leaves[0], c["x"], c["batch"], c["rootindex"], leaves[1], leaves[2], leaves[3],
                       c["running_mean"], c["running_var"], c["num_batches_tracked"])
    dh1, dW2, dgamma, dbeta = torch.autograd.grad((c["up"] * z2).sum(), leaves)
    rm, rv, nbt = new["bn1.running_mean"], new["bn1.running_var"], new["bn1.num_batches_tracked"]
    if momentum is None:   # the cumulative average: bn_train blends with the default momentum
        N = c["h1"].size(0)
        cat = torch.cat((c["h1"], c["x"][c["rootindex"][c["batch"]]]), 1)
        mean = cat.mean(0)
        var = ((cat - mean) ** 2).mean(0)
        m = 1.0 / float(nbt)
        rm = (1 - m) * c["running_mean"] + m * mean
        rv = (1 - m) * c["running_var"] + m * var * N / max(N - 1, 1)
    return dict(z2=z2.detach(), dh1=dh1, dW2=dW2, dgamma=dgamma, dbeta=dbeta, running_mean=rm, running_var=rv,
                num_batches_tracked=nbt, y=y.detach())


# ----------------------------------------------------------------------------- cases
def tree_sizes(N, B, g):
    """Unequal tree sizes that sum to N.  (5, 3, .): one tree of a single node; (64, 4, .): tree 1 is empty."""
    if (N, B) == (5, 3):
        return [2, 1, 2]
    if (N, B) == (64, 4):
        return [30, 0, 20, 14]
    cuts = torch.randperm(N - 1, generator=g)[:B - 1].sort().values + 1
    edges = [0] + cuts.tolist() + [N]
    return [edges[k + 1] - edges[k] for k in range(B)]


def _offenders(case):
    c = {k: (v.double() if v.is_floating_point() else v) for k, v in case.items()}
    with torch.no_grad():
        _, y, _ = dense(c["h1"], c["x"], c["batch"], c["rootindex"], c["W2"], c["gamma"], c["beta"],
                        c["running_mean"], c["running_var"], c["num_batches_tracked"])
    return y, float(y.abs().max())


@functools.lru_cache(maxsize=None)
def make_case(N, B, F_in, seed=0):
    """One seeded case, fp32 on the CPU: h1, x (TF-IDF-like: ~90 % exact zeros, column 1 zero in every row, so
    var = 0 there), a sorted batch vector, rootindex, W2, bn1's parameters and buffers drawn by the recipe of
    test_gpu_ebgcn_train._randomised, and ``up`` [N, 64], the upstream gradient's weights.

    relu's mask jumps at y = 0 and an fp32 kernel may land on the other side of a pre-activation that is 0 to
    rounding.  The margin the tests assert (no |y| < MARGIN max|y| in the fp64 restatement) is made, not hoped
    for: a batch of this size always draws some y that close, so the offending entries are moved out - an h1
    entry or a nonzero root feature is shifted, and where a column's zero entries share an offending y = t_c,
    that column's bias is.  The loop ends when a pass finds none at 1.5 MARGIN."""
    g = torch.Generator().manual_seed(7919 * seed + 1000 * N + 10 * B + F_in)
    sizes = tree_sizes(N, B, g)
    batch = torch.repeat_interleave(torch.arange(B), torch.tensor(sizes))
    first = torch.cumsum(torch.tensor([0] + sizes[:-1]), 0)
    rootindex = first.clone()                                   # each tree's first node ...
    if (N, B) == (64, 4):
        rootindex[1] = 0                                        # the empty tree's entry is never used
        rootindex[2] = 3                                        # ... but tree 2's root lies in tree 0
    h1 = torch.randn(N, H, generator=g) * 0.7
    x = torch.rand(N, F_in, generator=g) * (torch.rand(N, F_in, generator=g) < 0.1)
    x[:, 1] = 0.0
    C = H + F_in
    case = dict(
        h1=h1, x=x, batch=batch, rootindex=rootindex,
        W2=(torch.rand(H, C, generator=g) * 2 - 1) * (6.0 / (H + C)) ** 0.5,     # glorot, GCNConv's lin
        running_mean=torch.randn(C, generator=g) * 0.3, running_var=torch.rand(C, generator=g) * 1.5 + 0.5,
        gamma=torch.rand(C, generator=g) + 0.5, beta=torch.randn(C, generator=g) * 0.3,
        num_batches_tracked=torch.tensor(seed + 3), up=torch.randn(N, H, generator=g))
    root_of_node = rootindex[batch]
    for _ in range(50):
        y, top = _offenders(case)
        thr = 1.5 * MARGIN * top
        bad = (y.abs() < thr).nonzero()
        if not len(bad):
            break
        var = torch.cat((h1, x[root_of_node]), 1).double().var(0, unbiased=False)
        gfold = case["gamma"].double() / torch.sqrt(var + T.BN_EPS)
        moved = set()
        for i, c in bad.tolist():
            step = float(3 * thr / gfold[c]) if y[i, c] >= 0 else -float(3 * thr / gfold[c])
            r = int(root_of_node[i])
            if c < H:
                h1[i, c] += step
            elif x[r, c - H] != 0:
                if (r, c) not in moved:          # one root row serves every node of its tree
                    x[r, c - H] += abs(step)
                moved.add((r, c))
            elif c not in moved:
                # every zero entry of the column moves with its bias; the next pass looks again
                case["beta"][c] += 3 * thr if y[i, c] >= 0 else -3 * thr
                moved.add(c)
    else:
        raise AssertionError("make_case: could not clear the relu margin")
    return case
