"""The reference's TreeBERT training-loop body (model/Twitter/BERT_Twitter.py:89-119) restated in
plain torch with autograd, shared by tests/test_bert_train.py (CPU) and tests/test_gpu_bert_train.py.

(a) The loop body: one *full-sequence* causal encoder call per tree (``BertModel(is_decoder=True)`` on
    ``inputs_embeds`` in training mode: dropout after the embeddings' LayerNorm, on the attention
    probabilities, after ``attention.output.dense`` and after ``output.dense``), ``fc``,
    ``log_softmax``, ``nll_loss``, ``backward``, ``torch.optim.Adam(lr=5e-4, weight_decay=1e-4)``, in
    fp64 (the oracle) or fp32 (torch's own arithmetic).  Trees of one length go through the encoder
    as one batch: a tree is still one sequence of its own.  The masks of a tree's first row (and of
    the one probability its first row keeps, per head) come from (b); the masks of every other row
    come from a torch generator.
(b) bgcn_bert_train_grad's keep function (include/bgcn.h) restated bit for bit in integer torch ops.
(c) TRAIN_CASES with their own seeds: the smallest shapes reaching each path of the native call.

bert_ref.py's ``make_state_dict``, ``_ln``, ``_lin`` and ``gelu`` are reused as they are."""
import functools
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

import bert_ref as R

BAR = 1e-4            # max|got - ref| / max|ref| per gradient tensor; absolute on loss and logp
LR, WEIGHT_DECAY = 5e-4, 1e-4
DROPS = {"p0": (0.0, 0.0), "p01": (0.1, 0.1)}   # (hidden_dropout, attn_dropout)
DROP_SEED = 0x1234_5678_9ABC_DEF1

# ---------------------------------------------------------------- (b) the keep function
_M32 = 0xFFFFFFFF


def _mul32(x, c):
    """(x * c) mod 2^32 for an int64 tensor x in [0, 2^32) without leaving int64's range."""
    return (x * (c & 0xFFFF) + (((x * (c >> 16)) & 0xFFFF) << 16)) & _M32


def mix32(x):
    x = x ^ (x >> 16)
    x = _mul32(x, 0x7FEB352D)
    x = x ^ (x >> 15)
    x = _mul32(x, 0x846CA68B)
    return x ^ (x >> 16)


def drop_hash(seed, site, b, j):
    """hash(seed, site, b, j) of include/bgcn.h; ``b`` and ``j`` int64 tensors (broadcast together)."""
    seed = int(seed) & (2 ** 64 - 1)
    lo, hi = seed & _M32, seed >> 32
    base = mix32(mix32(b ^ lo) ^ ((site * 0x9E3779B9 + hi) & _M32))
    return mix32(base ^ _mul32(j, 0x85EBCA6B))


def _f32(p):
    return torch.tensor(float(p), dtype=torch.float32)


def drop_threshold(p):
    return int(math.floor(float(_f32(p).double()) * 4294967296.0 + 0.5))


def drop_scale(p):
    """The fp32 quotient 1.0f / (1.0f - p), as a Python float."""
    return float(torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) - _f32(p)))


def keep(seed, site, b, j, p):
    """Whether the draw of (site, tree b, column or head j) is kept at rate ``p``: a bool tensor."""
    b = torch.as_tensor(b, dtype=torch.int64)
    j = torch.as_tensor(j, dtype=torch.int64)
    return drop_hash(seed, site, b, j) >= drop_threshold(p)


# ---------------------------------------------------------------- (a) the loop body
def _encode(P, seq, masks, layers, heads, scale_h, scale_a):
    """``seq [G, n, hidden]``: G sequences of n rows, each on its own -> last_hidden_state."""
    G, n, hidden = seq.shape
    e = "BERT.embeddings."
    h = R._ln(seq + P[e + "position_embeddings.weight"][:n] + P[e + "token_type_embeddings.weight"][0], P,
              e + "LayerNorm")
    h = h * masks[0] * scale_h
    causal = torch.ones(n, n, dtype=torch.bool).tril()
    for i in range(layers):
        p = f"BERT.encoder.layer.{i}."
        q, k, v = (R._lin(h, P, p + "attention.self." + w).view(G, n, heads, 64).transpose(1, 2)
                   for w in ("query", "key", "value"))
        s = (q @ k.transpose(2, 3)) / 8.0
        prob = torch.softmax(s.masked_fill(~causal, float("-inf")), dim=-1) * masks[3 * i + 1] * scale_a
        ctx = (prob @ v).transpose(1, 2).reshape(G, n, hidden)
        a = R._ln(R._lin(ctx, P, p + "attention.output.dense") * masks[3 * i + 2] * scale_h + h, P,
                  p + "attention.output.LayerNorm")
        h = R._ln(R._lin(R.gelu(R._lin(a, P, p + "intermediate.dense")), P, p + "output.dense") * masks[3 * i + 3]
                  * scale_h + a, P, p + "output.LayerNorm")
    return h


def _masks(trees, n, hidden, heads, layers, seed, p_h, p_a, gen, dtype):
    """The masks of one group of trees (indices ``trees``) of n rows, per site: [G, n, hidden], or
    [G, heads, n, n] for the attention sites.  First row / first probability: the keep function."""
    G = len(trees)
    b = torch.tensor(trees, dtype=torch.int64)[:, None]
    out = []
    for site in range(3 * layers + 1):
        if site % 3 == 1:
            m = torch.rand(G, heads, n, n, generator=gen) >= p_a
            m[:, :, 0, 0] = keep(seed, site, b, torch.arange(heads)[None, :], p_a)
        else:
            m = torch.rand(G, n, hidden, generator=gen) >= p_h
            m[:, 0, :] = keep(seed, site, b, torch.arange(hidden)[None, :], p_h)
        out.append(m.to(dtype))
    return out


def forward(P, x, rootindex, layers, heads, seed, p_h, p_a, other_seed=0):
    """``logp [B, C]`` of the batch in training mode; ``P`` the parameters by ``state_dict`` name."""
    roots = [int(v) for v in rootindex.tolist()]
    N, B, hidden = x.size(0), len(roots), x.size(1)
    ends = roots[1:] + [N]
    by_len = {}
    for b, (r, e) in enumerate(zip(roots, ends)):
        by_len.setdefault(e - r, []).append(b)
    gen = torch.Generator().manual_seed(77 + other_seed)
    scale_h, scale_a = drop_scale(p_h), drop_scale(p_a)
    pooled = [None] * B
    for n, trees in sorted(by_len.items()):
        seq = torch.stack([x[roots[b]:roots[b] + n] for b in trees])
        masks = _masks(trees, n, hidden, heads, layers, seed, p_h, p_a, gen, x.dtype)
        h = _encode(P, seq, masks, layers, heads, scale_h, scale_a)
        out = torch.tanh(R._lin(h[:, 0], P, "BERT.pooler.dense"))
        for k, b in enumerate(trees):
            pooled[b] = out[k]
    return F.log_softmax(R._lin(torch.stack(pooled), P, "fc"), dim=-1)


def grad_names(c):
    """The names bgcn_bert_train_grad writes a gradient for: all but word_embeddings."""
    return [k for k in c.sd if "word_embeddings" not in k]


def loss_and_grads(c, dtype, p_h, p_a, seed=DROP_SEED, other_seed=0, x=None):
    """One loop body up to ``backward``: loss, logp and the gradients by name, plus ``"x"``."""
    P = {k: v.to(dtype).clone().requires_grad_(True) for k, v in c.sd.items()}
    x = (c.x if x is None else x).to(dtype).clone().requires_grad_(True)
    logp = forward(P, x, c.rootindex, c.cfg["layers"], c.heads, seed, p_h, p_a, other_seed)
    loss = F.nll_loss(logp, c.y)
    loss.backward()
    grads = {k: P[k].grad.detach() for k in grad_names(c)}
    assert P["BERT.embeddings.word_embeddings.weight"].grad is None
    grads["x"] = x.grad.detach()
    return SimpleNamespace(loss=loss.detach(), logp=logp.detach(), grads=grads, pred=logp.detach().max(dim=1)[1])


def train_losses(c, steps, dtype, p_h, p_a, seed=DROP_SEED):
    """``steps`` iterations of the loop with torch.optim.Adam, step k drawing its masks from ``seed + k``:
    the losses and the final parameters."""
    P = {k: v.to(dtype).clone().requires_grad_(True) for k, v in c.sd.items()}
    opt = torch.optim.Adam(list(P.values()), lr=LR, weight_decay=WEIGHT_DECAY)
    x = c.x.to(dtype)
    losses = []
    for k in range(steps):
        opt.zero_grad()
        loss = F.nll_loss(forward(P, x, c.rootindex, c.cfg["layers"], c.heads, seed + k, p_h, p_a, k), c.y)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses, {k: v.detach() for k, v in P.items()}


def rel_err(got, ref):
    """The project's gradient metric max|got - ref| / max|ref|; an all-zero reference demands exact
    zeros (0.0 then, else inf)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    top = float(ref.abs().max())
    if top == 0.0:
        return 0.0 if float(got.abs().max()) == 0.0 else float("inf")
    return float((got - ref).abs().max()) / top


# ---------------------------------------------------------------- (c) the cases
_SMALL = dict(hidden=128, intermediate=256, layers=2, max_pos=512, out=4, weight_factor=6.0)
_LENGTHS_5 = [2, 5, 1, 9, 3]
TRAIN_CASES = {
    # B = 1, one row: gemm_tn over a reduction of length 1, every column sum over one row
    "t_single": dict(_SMALL, lengths=[1], seed=301),
    # lengths around the eval path's tiles, rows above the first tree, a row stride above hidden
    "t_boundaries": dict(_SMALL, lengths=[1, 2, 31, 33, 64], first=2, pad_cols=8, seed=302),
    # B = 300 > 256: the setup's second pass over B, more than one block of every row kernel
    "t_many_trees": dict(_SMALL, hidden=64, intermediate=64, layers=1, lengths=[1 + b % 3 for b in range(300)],
                         first=3, seed=303),
    # kMaxHidden: 16 values per lane in both LN kernels, 16 heads
    "t_hidden_1024": dict(_SMALL, hidden=1024, intermediate=64, layers=1, lengths=[2, 3], weight_factor=2.0, seed=304),
    # 5 heads (odd per), the widest intermediate
    "t_hidden_320": dict(_SMALL, hidden=320, intermediate=4096, layers=1, lengths=[3, 1, 2], weight_factor=3.0, seed=305),
    # every slot of d_layer, 392 tensors for the chunked optimiser
    "t_layers_24": dict(_SMALL, hidden=64, intermediate=64, layers=24, lengths=[1, 4, 2], weight_factor=2.0, seed=306),
    # BERT-base's widths
    "t_full_width": dict(hidden=768, intermediate=3072, layers=2, max_pos=512, out=4, weight_factor=2.5,
                         lengths=[1, 3, 2], seed=307),
    # one class: softmax = 1, dz = 0, every gradient exactly zero
    "t_classes_1": dict(_SMALL, out=1, lengths=_LENGTHS_5, seed=308),
    "t_classes_63": dict(_SMALL, out=63, lengths=_LENGTHS_5, seed=309),
    # B = 8200 >= the GEMMs' row switch: the six-product forward GEMM where its shape allows, gemm_tn
    # with its reduction split
    "t_rows_over_switch": dict(_SMALL, hidden=64, intermediate=128, layers=1, lengths=[1] * 8200, seed=310),
}
# (case, dropout setting): every case at both settings but t_classes_1, whose gradients are all zero
PARITY = [(n, d) for n in TRAIN_CASES for d in DROPS if not (n == "t_classes_1" and d == "p01")]


@functools.lru_cache(maxsize=None)
def case(name):
    """The seeded inputs of a case (read-only, shared)."""
    c = TRAIN_CASES[name]
    seed = c["seed"]
    g = torch.Generator().manual_seed(1000 + seed)
    first = c.get("first", 0)
    N = first + sum(c["lengths"])
    wide = torch.randn(N, c["hidden"] + c.get("pad_cols", 0), generator=g)
    x = wide[:, :c["hidden"]]             # a column slice when pad_cols > 0 (ldx > hidden)
    starts = (torch.tensor([first] + c["lengths"][:-1]).cumsum(0)).tolist()
    rootindex = torch.tensor(starts, dtype=torch.int64)
    y = torch.randint(0, c["out"], (len(starts),), generator=g)
    sd = R.make_state_dict(c["hidden"], c["intermediate"], c["layers"], c["max_pos"], c["out"], seed,
                           c["weight_factor"])
    return SimpleNamespace(name=name, cfg=c, seed=seed, x=x, rootindex=rootindex, y=y, N=N, B=len(starts), first=first,
                           heads=c["hidden"] // 64, sd=sd)


@functools.lru_cache(maxsize=None)
def oracle(name, drop):
    """The fp64 loop body of a case at a dropout setting of DROPS, computed once and shared."""
    p_h, p_a = DROPS[drop]
    return loss_and_grads(case(name), torch.float64, p_h, p_a)
