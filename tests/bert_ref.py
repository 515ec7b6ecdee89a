"""The reference's TreeBERT baseline restated in plain torch (model/Twitter/BERT_Twitter.py:20-42:
``BertModel(is_decoder=True)`` on ``inputs_embeds``, eval mode, no attention mask, then ``fc`` and
``log_softmax``), looped over the trees one sequence at a time as the reference does, in fp64 (the
oracle) or fp32 (torch's own arithmetic).  No ``transformers`` import.  Also the seeded cases shared
by tests/test_bert.py, tests/test_gpu_bert.py (CASES) and tests/test_gpu_bert_edges.py (EDGE_CASES)."""
import functools
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

LN_EPS = 1e-12
QUERY_TILE = 32   # bgcn_bert_eval's queries per workgroup (BGCN_BERT_QUERY_TILE)
VOCAB = 8         # word_embeddings is never read: the cases keep it tiny


def make_state_dict(hidden, intermediate, layers, max_pos, out, seed, weight_factor=1.0, qk_factor=1.0):
    """A ``TreeBERT`` state dict drawn under ``seed`` in fp32: Linear and embedding weights normal with
    std 0.02 * weight_factor (the q and k weights of head 0 times ``qk_factor`` more), biases normal
    with the same std (so a misplaced bias shows), LayerNorm weights 1 + 0.3 n and biases 0.1 n (the
    spread of the weights spreads the rows' sums, which the rankings order)."""
    g = torch.Generator().manual_seed(seed)
    std = 0.02 * weight_factor
    sd = {}

    def lin(name, o, i, f=1.0):
        sd[name + ".weight"] = torch.randn(o, i, generator=g) * std
        sd[name + ".weight"][:64] *= f
        sd[name + ".bias"] = torch.randn(o, generator=g) * std

    def ln(name):
        sd[name + ".weight"] = 1.0 + 0.3 * torch.randn(hidden, generator=g)
        sd[name + ".bias"] = 0.1 * torch.randn(hidden, generator=g)

    e = "BERT.embeddings."
    sd[e + "word_embeddings.weight"] = torch.randn(VOCAB, hidden, generator=g) * std
    sd[e + "position_embeddings.weight"] = torch.randn(max_pos, hidden, generator=g) * std
    sd[e + "token_type_embeddings.weight"] = torch.randn(2, hidden, generator=g) * std
    ln(e + "LayerNorm")
    for i in range(layers):
        p = f"BERT.encoder.layer.{i}."
        lin(p + "attention.self.query", hidden, hidden, qk_factor)
        lin(p + "attention.self.key", hidden, hidden, qk_factor)
        lin(p + "attention.self.value", hidden, hidden)
        lin(p + "attention.output.dense", hidden, hidden)
        ln(p + "attention.output.LayerNorm")
        lin(p + "intermediate.dense", intermediate, hidden)
        lin(p + "output.dense", hidden, intermediate)
        ln(p + "output.LayerNorm")
    lin("BERT.pooler.dense", hidden, hidden)
    lin("fc", out, hidden)
    return sd


def _ln(v, sd, name):
    return F.layer_norm(v, (v.size(-1),), sd[name + ".weight"], sd[name + ".bias"], LN_EPS)


def _lin(v, sd, name):
    return F.linear(v, sd[name + ".weight"], sd[name + ".bias"])


def gelu(v):
    return v * 0.5 * (1.0 + torch.erf(v / math.sqrt(2.0)))


def encode(sd, seq, layers, heads):
    """One sequence ``seq [n, hidden]`` -> (last_hidden_state [n, hidden], per layer the attention
    probabilities [heads, n, n], the largest |score| that entered a softmax, per layer head 0's
    :func:`tile_gap` [n])."""
    n, hidden = seq.shape
    e = "BERT.embeddings."
    h = _ln(seq + sd[e + "position_embeddings.weight"][:n] + sd[e + "token_type_embeddings.weight"][0], sd,
            e + "LayerNorm")
    causal = torch.ones(n, n, dtype=torch.bool).tril()
    probs, top, gaps = [], 0.0, []
    for i in range(layers):
        p = f"BERT.encoder.layer.{i}."
        q, k, v = (_lin(h, sd, p + "attention.self." + w).view(n, heads, 64).transpose(0, 1)
                   for w in ("query", "key", "value"))
        s = (q @ k.transpose(1, 2)) / 8.0
        top = max(top, float(s[:, causal].abs().max()))
        P = torch.softmax(s.masked_fill(~causal, float("-inf")), dim=-1)
        probs.append(P)
        gaps.append(tile_gap(s[0]))
        ctx = (P @ v).transpose(0, 1).reshape(n, hidden)
        a = _ln(_lin(ctx, sd, p + "attention.output.dense") + h, sd, p + "attention.output.LayerNorm")
        h = _ln(_lin(gelu(_lin(a, sd, p + "intermediate.dense")), sd, p + "output.dense") + a, sd,
                p + "output.LayerNorm")
    return h, probs, top, gaps


def tile_gap(s):
    """Per query row of one head's scores ``s [n, n]``: the largest causal score among the keys of the
    later key tiles (key >= QUERY_TILE) minus the largest of the first tile's; nan for the rows that
    reach no later tile.  Positive: the running maximum moves after tile 0 and the sum so far is
    rescaled by exp(-gap); negative: the later tiles' terms are exp(gap) of the first's."""
    n = s.size(0)
    causal = torch.ones(n, n, dtype=torch.bool).tril()
    first = s[:, :QUERY_TILE].masked_fill(~causal[:, :QUERY_TILE], float("-inf")).amax(-1)
    if n <= QUERY_TILE:
        return torch.full((n,), float("nan"), dtype=s.dtype)
    later = s[:, QUERY_TILE:].masked_fill(~causal[:, QUERY_TILE:], float("-inf")).amax(-1)
    return torch.where(torch.isinf(later), torch.full_like(later, float("nan")), later - first)


def rank(values):
    """topk(k = n) under bgcn_segment_rank's tie rule: descending, equal values by ascending index."""
    order = torch.sort(-values, stable=True).indices
    return order, values[order]


@torch.no_grad()
def run(sd, x, rootindex, layers, heads, y=None, dtype=torch.float64):
    """The reference's loop over one batch: tree b = x[rootindex[b] : rootindex[b + 1]] (the last to
    N).  hidden [N, hidden] / hidden_sum [N] / attn_sum [N] are zeros above rootindex[0]."""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    x = x.to(dtype)
    roots = [int(v) for v in rootindex.tolist()]
    N, B, hidden = x.size(0), len(roots), x.size(1)
    res = SimpleNamespace(hidden=torch.zeros(N, hidden, dtype=dtype), attn_sum=torch.zeros(N, dtype=dtype),
                          logp=torch.zeros(B, sd["fc.weight"].size(0), dtype=dtype), pooled=torch.zeros(B, hidden, dtype=dtype),
                          row_max=[], top_score=0.0, rank_hidden=[], rank_attn=[], loss=None, tile_gap=[])
    for b, r in enumerate(roots):
        end = N if b == B - 1 else roots[b + 1]
        h, probs, top, gaps = encode(sd, x[r:end], layers, heads)
        res.tile_gap.append(gaps)   # [tree][layer] -> [n], head 0
        res.hidden[r:end] = h
        # attention_head.sum(-2).sum(1) per layer (explain_PHEME.py:590), summed over the layers
        res.attn_sum[r:end] = sum(P.sum(-2).sum(0) for P in probs)
        res.top_score = max(res.top_score, top)
        for P in probs:
            if end - r >= 8:
                res.row_max.append(P[:, 7:].amax(-1).flatten())   # rows with at least 8 keys
        res.pooled[b] = torch.tanh(_lin(h[0], sd, "BERT.pooler.dense"))
        res.logp[b] = F.log_softmax(_lin(res.pooled[b], sd, "fc"), dim=-1)
    res.hidden_sum = res.hidden.sum(-1)
    for b, r in enumerate(roots):
        end = N if b == B - 1 else roots[b + 1]
        res.rank_hidden.append(rank(res.hidden_sum[r:end]))
        res.rank_attn.append(rank(res.attn_sum[r:end]))
    res.row_max = torch.cat(res.row_max) if res.row_max else torch.zeros(0, dtype=dtype)
    res.pred = res.logp.max(dim=1)[1]
    if y is not None:
        res.loss = F.nll_loss(res.logp, y)
        res.correct = int(res.pred.eq(y).sum())
    return res


# ---- the cases (the issue's table); sizes the table leaves open are the smallest the kernels take.
# weight_factor: with std-0.02 weights attention is near-uniform and hides indexing errors.
_SMALL = dict(hidden=128, intermediate=256, layers=2, max_pos=512, out=4, weight_factor=6.0)
CASES = {
    "single": dict(_SMALL, lengths=[1]),
    "boundaries": dict(_SMALL, lengths=[1, 2, 31, 32, 33, 63, 64, 65]),
    "cap": dict(_SMALL, layers=1, lengths=[512, 511]),
    "offset_strided": dict(_SMALL, lengths=[3, 12, 9], first=2, pad_cols=8),
    "many": dict(_SMALL, hidden=64, intermediate=64, layers=1, lengths=[1 + b % 2 for b in range(130)]),
    "full_width": dict(hidden=768, intermediate=3072, layers=2, max_pos=512, out=4, weight_factor=2.5,
                       lengths=[1, 14, 25]),
    # head 0's q / k weights scaled until its scores pass +-88 on their way into the softmax: exp
    # overflows fp32 without the max subtraction.  Head 1 keeps the spread condition's soft rows.
    "sharp": dict(_SMALL, intermediate=128, layers=1, lengths=[12, 24], qk_factor=4.0),
}
# ---- the edge cases of tests/test_gpu_bert_edges.py: shapes and paths the table above does not
# reach.  Each entry carries its own seed (case() derives a seed from the name's position in
# sorted(CASES), so CASES itself must not grow).  The seeds, weight_factor and qk_factor are chosen so
# that tests/test_bert.py's conditions hold at their limits (feasibility 1e-5, 5 % left out, spread,
# prediction gap, sharp_tiles' cross-tile gaps).
_LENGTHS_5 = [2, 5, 1, 9, 3]
EDGE_CASES = {
    # B = 300 > 256: the second iteration of the setup's loops over B; roots, head and finish at B = 300
    "many_trees": dict(_SMALL, hidden=64, intermediate=64, layers=1, lengths=[1 + b % 3 for b in range(300)],
                       first=3, seed=251),
    # 3 heads and query tiles 0 .. 2: the partial column sums' [qt][head][row] index
    "heads3_tiles": dict(_SMALL, hidden=192, intermediate=192, lengths=[70, 33, 1, 96], weight_factor=4.0, seed=202),
    # head 0's scores spread until the largest of a later key tile is more than 10 above (and, in other
    # rows, below) the first tile's: the running maximum's and sum's rescale across key tiles
    "sharp_tiles": dict(_SMALL, intermediate=128, layers=1, lengths=[70, 100], weight_factor=1.5, qk_factor=16.0,
                        seed=203),
    # kMaxHidden: 16 values per lane in ln_row, 16 heads, the head's whole pooled[] array
    "hidden_1024": dict(_SMALL, hidden=1024, intermediate=64, layers=1, lengths=[5, 40], weight_factor=2.0, seed=204),
    # 5 heads (odd per); the head's dot product has a partly active second iteration; the largest intermediate
    "hidden_320": dict(_SMALL, hidden=320, intermediate=4096, layers=1, lengths=[3, 34], weight_factor=3.0, seed=205),
    # every slot of bgcn_bert_args::layer; attn_sum accumulated 24 times
    "layers_24": dict(_SMALL, hidden=64, intermediate=64, layers=24, lengths=[1, 9, 33], weight_factor=2.0, seed=206),
    # the head's class loop over the four waves, seq_head_tail at 1, 63 and 64 lanes
    "classes_1": dict(_SMALL, out=1, lengths=_LENGTHS_5, seed=207),
    "classes_63": dict(_SMALL, out=63, lengths=_LENGTHS_5, seed=208),
    "classes_64": dict(_SMALL, out=64, lengths=_LENGTHS_5, seed=209),
    # every grid is sized from max_pos: not a multiple of 32 or 256, and the cap at a max_pos other than 512
    "short_pos": dict(_SMALL, max_pos=40, lengths=[40, 39, 8], seed=210),
    # N = 8217 >= kX6MinRows: every full-form GEMM on the six-product bf16-MFMA kernel; the root-only
    # form of the same batch (127 rows) stays on the exact-fp32 one
    "rows_over_switch": dict(_SMALL, intermediate=128, layers=1, lengths=[65] * 126 + [27], seed=211),
}
PRED_GAP = 2e-4    # the oracle's top-1 to top-2 logp gap of every edge-case tree exceeds this: twice the GPU bar
TILE_GAP = 10.0    # sharp_tiles: rows whose later tiles lead the first by more than this, and rows the other way
RANK_GAP = 2e-4    # positions whose oracle value is closer than this to a neighbour's are not compared
RANK_SKIP = 0.05   # at most this share of a case's positions may be left out that way


def _make(name, c, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    first = c.get("first", 0)
    N = first + sum(c["lengths"])
    wide = torch.randn(N, c["hidden"] + c.get("pad_cols", 0), generator=g)
    x = wide[:, :c["hidden"]]             # a column slice when pad_cols > 0 (ldx > hidden)
    starts, s = [], first
    for n in c["lengths"]:
        starts.append(s)
        s += n
    rootindex = torch.tensor(starts, dtype=torch.int64)
    y = torch.randint(0, c["out"], (len(starts),), generator=g)
    sd = make_state_dict(c["hidden"], c["intermediate"], c["layers"], c["max_pos"], c["out"], seed,
                         c["weight_factor"], c.get("qk_factor", 1.0))
    heads = c["hidden"] // 64
    ref = run(sd, x, rootindex, c["layers"], heads, y)
    batch = torch.repeat_interleave(torch.arange(len(starts)), torch.tensor(c["lengths"]))
    return SimpleNamespace(name=name, cfg=c, seed=seed, x=x, rootindex=rootindex, y=y, N=N, B=len(starts), first=first,
                           heads=heads, sd=sd, ref=ref, batch=batch)


@functools.lru_cache(maxsize=None)
def case(name):
    """The seeded inputs of a case and its fp64 oracle, computed once and shared (read-only)."""
    return _make(name, CASES[name], sorted(CASES).index(name) + 1)


@functools.lru_cache(maxsize=None)
def edge_case(name):
    """As case(), for EDGE_CASES and the entry's own seed."""
    c = EDGE_CASES[name]
    return _make(name, c, c["seed"])


def pred_gap(logp):
    """The smallest top-1 to top-2 gap of ``logp [B, C]`` over the trees (inf for one class)."""
    if logp.size(1) < 2:
        return float("inf")
    top = logp.topk(2, dim=1).values
    return float((top[:, 0] - top[:, 1]).min())


def model_for(c, device=None):
    """A ``bigcn_amd.TreeBERT`` of the case's sizes holding the case's weights, in eval mode."""
    from bigcn_amd import TreeBERT
    cfg = c.cfg
    m = TreeBERT(hidden=cfg["hidden"], heads=c.heads, intermediate=cfg["intermediate"], num_layers=cfg["layers"],
                 max_pos=cfg["max_pos"], vocab=VOCAB, num_classes=cfg["out"])
    m.load_state_dict(c.sd, strict=True)
    if device is not None:
        m = m.to(device)
    return m.eval()


def rank_compared(sorted_values):
    """The positions of one tree's oracle ranking whose value is more than RANK_GAP from both neighbours'."""
    gap = (sorted_values[:-1] - sorted_values[1:]).abs() > RANK_GAP
    ok = torch.ones(sorted_values.numel(), dtype=torch.bool)
    ok[:-1] &= gap
    ok[1:] &= gap
    return ok
