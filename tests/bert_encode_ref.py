"""The feature extraction of the PHEME study (Process/getPHEMEgraph.py:104-118) restated in plain torch:

    embeddings = model.embeddings(input_ids)         # [n, T, hidden]
    cls = model(input_ids).pooler_output             # [n, hidden]

with ``model`` a plain ``BertModel`` in eval mode: not a decoder, no attention mask, so every position
(padding included) attends to every other.  fp64 is the oracle, fp32 torch's own arithmetic.  No
``transformers`` import (tests/test_bert_encode.py compares this file with ``transformers`` where it is
installed).  Also the seeded cases shared by tests/test_bert_encode.py and tests/test_gpu_bert_encode.py.
"""
import functools
from types import SimpleNamespace

import torch

import bert_ref as R

BAR = 1e-4        # the GPU tests' bar against the fp64 oracle (bert_gpu_util.BAR)
KEY_TILE = 32     # keys per tile of the attention kernel (BGCN_BERT_QUERY_TILE)
QUERY_BLOCK = 128  # queries per workgroup of the attention kernel: four tiles
TILE_GAP = 10.0   # "sharp": rows whose later key tiles lead the first by more than this, and rows the other way


def make_state_dict(hidden, intermediate, layers, max_pos, vocab, seed, weight_factor=1.0, qk_factor=1.0):
    """A ``BertModel`` state dict (its own names: ``embeddings.word_embeddings.weight`` ...
    ``pooler.dense.bias``) drawn as :func:`bert_ref.make_state_dict` draws a TreeBERT's: weights normal
    with std 0.02 * weight_factor (head 0's q and k times ``qk_factor`` more), random biases (so a
    misplaced bias shows), LayerNorm weights 1 + 0.3 n and biases 0.1 n (so a misplaced row shows);
    ``word_embeddings`` has ``vocab`` rows of its own draw."""
    sd = R.make_state_dict(hidden, intermediate, layers, max_pos, 1, seed, weight_factor, qk_factor)
    sd = {k[len("BERT."):]: v for k, v in sd.items() if k.startswith("BERT.")}
    g = torch.Generator().manual_seed(7000 + seed)
    sd["embeddings.word_embeddings.weight"] = torch.randn(vocab, hidden, generator=g) * 0.02 * weight_factor
    return sd


def tile_gap(s):
    """Per query row of one head's scores ``s [..., T, T]``: the largest score among the keys of the later
    key tiles (key >= KEY_TILE) minus the largest of the first tile's; nan when there is one tile only.
    Positive: the running maximum moves after tile 0 and the sum so far is rescaled by exp(-gap)."""
    if s.size(-1) <= KEY_TILE:
        return torch.full(s.shape[:-1], float("nan"), dtype=s.dtype)
    return s[..., KEY_TILE:].amax(-1) - s[..., :KEY_TILE].amax(-1)


def embeddings(sd, ids):
    """``model.embeddings(ids)`` for ``ids [n, T]``: token type 0, positions 0 .. T - 1."""
    e = "embeddings."
    T = ids.size(1)
    v = sd[e + "word_embeddings.weight"][ids] + sd[e + "token_type_embeddings.weight"][0] \
        + sd[e + "position_embeddings.weight"][:T]
    return R._ln(v, sd, e + "LayerNorm")


@torch.no_grad()
def run(sd, ids, layers, heads, dtype=torch.float64):
    """``embeddings [n, T, hidden]``, ``hidden`` (last_hidden_state) and ``cls [n, hidden]`` (pooler_output)
    of ``ids [n, T]``; ``tile_gap``: per layer head 0's :func:`tile_gap` ``[n, T]``; ``top_score``."""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    n, T = ids.shape
    emb = embeddings(sd, ids)
    h, hidden = emb, emb.size(-1)
    gaps, top = [], 0.0
    for i in range(layers):
        p = f"encoder.layer.{i}."
        q, k, v = (R._lin(h, sd, p + "attention.self." + w).view(n, T, heads, 64).transpose(1, 2)
                   for w in ("query", "key", "value"))
        s = (q @ k.transpose(2, 3)) / 8.0
        top = max(top, float(s.abs().max()))
        gaps.append(tile_gap(s[:, 0]))
        ctx = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(n, T, hidden)
        a = R._ln(R._lin(ctx, sd, p + "attention.output.dense") + h, sd, p + "attention.output.LayerNorm")
        h = R._ln(R._lin(R.gelu(R._lin(a, sd, p + "intermediate.dense")), sd, p + "output.dense") + a, sd,
                  p + "output.LayerNorm")
    cls = torch.tanh(R._lin(h[:, 0], sd, "pooler.dense"))
    return SimpleNamespace(embeddings=emb, hidden=h, cls=cls, tile_gap=gaps, top_score=top)


# ---- the cases.  weight_factor: with std-0.02 weights attention is near-uniform and hides indexing errors.
_SMALL = dict(hidden=128, intermediate=128, layers=2, vocab=16, max_pos=192, weight_factor=6.0)
EDGE_T = (1, 31, 32, 33, 70, QUERY_BLOCK + 1, 192)   # 70: three key tiles, the last partial; 129: a second workgroup
EDGE_N = (1, 3, 5)
CASES = {f"t{T}_n{n}": dict(_SMALL, T=T, n=n) for T in EDGE_T for n in EDGE_N}
# head 0's q / k weights scaled (bert_ref's qk_factor) until a later key tile's largest score leads the first
# tile's by more than TILE_GAP in some rows and trails it by as much in others: the running maximum moves
# and the sum so far is rescaled
CASES["sharp"] = dict(_SMALL, layers=1, T=100, n=2, weight_factor=1.5, qk_factor=16.0)
# M = n T = 8192 is kX6MinRows, where every [M, .] GEMM changes kernel; n = 63 stays just below it
CASES["rows_at_switch"] = dict(_SMALL, layers=1, T=128, n=64)
CASES["rows_under_switch"] = dict(_SMALL, layers=1, T=128, n=63)
_NAMES = sorted(CASES)


def make_ids(n, T, vocab, g):
    """Random ids with what the tokenizer's output has: a run of 0 (padding, attended like any token) at the
    end of every sequence of more than two tokens, and ``vocab - 1`` in every sequence's first position or,
    in the odd sequences, just before the padding."""
    ids = torch.randint(0, vocab, (n, T), generator=g)
    for b in range(n):
        pad = (T // 3 + b) % T if T > 2 else 0
        if pad:
            ids[b, T - pad:] = 0
        ids[b, (T - pad - 1) if b % 2 else 0] = vocab - 1
    return ids


@functools.lru_cache(maxsize=None)
def case(name):
    """The seeded inputs of a case and its fp64 oracle, computed once and shared (read-only).  The two
    switch cases share weights and ids: the first 63 sequences of one are the other's."""
    c = CASES[name]
    shared = "rows_at_switch" if name == "rows_under_switch" else name
    seed = 300 + _NAMES.index(shared)
    heads = c["hidden"] // 64
    sd = make_state_dict(c["hidden"], c["intermediate"], c["layers"], c["max_pos"], c["vocab"], seed,
                         c["weight_factor"], c.get("qk_factor", 1.0))
    ids = make_ids(CASES[shared]["n"], c["T"], c["vocab"], torch.Generator().manual_seed(1000 + seed))[:c["n"]]
    return SimpleNamespace(name=name, cfg=c, seed=seed, heads=heads, sd=sd, ids=ids,
                           ref=run(sd, ids, c["layers"], heads))


def model_for(c, device=None):
    """A ``bigcn_amd.TweetEncoder`` of the case's sizes holding the case's weights."""
    from bigcn_amd import TweetEncoder
    cfg = c.cfg
    m = TweetEncoder(hidden=cfg["hidden"], heads=c.heads, intermediate=cfg["intermediate"], num_layers=cfg["layers"],
                     max_pos=cfg["max_pos"], vocab=cfg["vocab"])
    m.load_state_dict(c.sd, strict=True)
    return m if device is None else m.to(device)
