"""The reference's LSTM baseline restated (model/Twitter/LSTM_Twitter.py:19-49 and the test loop
:146-173): ``torch.nn.LSTM`` + ``Linear`` on the CPU, looped over the trees one sequence at a time
exactly as the reference does, in fp64 (the oracle) or fp32 (the reference's own arithmetic).
Also the seeded case generators shared by tests/test_lstm.py, tests/test_gpu_lstm.py (CASES) and
tests/test_gpu_lstm_edges.py (EDGE_CASES)."""
import functools
from types import SimpleNamespace

import torch
import torch.nn.functional as F

SATURATED_FACTOR = 4.0   # the "saturated" variant multiplies every LSTM weight by this


def build(in_feats, hid, out_feats, num_layers, dtype=torch.float64, seed=0, weight_factor=1.0):
    """(lstm, fc) as the reference's constructor makes them, torch's default init under ``seed``
    (drawn in fp32, then cast, so every dtype holds the same values)."""
    torch.manual_seed(seed)
    lstm = torch.nn.LSTM(in_feats, hid, num_layers=num_layers, batch_first=True, bidirectional=True, bias=False)
    fc = torch.nn.Linear(hid * num_layers * 2, out_feats)
    if weight_factor != 1.0:
        with torch.no_grad():
            for p in lstm.parameters():
                p.mul_(weight_factor)
    return lstm.to(dtype).eval(), fc.to(dtype).eval()


def state_dict(lstm, fc):
    sd = {"lstm." + k: v.detach().clone() for k, v in lstm.state_dict().items()}
    sd.update({"fc." + k: v.detach().clone() for k, v in fc.state_dict().items()})
    return sd


def _sub_lstm(lstm, layers):
    """The first ``layers`` layers of ``lstm`` as a module of their own (per-layer outputs)."""
    sub = torch.nn.LSTM(lstm.input_size, lstm.hidden_size, num_layers=layers, batch_first=True, bidirectional=True,
                        bias=False).to(lstm.weight_ih_l0.dtype)
    sub.load_state_dict({k: v for k, v in lstm.state_dict().items() if int(k.split("_l")[1][0]) < layers})
    return sub.eval()


@torch.no_grad()
def run(lstm, fc, x, rootindex, y=None):
    """The reference's loop over one batch: tree b = x[rootindex[b] : rootindex[b + 1]] (the last
    to N), each an unbatched sequence.  Returns layer_out (per layer [N, 2H], zeros above
    rootindex[0]), h_n [2L, B, H], logp [B, C], loss, pred."""
    dtype = lstm.weight_ih_l0.dtype
    x = x.to(dtype)
    roots = [int(v) for v in rootindex.tolist()]
    N, B, H, L = x.size(0), len(roots), lstm.hidden_size, lstm.num_layers
    subs = [_sub_lstm(lstm, l + 1) for l in range(L - 1)] + [lstm]
    layer_out = [torch.zeros(N, 2 * H, dtype=dtype) for _ in range(L)]
    h_n = torch.zeros(2 * L, B, H, dtype=dtype)
    logp = torch.zeros(B, fc.out_features, dtype=dtype)
    for b, r in enumerate(roots):
        sl = x[r:] if b == B - 1 else x[r:roots[b + 1]]
        for l in range(L):
            out, (hn, _) = subs[l](sl)
            layer_out[l][r:r + sl.size(0)] = out
        h_n[:, b] = hn
        logp[b] = F.log_softmax(fc(hn.reshape(-1, H * L * 2)), dim=1)[0]
    res = SimpleNamespace(layer_out=layer_out, out=layer_out[-1], h_n=h_n, logp=logp, loss=None, pred=logp.max(dim=1)[1])
    if y is not None:
        res.loss = F.nll_loss(logp, y)
        res.correct = int(res.pred.eq(y).sum())
    return res


@torch.no_grad()
def run_packed(lstm, fc, x, rootindex):
    """The same batch as one padded-and-packed nn.LSTM call: (out [N, 2H] from rootindex[0] on, h_n, logp)."""
    roots = [int(v) for v in rootindex.tolist()]
    ends = roots[1:] + [x.size(0)]
    seqs = [x[s:e].to(lstm.weight_ih_l0.dtype) for s, e in zip(roots, ends)]
    packed = torch.nn.utils.rnn.pack_sequence(seqs, enforce_sorted=False)
    out, (hn, _) = lstm(packed)
    pad, lens = torch.nn.utils.rnn.pad_packed_sequence(out, batch_first=True)
    rows = torch.cat([pad[b, :int(lens[b])] for b in range(len(seqs))])
    flat = hn.transpose(0, 1).reshape(len(seqs), -1)
    return rows, hn, F.log_softmax(fc(flat), dim=1)


# ---- the cases of tests/test_gpu_lstm.py (the issue's table); dimensions the table leaves open
# are the smallest the kernels take
SEQ_TILE = 32   # bgcn_lstm_eval's sequences per workgroup (BGCN_LSTM_SEQ_TILE)
CASES = {
    "boundaries": dict(in_feats=20, hid=64, layers=2, out=4, lengths=[1, 2, 3, 33, 64, 65]),
    "pheme": dict(in_feats=768, hid=768, layers=2, out=4, lengths=[1, 2, 67, 5]),
    "twitter": dict(in_feats=5000, hid=64, layers=2, out=64, lengths=[3, 1, 40]),
    "tile_plus_one": dict(in_feats=20, hid=64, layers=2, out=4, lengths=[1 + b % 5 for b in range(SEQ_TILE + 1)]),
    "one_layer": dict(in_feats=20, hid=64, layers=1, out=4, lengths=[1, 4, 9]),
    "three_layers": dict(in_feats=20, hid=64, layers=3, out=4, lengths=[1, 4, 9]),
    "offset_strided": dict(in_feats=768, hid=64, layers=2, out=4, lengths=[3, 7], first=2, pad_cols=8),
    "saturated": dict(in_feats=20, hid=64, layers=2, out=4, lengths=[1, 2, 3, 33, 64, 65],
                      weight_factor=SATURATED_FACTOR),
}


# ---- the edge cases of tests/test_gpu_lstm_edges.py: shapes the table above does not reach.  Each
# entry carries its own seed (case() derives a seed from the name's position in sorted(CASES), so
# CASES itself must not grow: a new name there would change every existing case's data).
EDGE_CASES = {
    # B = 300 > 256: the second iteration of the setup's and the finish's loops over B; 10 sequence tiles
    "many_trees": dict(in_feats=8, hid=64, layers=1, out=4, lengths=[1 + b % 3 for b in range(300)], seed=101),
    # two and four iterations of a wave's k loop in the step
    "hid_128": dict(in_feats=12, hid=128, layers=2, out=5, lengths=[1, 5, 18, 2], seed=112),
    "hid_256": dict(in_feats=12, hid=256, layers=1, out=3, lengths=[1, 7, 3], seed=103),
    # the largest configuration the entry point takes: the head's h_n holds 2 L H = 8192 values
    "largest": dict(in_feats=4, hid=1024, layers=4, out=3, lengths=[2, 1, 3], seed=104),
    # N = 8217 rows: both layers' input GEMMs run on the six-product kernel (8192 rows and more)
    "rows_over_switch": dict(in_feats=20, hid=64, layers=2, out=4,
                             lengths=[1 + (37 * b) % 129 for b in range(126)], seed=105),
    "one_class": dict(in_feats=8, hid=64, layers=1, out=1, lengths=[1, 4, 2], seed=106),
    "classes_63": dict(in_feats=8, hid=64, layers=1, out=63, lengths=[1, 4, 2], seed=107),
    # rows above the first start, more than one sequence tile
    "offset_many": dict(in_feats=8, hid=64, layers=2, out=4, lengths=[1 + b % 4 for b in range(40)], first=5,
                        seed=108),
}


def _make(name, c, seed):
    g = torch.Generator().manual_seed(seed)
    first = c.get("first", 0)
    N = first + sum(c["lengths"])
    wide = torch.randn(N, c["in_feats"] + c.get("pad_cols", 0), generator=g)
    x = wide[:, :c["in_feats"]]           # a column slice when pad_cols > 0 (ldx > in_feats)
    starts, s = [], first
    for n in c["lengths"]:
        starts.append(s)
        s += n
    rootindex = torch.tensor(starts, dtype=torch.int64)
    y = torch.randint(0, c["out"], (len(starts),), generator=g)
    factor = c.get("weight_factor", 1.0)
    lstm, fc = build(c["in_feats"], c["hid"], c["out"], c["layers"], torch.float64, seed, factor)
    ref = run(lstm, fc, x, rootindex, y)
    return SimpleNamespace(name=name, cfg=c, seed=seed, x=x, rootindex=rootindex, y=y, N=N, B=len(starts),
                           max_len=max(c["lengths"]), weight_factor=factor, sd=state_dict(lstm, fc), ref=ref)


@functools.lru_cache(maxsize=None)
def case(name):
    """The seeded inputs of a case and its fp64 oracle, computed once and shared (read-only)."""
    return _make(name, CASES[name], sorted(CASES).index(name) + 1)


@functools.lru_cache(maxsize=None)
def edge_case(name):
    """As case(), for EDGE_CASES and the entry's own seed."""
    c = EDGE_CASES[name]
    return _make(name, c, c["seed"])


def margin_ok(logp, gap=1e-3):
    """Trees whose fp64 top-two logit gap exceeds ``gap`` (log_softmax shifts a row by a constant)."""
    if logp.size(1) < 2:
        return torch.ones(logp.size(0), dtype=torch.bool)
    top = logp.topk(2, dim=1).values
    return (top[:, 0] - top[:, 1]) > gap
