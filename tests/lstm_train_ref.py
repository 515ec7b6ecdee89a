"""The reference's LSTM training loop body restated with autograd (model/Twitter/LSTM_Twitter.py:96-126):
one unbatched ``nn.LSTM`` call per tree, ``log_softmax(fc(h_n))``, ``F.nll_loss``, ``backward`` and
``torch.optim.Adam`` - in fp64 (the oracle) or fp32 (the reference's own arithmetic).  Shared by
tests/test_lstm_train.py and tests/test_gpu_lstm_train.py, with the training cases beyond
``lstm_ref.CASES`` (their own table and seeds; ``lstm_ref`` is not touched).

Error metric of a gradient tensor: ``max|got - ref| / max|ref|``.  These gradients peak between 2e-4
and 0.7, so the project's absolute 1e-4 would pass a half-wrong one; the bar is 1e-4 in this metric
(loss and logp: 1e-4 absolute)."""
import functools
from types import SimpleNamespace

import torch
import torch.nn.functional as F

import lstm_ref as R

BAR = 1e-4
LR, WEIGHT_DECAY = 5e-4, 1e-4   # the reference's optimiser (LSTM_Twitter.py)

# The smallest shapes that reach each code path of bgcn_lstm_train_grad.
TRAIN_CASES = {
    # B = 300 > 256: the second pass of every loop over B; 10 sequence tiles
    "t_many_trees": dict(in_feats=8, hid=64, layers=1, out=4, lengths=[1 + b % 3 for b in range(300)], seed=201),
    # two and four iterations of the backward step's reduction loop (a wave covers H of the 4H terms)
    "t_hid_128": dict(in_feats=12, hid=128, layers=2, out=5, lengths=[1, 5, 18, 2], seed=202),
    "t_hid_256": dict(in_feats=12, hid=256, layers=1, out=3, lengths=[1, 7, 3], seed=203),
    # the largest head: 2 L H = 8192
    "t_largest": dict(in_feats=4, hid=1024, layers=4, out=3, lengths=[2, 1, 3], seed=204),
    "t_one_class": dict(in_feats=8, hid=64, layers=1, out=1, lengths=[1, 4, 2], seed=205),
    "t_classes_63": dict(in_feats=8, hid=64, layers=1, out=63, lengths=[1, 4, 2], seed=206),
    # N = 8217 >= 8192 rows: the input GEMMs take the six-product kernel, and the weight-gradient GEMMs
    # reduce over 8217 rows in several splits
    "t_rows_over_switch": dict(in_feats=20, hid=64, layers=2, out=4,
                               lengths=[1 + (37 * b) % 129 for b in range(126)], seed=207),
}
PARITY_CASES = sorted(R.CASES) + sorted(TRAIN_CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    """The seeded inputs of a case (``lstm_ref.case`` for its names, else TRAIN_CASES under the entry's seed)."""
    if name in R.CASES:
        return R.case(name)
    c = TRAIN_CASES[name]
    return R._make(name, c, c["seed"])


def _trees(c):
    roots = [int(v) for v in c.rootindex.tolist()]
    return list(zip(roots, roots[1:] + [c.N]))


def _loop(lstm, fc, x, spans, y):
    """LSTM_Twitter.py:103-112: one nn.LSTM call per tree, the rows concatenated, nll_loss."""
    H, L = lstm.hidden_size, lstm.num_layers
    rows = []
    for s, e in spans:
        _, (hn, _) = lstm(x[s:e])
        rows.append(F.log_softmax(fc(hn.reshape(-1, H * L * 2)), dim=1))
    logp = torch.cat(rows)
    return logp, F.nll_loss(logp, y)


def names(layers):
    """The state_dict names."""
    out = []
    for l in range(layers):
        for rev in ("", "_reverse"):
            out += [f"lstm.weight_ih_l{l}{rev}", f"lstm.weight_hh_l{l}{rev}"]
    return out + ["fc.weight", "fc.bias"]


def _build(c, dtype):
    lstm, fc = R.build(c.cfg["in_feats"], c.cfg["hid"], c.cfg["out"], c.cfg["layers"], dtype, c.seed, c.weight_factor)
    params = {"lstm." + k: p for k, p in lstm.named_parameters()}
    params.update({"fc." + k: p for k, p in fc.named_parameters()})
    return lstm, fc, params


def grads_of(c, dtype=torch.float64):
    """loss, logp and the loss's gradient for every parameter (by state_dict name) and for ``x``."""
    lstm, fc, params = _build(c, dtype)
    x = c.x.to(dtype).clone().requires_grad_(True)
    logp, loss = _loop(lstm, fc, x, _trees(c), c.y)
    loss.backward()
    g = {k: p.grad.detach().clone() for k, p in params.items()}
    g["x"] = x.grad.detach().clone()
    return SimpleNamespace(loss=loss.detach(), logp=logp.detach(), grads=g)


@functools.lru_cache(maxsize=None)
def oracle(name):
    """The fp64 loop body of a case: computed once and shared (read-only)."""
    return grads_of(case(name), torch.float64)


def train_losses(c, steps, dtype=torch.float64):
    """The losses of ``steps`` iterations of the reference loop on the same batch with the reference's Adam."""
    lstm, fc, params = _build(c, dtype)
    opt = torch.optim.Adam(list(lstm.parameters()) + list(fc.parameters()), lr=LR, weight_decay=WEIGHT_DECAY)
    x = c.x.to(dtype)
    out = []
    for _ in range(steps):
        opt.zero_grad()
        _, loss = _loop(lstm, fc, x, _trees(c), c.y)
        loss.backward()
        opt.step()
        out.append(float(loss.detach()))
    return out


def rel_err(got, ref):
    """max|got - ref| / max|ref|; an all-zero reference (one class: dz = 0) demands exact zeros."""
    got, ref = got.detach().double().cpu(), ref.double()
    top = float(ref.abs().max())
    diff = float((got - ref).abs().max())
    if top == 0.0:
        return 0.0 if diff == 0.0 else float("inf")
    return diff / top
