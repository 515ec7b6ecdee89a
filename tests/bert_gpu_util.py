"""Helpers shared by the GPU tests of the TreeBERT baseline (test_gpu_bert.py, test_gpu_bert_edges.py).
A name is one of bert_ref.CASES or bert_ref.EDGE_CASES."""
import functools
from types import SimpleNamespace

import torch

import bert_ref as R

DEV = torch.device("cuda:0")
BAR = 1e-4


def _case(name):
    return R.case(name) if name in R.CASES else R.edge_case(name)


@functools.lru_cache(maxsize=None)
def _model(name):
    return R.model_for(_case(name), DEV)


@functools.lru_cache(maxsize=None)
def _inputs(name):
    c = _case(name)
    wide = c.x._base if c.x._base is not None else c.x
    x = wide.to(DEV)[:, :c.cfg["hidden"]]       # the case's row stride survives the copy
    return x, c.rootindex.to(DEV), c.y.to(DEV)


def _data(name, T=3, drop_first=False):
    """A PyG-like batch whose ``x [N, T * hidden]`` max-pools over T to the case's rows.  ``drop_first``:
    without the rows above the first tree, which a PyG batch vector cannot name."""
    c = _case(name)
    x, root, y = _inputs(name)
    if drop_first and c.first:
        d = _data(name, T)
        return SimpleNamespace(x=d.x[c.first:], rootindex=root - c.first, y=y, batch=c.batch.to(DEV))
    g = torch.Generator().manual_seed(5)
    lower = x.unsqueeze(1) - torch.rand(c.N, T - 1, c.cfg["hidden"], generator=g).to(DEV)
    wide = torch.cat((lower[:, :1], x.unsqueeze(1), lower[:, 1:]), 1).reshape(c.N, -1).contiguous()
    return SimpleNamespace(x=wide, rootindex=root, y=y, batch=c.batch.to(DEV))


def _err(got, want):
    return float((got.double().cpu() - want).abs().max())


def _parity_errors(c, logp_root, logp, hidden, hsum, asum):
    """The worst differences from the oracle that the parity tests hold to BAR."""
    ref = c.ref
    return {"logp_root_only": _err(logp_root, ref.logp), "logp_full": _err(logp, ref.logp),
            "hidden": _err(hidden, ref.hidden), "hidden_sum/hidden": _err(hsum, ref.hidden_sum) / c.cfg["hidden"],
            "attn_sum": float(((asum.double().cpu() - ref.attn_sum).abs() / ref.attn_sum.abs().clamp(min=1)).max())}


def _check_rankings(c, res):
    """``bigcn_amd.explain``'s result against the oracle: values within the bar, the order equal
    wherever the oracle's sorted values are more than 2e-4 from both neighbours."""
    assert torch.equal(res.prediction.cpu(), c.ref.pred)
    roots = [r - c.first for r in c.rootindex.tolist() + [c.N]]
    for what, order, srt, ranks, scale in (("hidden", res.hidden_order, res.hidden_sorted, c.ref.rank_hidden, c.cfg["hidden"]),
                                           ("attn", res.attn_order, res.attn_sorted, c.ref.rank_attn, None)):
        for b, (o_ref, v_ref) in enumerate(ranks):
            a, e = roots[b], roots[b + 1]
            v = srt[a:e].double().cpu()
            tol = (BAR * scale) if scale else BAR * v_ref.abs().clamp(min=1)
            assert bool(((v - v_ref).abs() <= tol).all()), (what, b)
            ok = R.rank_compared(v_ref)
            assert torch.equal(order[a:e].cpu().long()[ok], o_ref[ok]), (what, b)
    rec = res.to_reference_dict(c.B - 1)
    assert len(rec["bert_attentions_top_k"][0]) == c.cfg["lengths"][-1] and rec["prediction"] == int(c.ref.pred[-1])
