"""GPU checks of the explain path: the ranking kernel against the ordering rule (exact), the
stage-sum kernels against the fp64 restatement (tests/explain_ref.py, itself pinned to
reference-produced fixtures by tests/test_explain.py), and explain() end to end on the fixtures.

Value bar (explain_ref.VALUE_BAR): ten times the error of the fp32 CPU restatement against its own
fp64 run on the same inputs - measured 3.84e-6 / 8.43e-6 / 4.51e-5 on the synthetic inputs with
F = 4 / 68 / 772 and 6.36e-6 on the fixtures, so the HIP path is allowed 3.84e-5 / 8.43e-5 /
4.51e-4 and 6.36e-5."""
import argparse
import functools
import glob
import json
import os

import numpy as np
import pytest
import torch

import explain_ref as X

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "explain_*.npz")))
NAMES = [os.path.basename(p)[len("explain_"):-len(".npz")] for p in FIXTURES]
DEV = "cuda:0"
TOL = 1e-4      # the project's standing relative bar (gcn_output, log_probs)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------ segment_rank
def _rank_lengths():
    from bigcn_amd.ops import SEGMENT_RANK_LDS
    return [1, 2, 3, 63, 64, 65, 0, 127, 129, SEGMENT_RANK_LDS, SEGMENT_RANK_LDS + 1]   # 0: a tree id without nodes


def _pattern(kind, n, rng):
    if kind == "small_ints":
        return rng.integers(-3, 4, size=n).astype(np.float32)
    if kind == "all_equal":
        return np.full(n, 2.5, dtype=np.float32)
    if kind == "ascending":
        return np.arange(n, dtype=np.float32) * 0.5 - 7
    if kind == "descending":
        return -np.arange(n, dtype=np.float32)
    if kind == "zeros":
        return rng.choice(np.array([0.0, -0.0, 1.0, -1.0], dtype=np.float32), size=n)
    if kind == "specials":
        v = rng.integers(-2, 3, size=n).astype(np.float32)
        v[rng.random(n) < 0.1] = np.inf
        v[rng.random(n) < 0.1] = -np.inf
        v[rng.random(n) < 0.1] = np.nan
        v[rng.random(n) < 0.1] = -0.0
        return v
    return rng.standard_normal(n).astype(np.float32)


PATTERNS = ("small_ints", "all_equal", "ascending", "descending", "zeros", "specials", "normal")


@functools.lru_cache(maxsize=None)
def _rank_case(S):
    """values [S, N] inside a wider [S, N + 5] array (a non-trivial ld), batch, B, the rule's answer."""
    rng = np.random.default_rng(S)
    lengths = _rank_lengths()
    N, B = sum(lengths), len(lengths)
    batch = np.repeat(np.arange(B), lengths)
    kinds = ("specials",) if S == 1 else PATTERNS[:S]
    base = np.full((S, N + 5), np.nan, dtype=np.float32)
    for s, kind in enumerate(kinds):
        base[s, :N] = np.concatenate([_pattern(kind, n, rng) for n in lengths])
    want = X.segment_rank(base[:, :N], batch, B)
    return base, batch, B, N, want


@pytest.mark.parametrize("S", [1, 7])
def test_segment_rank_is_the_rule_exactly(S):
    from bigcn_amd import segment_rank
    base, batch, B, N, (want_order, want_sorted) = _rank_case(S)
    vals = torch.from_numpy(base).to(DEV)[:, :N]
    assert vals.stride(0) == N + 5
    bt = torch.from_numpy(batch).to(DEV)
    order, srt = segment_rank(vals, bt, B)
    assert order.dtype == torch.int32 and srt.dtype == torch.float32 and order.shape == srt.shape == (S, N)
    assert np.array_equal(order.cpu().numpy(), want_order)
    assert np.array_equal(_bits(srt.cpu().numpy()), _bits(want_sorted))      # bit-equal, NaN and -0.0 included
    order2, srt2 = segment_rank(vals, bt, B)
    assert torch.equal(order, order2) and torch.equal(srt.view(torch.int32), srt2.view(torch.int32))


def test_segment_rank_edge_cases():
    from bigcn_amd import segment_rank
    empty = torch.zeros(1, 0, device=DEV)
    order, srt = segment_rank(empty, torch.zeros(0, dtype=torch.int64, device=DEV), 0)
    assert order.shape == srt.shape == (1, 0)
    v = np.random.default_rng(5).integers(0, 6, size=100).astype(np.float32)      # B = 1, a 1-D input
    order, srt = segment_rank(torch.from_numpy(v).to(DEV), torch.zeros(100, dtype=torch.int64, device=DEV), 1)
    assert order[0].cpu().tolist() == X.rank_segment(v).tolist()
    assert np.array_equal(srt[0].cpu().numpy(), v[X.rank_segment(v)])


def test_segment_rank_refuses_a_decreasing_batch():
    """Bad input is refused, not a fault: the kernels read and write nothing outside their arrays
    (the sort does not run at all once the bounds kernel has flagged the batch vector)."""
    from bigcn_amd import segment_rank
    v = torch.arange(8, dtype=torch.float32, device=DEV).view(1, 8)
    for bad in ([0, 0, 1, 1, 0, 1, 1, 1], [0, 0, 0, 1, 1, 1, 1, 2], [0, 0, 0, -1, 1, 1, 1, 1]):   # step down; id >= B; id < 0
        with pytest.raises(IndexError):
            segment_rank(v, torch.tensor(bad, device=DEV), 2)
    order, _ = segment_rank(v, torch.tensor([0, 0, 0, 1, 1, 1, 1, 1], device=DEV), 2)   # and still works after
    assert order[0].cpu().tolist() == [2, 1, 0, 4, 3, 2, 1, 0]


# ------------------------------------------------------------------ explain_sums
def _bn_module(bn, F_in):
    if bn is None:
        return None
    m = torch.nn.BatchNorm1d(64 + F_in)
    m.load_state_dict({k[len("bn1."):]: v.float() for k, v in bn[0].items()}, strict=False)
    return m.eval().to(DEV)


@pytest.mark.parametrize("F_in,trees,with_bn", X.sums_cases())
def test_explain_sums_matches_restatement(F_in, trees, with_bn):
    from bigcn_amd import ops
    h1, h2, x, batch, rootindex, bn = X.sums_case(F_in, X.SUMS_TREES[trees], with_bn, torch.float64)
    want = X.sums_from(h1, h2, x, batch, rootindex, bn)
    args = [t.float().to(DEV) for t in (h1, h2, x)] + [batch.to(DEV), rootindex.to(DEV)]
    sums, x_sum = ops.explain_sums(*args, _bn_module(bn, F_in), validate=True)
    assert sums.shape == want.shape == (6 if with_bn else 5, h1.size(0)) and sums.dtype == torch.float32
    err = float((sums.double().cpu() - want).abs().max())
    err_x = float((x_sum.double().cpu() - x.sum(-1)).abs().max())
    print(f"F={F_in} {trees} bn={with_bn}: sums err {err:.3e}, x_sum err {err_x:.3e}, bar {X.VALUE_BAR[F_in]:.3e}")
    assert err <= X.VALUE_BAR[F_in] and err_x <= X.VALUE_BAR[F_in]
    sums2, x_sum2 = ops.explain_sums(*args, _bn_module(bn, F_in))
    assert torch.equal(sums.view(torch.int32), sums2.view(torch.int32)) and torch.equal(x_sum, x_sum2)
    sums3, none = ops.explain_sums(*args, _bn_module(bn, F_in), want_x_sum=False)
    assert none is None and torch.equal(sums, sums3)


@pytest.mark.parametrize("with_bn", [False, True])
def test_explain_sums_flags_a_root_out_of_range(with_bn):
    """An out-of-range rootindex is never read: its tree's root terms are zero and status is set."""
    from bigcn_amd import ops
    h1, h2, x, batch, rootindex, bn = X.sums_case(68, X.SUMS_TREES["ragged"], with_bn, torch.float32)
    N = h1.size(0)
    rootindex = rootindex.clone()
    rootindex[2] = N + 5
    args = [t.to(DEV) for t in (h1, h2, x, batch, rootindex)]
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    sums, _ = ops.explain_sums(*args, _bn_module(bn, 68), status=status)
    assert int(status.item()) == 1
    in_tree = (batch == 2).to(DEV)
    assert torch.equal(sums[1][in_tree], sums[0][in_tree])            # sum h1[n] + 0
    assert not torch.equal(sums[1][~in_tree], sums[0][~in_tree])
    with pytest.raises(IndexError):
        ops.explain_sums(*args, _bn_module(bn, 68), validate=True)
    args[3] = torch.where(batch == 3, 9, batch).to(DEV)               # a tree id outside [0, B)
    with pytest.raises(IndexError):
        ops.explain_sums(args[0], args[1], args[2], args[3], X.sums_case(68, X.SUMS_TREES["ragged"], with_bn)[4].to(DEV),
                         _bn_module(bn, 68), validate=True)


# ------------------------------------------------------------------ explain(), end to end
def _model_and_batch(path):
    from bigcn_amd import EBGCN, BiGCN
    from bigcn_amd.data import Batch
    sd, b, cfg, exp = X.load_fixture(path)
    F_in = b["x"].size(1)
    if cfg["ebgcn"]:
        model = EBGCN(argparse.Namespace(input_features=F_in, hidden_features=64, output_features=64,
                                         num_class=cfg["num_class"], edge_num=cfg["edge_num"], edge_infer_td=True,
                                         edge_infer_bu=True, device=DEV))
    else:
        model = BiGCN(F_in, 64, 64, DEV)
    model.load_state_dict(sd, strict=True)
    data = Batch(num_graphs=len(b["rootindex"]), **b).to(DEV)
    return model.eval().to(DEV), data, b, cfg, exp


@functools.lru_cache(maxsize=None)
def _oracle(path):
    """The fp64 restatement of a fixture, computed once."""
    sd, b, cfg, _ = X.load_fixture(path, torch.float64)
    out = {d: X.direction(sd, prefix, b["x"], b[ek], b["batch"], b["rootindex"], bool(cfg["ebgcn"]))[:3]
           for d, prefix, ek in (("td", "TDrumorGCN", "edge_index"), ("bu", "BUrumorGCN", "BU_edge_index"))}
    out["logp"] = X.log_probs(sd, b, cfg)
    return out


def _rel_close(got, want, what):
    got, want = got.double().cpu(), want.double().cpu()
    err, scale = float((got - want).abs().max()), float(want.abs().max())
    print(f"{what}: max err {err:.3e}, max |ref| {scale:.3e}")
    assert got.shape == want.shape and err <= TOL * scale, what


@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_explain_on_reference_fixtures(path):
    from bigcn_amd import explain
    model, data, b, cfg, exp = _model_and_batch(path)
    want = _oracle(path)
    ex = explain(model, data)
    batch, B = b["batch"].numpy(), len(b["rootindex"])
    bar = X.VALUE_BAR["fixtures"]
    for d, res in (("td", ex.td), ("bu", ex.bu)):
        names, sums64, gcn64 = want[d]
        assert res.stage_names == names
        err = float((res.sums.double().cpu() - sums64).abs().max())
        print(f"{d} sums: max err {err:.3e} (bar {bar:.3e})")
        assert err <= bar
        # the order is the rule's stable sort of the sums RETURNED: no tolerance
        got_sums = res.sums.cpu().numpy()
        rule_order, rule_sorted = X.segment_rank(got_sums, batch, B)
        assert np.array_equal(res.order.cpu().numpy(), rule_order)
        assert np.array_equal(_bits(res.sorted.cpu().numpy()), _bits(rule_sorted))
        if B == 1:      # the reference's whole-batch topk is this tree's ranking
            for s, n in enumerate(names):
                assert res.order[s].cpu().tolist() == exp[f"{d}/{n}_topk/indices"].tolist(), (d, n)
        _rel_close(res.gcn_output, gcn64, d + " gcn_output")
        _rel_close(res.gcn_output, torch.from_numpy(exp[f"{d}/gcn_output"]), d + " gcn_output vs reference")
    _rel_close(ex.log_probs, want["logp"], "log_probs")
    assert ex.prediction.cpu().tolist() == exp["logp"].argmax(1).tolist()
    x_sum = b["x"].sum(-1).numpy()
    assert np.array_equal(ex.x_sum.cpu().numpy(), x_sum)                 # small integer counts: exact
    xo, xs = X.segment_rank(x_sum[None], batch, B)
    assert np.array_equal(ex.x_order.cpu().numpy(), xo[0]) and np.array_equal(ex.x_sorted.cpu().numpy(), xs[0])
    p = X.tree_ptr(batch, B)
    for t in range(B):
        rec = ex.to_reference_dict(t)
        assert json.loads(json.dumps(rec)) == rec
        assert rec["rootindex"] == int(b["rootindex"][t]) - p[t] and len(rec["x_sum_top_k"][0]) == p[t + 1] - p[t]
        assert set(rec["td_gcn_explanations"]) == {n + "_topk" for n in ex.td.stage_names} | {"gcn_output"}
    model.train()
    with pytest.raises(ValueError):
        explain(model, data)


def _tree_alone(b, t, p):
    from bigcn_amd.data import Batch
    a, e = int(p[t]), int(p[t + 1])
    keep = (b["edge_index"][0] >= a) & (b["edge_index"][0] < e)
    return Batch(x=b["x"][a:e], edge_index=b["edge_index"][:, keep] - a, BU_edge_index=b["BU_edge_index"][:, keep] - a,
                 batch=torch.zeros(e - a, dtype=torch.int64), rootindex=b["rootindex"][t:t + 1] - a, num_graphs=1).to(DEV)


@pytest.mark.parametrize("path", [p for p in FIXTURES if p.endswith("_mixed.npz")], ids=["bigcn_mixed", "ebgcn_mixed"])
def test_batched_explain_is_the_batch_of_one_form(path):
    """explain() on a multi-tree batch equals, tree by tree, explain() on each tree alone - the
    form the reference runs.  Ranks exactly, sums within the value bar.  EBGCN runs with
    batch_of_one=True: the reference's edge_infer reads node id - 1 and wraps id 0 to the LAST node
    of whatever batch it is given, so without it an edge at a tree's first node reads the previous
    tree (that default is what test_explain_on_reference_fixtures checks against the reference's
    own run on the whole batch)."""
    from bigcn_amd import explain
    model, data, b, cfg, _ = _model_and_batch(path)
    B = len(b["rootindex"])
    p = X.tree_ptr(b["batch"].numpy(), B)
    whole = explain(model, data, batch_of_one=True)
    bar = X.VALUE_BAR["fixtures"]
    for t in range(B):
        alone = explain(model, _tree_alone(b, t, p), batch_of_one=True)
        a, e = int(p[t]), int(p[t + 1])
        for w, o in ((whole.td, alone.td), (whole.bu, alone.bu)):
            assert torch.equal(w.order[:, a:e], o.order), t
            assert float((w.sums[:, a:e] - o.sums).abs().max()) <= bar, t
            assert float((w.gcn_output[t] - o.gcn_output[0]).abs().max()) <= TOL * float(o.gcn_output.abs().max())
        assert torch.equal(whole.x_order[a:e], alone.x_order)
