"""GPU checks of the EBGCN evaluation step (bgcn_ebgcn_eval_step, EBGCN.evaluate / validate /
check_status) against the fp64 restatement tests/ebgcn_ref.py.  Bar: the project's standing
|a - b| <= 1e-4 max|b| per tensor; predictions are compared wherever the fp64 top-2 margin exceeds
that bar."""
import argparse
import ctypes
import functools
import glob
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F_

import ebgcn_ref as R
from oracle import bigcn_oracle as O
from test_gpu_ebgcn import _randomised

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "ebgcn_*.npz")))
NAMES = [os.path.basename(p)[len("ebgcn_"):-len(".npz")] for p in FIXTURES]
DEV = "cuda:0"
TOL = 1e-4


def _close(got, want, what):
    got, want = got.double().cpu(), want.double().cpu()
    assert got.shape == want.shape, what
    if want.numel() == 0:
        return
    err, scale = float((got - want).abs().max()), float(want.abs().max())
    print(f"{what}: max err {err:.3e}, max |ref| {scale:.3e}")
    assert err <= TOL * scale, f"{what}: {err} vs {TOL} * {scale}"


def _args(F=36, K=2, td=True, bu=True, C=4):
    return argparse.Namespace(input_features=F, hidden_features=64, output_features=64, num_class=C, edge_num=K,
                              edge_infer_td=td, edge_infer_bu=bu, device=DEV)


def _margin_ok(want_logp):
    """Trees whose fp64 decision is not within the bar of a tie."""
    if want_logp.size(1) < 2:
        return torch.ones(want_logp.size(0), dtype=torch.bool)
    top = want_logp.topk(2, dim=1).values
    return (top[:, 0] - top[:, 1]) > TOL * float(want_logp.abs().max())


# ---- the fp64 restatement with the degree convention as a parameter (R.direction takes PyG's)
def _ref_direction(sd, d, x, ei, batch, rootindex, infer, degree_on, B):
    h1 = O.gcn_conv(x, ei, sd[d + ".conv1.lin.weight"], sd[d + ".conv1.bias"], degree_on=degree_on)
    pred = R.edge_pred(sd, d, h1, ei) if infer else None
    root_of_node = rootindex[batch]
    cat = torch.cat((h1, x[root_of_node]), 1)
    if cat.size(0) != 1:
        cat = R.bn_eval(cat, sd, d + ".bn1")
    cat = F_.relu(cat)
    ew = pred if pred is not None and pred.numel() else None
    h2 = F_.relu(O.gcn_conv(cat, ei, sd[d + ".conv2.lin.weight"], sd[d + ".conv2.bias"], edge_weight=ew,
                            degree_on=degree_on))
    h = torch.cat((h2, h1[root_of_node]), 1)
    out = torch.zeros(B, h.size(1), dtype=h.dtype).index_add_(0, batch, h)
    cnt = torch.bincount(batch, minlength=B).clamp(min=1).to(h.dtype)
    return out / cnt[:, None], pred


def _ref_forward(sd, b, args, degree_on="col"):
    B = int(b["rootindex"].numel())
    td, tp = _ref_direction(sd, "TDrumorGCN", b["x"], b["edge_index"], b["batch"], b["rootindex"],
                            args.edge_infer_td, degree_on, B)
    bu, bp = _ref_direction(sd, "BUrumorGCN", b["x"], b["BU_edge_index"], b["batch"], b["rootindex"],
                            args.edge_infer_bu, degree_on, B)
    z = F_.linear(torch.cat((bu, td), 1), sd["fc.weight"], sd["fc.bias"])
    return F_.log_softmax(z, dim=1), tp, bp


def _check_against(model, data, want, y, what):
    """evaluate() on `data` against the fp64 (logp, td_pred, bu_pred) `want`."""
    want_logp, want_td, want_bu = want
    B, C = want_logp.shape
    logp = torch.empty(B, C, dtype=torch.float32, device=DEV)
    loss, correct, pred = model.evaluate(data, logp=logp, pred=True)
    model.check_status()
    assert loss.shape == () and loss.dtype == torch.float32 and correct.shape == () and correct.dtype == torch.int32
    assert pred.shape == (B,) and pred.dtype == torch.int64
    _close(logp, want_logp, what + " log-probs")
    for name, got, w in (("td", model.last_edge_pred[0], want_td), ("bu", model.last_edge_pred[1], want_bu)):
        if w is None:
            assert got is None
        else:
            _close(got, w, f"{what} {name}_edge_pred")
    _close(loss.reshape(1), F_.nll_loss(want_logp, y.cpu()).reshape(1), what + " loss")
    ok = _margin_ok(want_logp)
    assert torch.equal(pred.cpu()[ok], want_logp.argmax(1)[ok]), what
    assert int(correct) == int((pred == y.to(DEV)).sum())
    assert torch.equal(pred, logp.argmax(1))        # ties go to the lowest class, as torch's max / argmax
    return logp, pred, ok


@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_fixtures_match_restatement_and_the_forward_path(path):
    from bigcn_amd import EBGCN
    from bigcn_amd.data import Batch
    sd, b, cfg, _ = R.load_fixture(path)
    sd64, b64, _, _ = R.load_fixture(path, torch.float64)
    want = R.fixture_forward(sd64, b64, cfg)
    model = EBGCN(_args(b["x"].size(1), cfg["edge_num"], bool(cfg["edge_infer_td"]), bool(cfg["edge_infer_bu"]),
                        cfg["num_class"]))
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV).train()        # evaluate() runs in eval mode whatever model.training says
    data = Batch(num_graphs=int(b["rootindex"].numel()), **b).to(DEV)
    if getattr(data, "y", None) is None:
        data.y = want[0].argmax(1).to(DEV)
    logp, pred, ok = _check_against(model, data, want, data.y, os.path.basename(path))
    assert float(ok.double().mean()) >= 0.9      # the fixtures' margins leave the decisions comparable
    old = model.eval()(data)[0]
    _close(logp, old, "against the forward path")
    assert torch.equal(pred, old.argmax(1))


def test_fixture_margins_leave_most_trees_compared():
    """On the CPU: at least 90 % of every fixture's trees have an fp64 top-2 margin above the bar."""
    for path in FIXTURES:
        sd64, b64, cfg, _ = R.load_fixture(path, torch.float64)
        ok = _margin_ok(R.fixture_forward(sd64, b64, cfg)[0])
        assert float(ok.double().mean()) >= 0.9, path


@functools.lru_cache(maxsize=None)
def _model(F, K, td, bu, C):
    from bigcn_amd import EBGCN
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(7 + F + K)
        m = _randomised(EBGCN(_args(F, K, td, bu, C)), 7 + F + K).eval()
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in m.state_dict().items()}
    return m.to(DEV), sd64


def _batch(sizes, F, C, seed=3, shuffle_edges=False, no_bu=False):
    from bigcn_amd.data import synth_batch
    rng = np.random.default_rng(seed)
    data = synth_batch(rng, sizes, F, C, 0.0, 0.0, device="cpu", root_random=True)
    data.y = torch.as_tensor(rng.integers(0, C, size=len(sizes)))
    data.x = data.x * torch.as_tensor(rng.uniform(0.5, 2.0, size=tuple(data.x.shape)), dtype=torch.float32)
    if shuffle_edges:      # edges no longer grouped by target (nor by source): the ordered general placement
        p = torch.as_tensor(rng.permutation(data.edge_index.size(1)))
        data.edge_index = data.edge_index[:, p].contiguous()
        q = torch.as_tensor(rng.permutation(data.BU_edge_index.size(1)))
        data.BU_edge_index = data.BU_edge_index[:, q].contiguous()
    if no_bu:
        data.BU_edge_index = torch.zeros(2, 0, dtype=torch.int64)
    b = {k: getattr(data, k) for k in ("x", "edge_index", "BU_edge_index", "batch", "rootindex")}
    b64 = {k: (v.double() if v.is_floating_point() else v) for k, v in b.items()}
    return data.to(DEV), b64


CASES = {
    "mixed_small_trees": dict(sizes=[1, 2, 33, 65]),
    "edge_tile_32": dict(sizes=[33]),
    "edge_tile_33": dict(sizes=[34]),
    "empty_direction": dict(sizes=[1, 2, 33, 65], no_bu=True),
    "td_infer_off": dict(sizes=[1, 2, 33, 65], td=False),
    "one_node": dict(sizes=[1]),
    "edge_num_1": dict(sizes=[1, 2, 33, 65], K=1),
    "edge_num_3": dict(sizes=[5, 40], K=3),
    "two_classes": dict(sizes=[1, 2, 33, 65], C=2),
    "degree_on_row": dict(sizes=[1, 2, 33, 65], degree_on="row"),
    "edges_not_grouped": dict(sizes=[1, 2, 33, 65], shuffle_edges=True),
    "edges_not_grouped_row": dict(sizes=[7, 300], shuffle_edges=True, degree_on="row"),
}


def _set_degree(model, degree_on):
    for d in (model.TDrumorGCN, model.BUrumorGCN):
        d.conv1.degree_on = d.conv2.degree_on = degree_on


@pytest.mark.parametrize("case", sorted(CASES))
def test_synthetic_batches_match_restatement(case):
    """F = 36 is not a multiple of 64; sizes [1, 2, 33, 65] give E_td = 97 (three edge tiles + 1)."""
    c = dict(CASES[case])
    F, K, C = 36, c.get("K", 2), c.get("C", 4)
    model, sd64 = _model(F, K, c.get("td", True), True, C)
    data, b64 = _batch(c["sizes"], F, C, shuffle_edges=c.get("shuffle_edges", False), no_bu=c.get("no_bu", False))
    degree_on = c.get("degree_on", "col")
    _set_degree(model, degree_on)
    try:
        want = _ref_forward(sd64, b64, model.args, degree_on)
        if c.get("no_bu"):
            assert want[2].numel() == 0
        logp, pred, _ = _check_against(model, data, want, data.y, case)
        _close(logp, model(data)[0], case + " against the forward path")
    finally:
        _set_degree(model, "col")


def _ws_array(model, address, count, dtype):
    ws = model._eval_state["ws"]
    off = address - ws.data_ptr()
    assert 0 <= off and off + 4 * count <= ws.numel()
    return ws[off:off + 4 * count].view(dtype)


@pytest.mark.parametrize("degree_on", ["col", "row"])
@pytest.mark.parametrize("shuffle", [False, True])
def test_reweighted_values_against_the_weighted_build(degree_on, shuffle):
    from bigcn_amd import _lib
    from bigcn_amd.ops import build_graph
    F, K, C = 36, 2, 4
    model, _ = _model(F, K, True, True, C)
    data, _ = _batch([1, 2, 33, 65, 300], F, C, seed=11, shuffle_edges=shuffle)
    _set_degree(model, degree_on)
    try:
        model.evaluate(data)
        model.check_status()
    finally:
        _set_degree(model, "col")
    N, B = data.x.size(0), data.num_graphs
    ws = model._eval_state["ws"]
    for d, ei in enumerate((data.edge_index, data.BU_edge_index)):
        E = ei.size(1)
        v = _lib.EbgcnEvalView()
        _lib.check(_lib.lib().bgcn_ebgcn_eval_saved(ws.data_ptr(), ws.numel(), N, B, F, data.edge_index.size(1),
                                                     data.BU_edge_index.size(1), K, d, ctypes.byref(v)))
        g = build_graph(ei, N, edge_weight=model.last_edge_pred[d], degree_on=degree_on, validate=True)
        t_ptr = _ws_array(model, v.t_ptr, N + 1, torch.int32)
        assert torch.equal(t_ptr, g.t_ptr)
        nnz = int(t_ptr[N])
        assert nnz == E + N
        assert torch.equal(_ws_array(model, v.t_col, E + N, torch.int32)[:nnz], g.t_col[:nnz])
        _close(_ws_array(model, v.t_w2, E + N, torch.float32)[:nnz], g.t_w[:nnz], f"t_w2 dir {d}")
        # each edge's recorded slot holds that edge
        slot = _ws_array(model, v.slot, E, torch.int32).long()
        assert torch.equal(g.t_col[slot].long(), ei[0]) and torch.equal(g.t_row[slot].long(), ei[1])


def test_two_calls_are_bitwise_equal():
    model, _ = _model(36, 2, True, True, 4)
    data, _ = _batch([1, 2, 33, 65, 300], 36, 4, seed=11, shuffle_edges=True)
    outs = []
    for _ in range(2):
        logp = torch.empty(data.num_graphs, 4, dtype=torch.float32, device=DEV)
        loss, correct, pred = model.evaluate(data, logp=logp, pred=True)
        outs.append((logp, loss.clone(), correct.clone(), pred, model.last_edge_pred))
    a, b = outs
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    assert torch.equal(a[4][0], b[4][0]) and torch.equal(a[4][1], b[4][1])


def test_unsorted_batch_vector_takes_the_general_readout():
    from bigcn_amd import _lib
    from bigcn_amd.data import Batch
    model, _ = _model(36, 2, True, True, 4)
    data, _ = _batch([3, 20, 9], 36, 4, seed=5)
    # renumber the nodes by a permutation: the same trees, a batch vector that is not sorted
    N = data.x.size(0)
    perm = torch.as_tensor(np.random.default_rng(1).permutation(N), device=DEV)     # old id -> new id
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(N, device=DEV)
    mixed = Batch(**{k: v for k, v in data.__dict__.items() if not k.startswith("_")})
    mixed.x, mixed.batch = data.x[inv].contiguous(), data.batch[inv].contiguous()
    mixed.edge_index, mixed.BU_edge_index, mixed.rootindex = perm[data.edge_index], perm[data.BU_edge_index], perm[data.rootindex]
    assert not bool((mixed.batch[1:] >= mixed.batch[:-1]).all())
    logp = torch.empty(3, 4, dtype=torch.float32, device=DEV)
    model.evaluate(mixed, logp=logp)
    assert int(model._eval_state["status"].item()) == _lib.BGCN_STATUS_BATCH_UNSORTED
    model.check_status()           # information only: nothing to raise
    # edge_infer reads rows "one lower than the list says" (id - 1): renumbering changes which rows an
    # edge reads, so the comparison is against the forward path on the SAME renumbered batch
    _close(logp, model(mixed)[0], "unsorted batch against the forward path")


def test_invalid_indices_are_flagged_and_leave_the_next_batch_alone():
    model, _ = _model(36, 2, True, True, 4)
    good, _ = _batch([1, 2, 33, 65], 36, 4)
    logp0 = torch.empty(4, 4, dtype=torch.float32, device=DEV)
    loss0, _, pred0 = model.evaluate(good, logp=logp0, pred=True)
    loss0 = loss0.clone()
    model.check_status()
    N = good.x.size(0)
    for field, pos in (("rootindex", (2,)), ("edge_index", (1, 40)), ("BU_edge_index", (0, 7))):
        bad, _ = _batch([1, 2, 33, 65], 36, 4)
        t = getattr(bad, field).clone()
        t[pos] = N if field != "BU_edge_index" else -1
        setattr(bad, field, t)
        logp = torch.empty(4, 4, dtype=torch.float32, device=DEV)
        loss, correct, pred = model.evaluate(bad, logp=logp, pred=True)
        assert bool(torch.isfinite(logp).all()) and bool(torch.isfinite(loss))
        assert all(bool(torch.isfinite(p).all()) for p in model.last_edge_pred)
        with pytest.raises(IndexError):
            model.check_status()
        model.check_status()       # reported once
    logp1 = torch.empty(4, 4, dtype=torch.float32, device=DEV)
    loss1, _, pred1 = model.evaluate(good, logp=logp1, pred=True)
    model.check_status()
    assert torch.equal(logp0, logp1) and torch.equal(loss0, loss1) and torch.equal(pred0, pred1)


def test_validate_is_the_manual_loop_and_does_not_sync():
    from bigcn_amd import EpochMetrics, evaluation4class
    from bigcn_amd.metrics import class_metrics
    model, _ = _model(36, 2, True, True, 4)
    batches = [_batch(sizes, 36, 4, seed=20 + k)[0] for k, sizes in enumerate(([3, 5, 2], [1, 4, 6, 2, 3], [7, 2]))]
    manual = []
    for b in batches:
        loss, correct, pred = model.evaluate(b, pred=True)
        manual.append((loss.clone(), correct.clone(), pred.clone()))
    torch.cuda.synchronize()
    model.check_status()
    try:
        torch.cuda.set_sync_debug_mode("error")
        sync_checked = True
    except Exception:       # this torch build has no such mode: the loop still runs, unchecked
        sync_checked = False
    try:
        m = model.validate(batches)                      # a host sync in here raises
        m2 = EpochMetrics(4, 3, DEV)
        assert model.validate(batches[:2], m2) is m2
        model.validate(batches[2:], m2)                  # records are appended
        if sync_checked:
            with pytest.raises(RuntimeError):
                m.status.item()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    print("sync debug mode checked:", sync_checked)
    model.check_status()
    preds = torch.cat([p for _, _, p in manual]).cpu().tolist()
    ys = torch.cat([b.y for b in batches]).cpu().tolist()
    tuples = [evaluation4class(p.cpu().tolist(), b.y.cpu().tolist()) for (_, _, p), b in zip(manual, batches)]
    for res in (m.result(), m2.result()):
        for k, (loss, correct, pred) in enumerate(manual):
            assert res.losses[k] == float(loss) and res.correct[k] == int(correct)
            assert res.sizes[k] == batches[k].num_graphs
        assert res.batch_metrics == tuples
        assert res.metrics == tuple(float(np.mean([t[j] for t in tuples])) for j in range(17))
        # the whole epoch's confusion matrix gives evaluation4class of the gathered predictions
        conf = np.zeros((4, 4), dtype=np.int64)
        for p, y in zip(preds, ys):
            conf[y, p] += 1
        assert np.array_equal(res.confusion, conf)
        assert class_metrics(res.confusion, 4) == evaluation4class(preds, ys)
