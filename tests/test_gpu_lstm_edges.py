"""Edge-shape, workspace and invariance checks of the LSTM baseline (bgcn_lstm_eval, bigcn_amd.LSTM)
beside tests/test_gpu_lstm.py: the cases of ``lstm_ref.EDGE_CASES`` against the fp64 oracle, and
properties that hold bit for bit by construction.

a. Parity: ``out``, ``h_n`` and ``logp`` within 1e-4 absolute of the fp64 loop (the project's bar;
   test_lstm.py::test_the_bar_is_feasible shows torch's own fp32 at <= 1e-5 on these cases).  With
   BGCN_LSTM_PARITY_OUT set, this file's records go to that path in the format of
   profiles/lstm_parity.json (profiles/lstm_parity_edges.json is such a record; run this file alone
   to write it).
b. The argmax's "first maximal class" with two bitwise-equal logits.
c. Nothing read from the workspace or the outputs before it is written: a call on a workspace of
   NaN bits or of 3e38 gives the bits of a call on a zeroed one.
d. The optional outputs of include/bgcn.h.
e. Exact invariances.  The step's MFMA columns (trees) and the GEMM's rows are computed
   independently of their neighbours, every sum has a fixed order and nothing is accumulated with
   float atomics, so a tree's bits do not depend on which other trees share its batch, on its
   position in it, or on how many step launches follow its last one.
f. Validity decided on the device, with faults at tree indices past 256 (the setup's and the
   finish's loops over B take steps of 256).  None of these inputs reads or writes out of bounds:
   the header promises that a flagged batch is emptied.
"""
import ctypes
import functools
import json
import os
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import lstm_ref as R
import lstm_gpu_util as U
from lstm_gpu_util import DEV, _buf, _data, _ends, _x

pytestmark = pytest.mark.gpu

TOL = 1e-4
_parity = {}


def _case(name):
    return R.case(name) if name in R.CASES else R.edge_case(name)


def _new_model(name, sd=None):
    return U._new_model(_case(name), sd)


@functools.lru_cache(maxsize=None)
def _model(name):
    return _new_model(name)


def _err(got, want):
    return float((got.double().cpu() - want).abs().max())


# ---------------------------------------------------------------- a. parity
@pytest.mark.parametrize("name", sorted(R.EDGE_CASES))
def test_parity_with_the_fp64_oracle(name):
    """rows_over_switch: N = 8217 is at or above kX6MinRows = 8192 (bgcn_internal.h), so both layers'
    input GEMMs (Nc = 8H = 512; K = 20, then K = 2H = 128) run on the six-product kernel."""
    c = R.edge_case(name)
    m = _new_model(name)   # not kept: "largest" holds about 340 MB of weights
    x = _x(c)
    logp, out, h_n = m.forward_batch(x, c.rootindex.to(DEV), max_len=c.max_len, return_states=True)
    m.check_status()
    errs = {"out": _err(out, c.ref.out), "h_n": _err(h_n, c.ref.h_n), "logp": _err(logp, c.ref.logp)}
    print(name, {k: f"{v:.3e}" for k, v in errs.items()})
    _parity[name] = {"N": c.N, "B": c.B, "in_feats": c.cfg["in_feats"], "hid": c.cfg["hid"],
                     "layers": c.cfg["layers"], "out_feats": c.cfg["out"], "weight_factor": c.weight_factor,
                     "max_abs_err": errs, "bar": TOL, "margin": TOL / max(max(errs.values()), 1e-30)}
    path = os.environ.get("BGCN_LSTM_PARITY_OUT")
    if path:
        with open(path, "w") as f:
            json.dump(_parity, f, indent=1, sort_keys=True)
    for what, e in errs.items():
        assert e <= TOL, (what, e)
    if name == "many_trees":
        assert c.B == 300 > 256
    if name == "rows_over_switch":
        assert c.N >= 8192
    if name == "largest":
        assert h_n.shape == (8, 3, 1024) and c.cfg["in_feats"] == 4
    if name == "offset_many":
        assert int(c.rootindex[0]) == 5 and c.B > R.SEQ_TILE
        assert float(out[:5].abs().sum()) == 0.0
    if name == "one_class":
        loss, correct, pred = m.evaluate(_data(c), pred=True, max_len=c.max_len)
        m.check_status()
        assert logp.shape == (3, 1) and bool((logp == 0.0).all())
        assert bool((pred == 0).all()) and float(loss) == 0.0 and int(correct) == 3


@pytest.mark.parametrize("name", ["many_trees", "rows_over_switch", "classes_63"])
def test_evaluate_is_the_reference_loop(name):
    c = R.edge_case(name)
    m = _new_model(name)
    loss, correct, pred = m.evaluate(_data(c), pred=True, max_len=c.max_len)
    m.check_status()
    want_loss = float(F.nll_loss(c.ref.logp, c.y))
    print(name, "loss", float(loss), "oracle", want_loss)
    assert abs(float(loss) - want_loss) <= TOL
    ok = R.margin_ok(c.ref.logp)
    assert float(ok.float().mean()) >= 0.9
    assert torch.equal(pred.cpu()[ok], c.ref.pred[ok])
    assert int(correct) == int(pred.cpu().eq(c.y).sum())
    if bool(ok.all()):
        assert int(correct) == c.ref.correct


# ---------------------------------------------------------------- b. a real tie
def test_argmax_takes_the_first_of_two_equal_classes():
    """Classes 1 and 3 get the same fc row and bias, so their logits come from the same arithmetic (each
    class is one wave's fixed-order sum) and are bitwise equal; + 50 on both biases puts them on top.
    torch's max returns the first maximal index: 1."""
    c = R.case("boundaries")
    sd = {k: v.clone() for k, v in c.sd.items()}
    sd["fc.weight"][3] = sd["fc.weight"][1]
    sd["fc.bias"][3] = sd["fc.bias"][1]
    sd["fc.bias"][1] += 50.0
    sd["fc.bias"][3] += 50.0
    m = _new_model("boundaries", sd)
    logp = torch.empty(c.B, 4, device=DEV)
    loss, correct, pred = m.evaluate(_data(c), logp=logp, pred=True, max_len=c.max_len)
    m.check_status()
    assert torch.equal(logp[:, 1], logp[:, 3])
    assert bool((logp[:, 1] > logp[:, 0]).all()) and bool((logp[:, 1] > logp[:, 2]).all())
    assert pred.tolist() == [1] * c.B
    assert int(correct) == int(c.y.eq(1).sum())


# ---------------------------------------------------------------- the C ABI, called directly
OUTPUTS = ("out", "h_n", "loss", "correct", "pred")


def _capi(name, fill="zero", want=OUTPUTS, labels=True, rootindex=None, max_len=None, out_shift=0):
    """One bgcn_lstm_eval call on the case, on a workspace of the call's own and outputs all pre-filled
    with ``fill``.  ``want``: the optional outputs passed (the others are NULL); ``out_shift``: floats
    between ``out`` and the start of its allocation.  Returns host copies and the status word."""
    from bigcn_amd import _lib
    lib = _lib.lib()
    c = _case(name)
    w = U._weights(name, _case)
    H, L, C, N, B = c.cfg["hid"], c.cfg["layers"], c.cfg["out"], c.N, c.B
    x = _x(c)
    root = (c.rootindex if rootindex is None else rootindex).to(DEV)
    y = c.y.to(DEV)
    need = lib.bgcn_lstm_workspace_size(N, B, c.cfg["in_feats"], H, L)
    assert need > 0
    ws = _buf(need, fill)
    bufs = {"logp": _buf(4 * B * C, fill), "status": _buf(4, fill), "out": _buf(4 * (N * 2 * H + out_shift), fill),
            "h_n": _buf(4 * 2 * L * B * H, fill), "loss": _buf(4, fill), "correct": _buf(4, fill),
            "pred": _buf(8 * B, fill)}
    a = _lib.LstmArgs()
    U._fwd_args(a, c, w, x, root, max_len)
    a.y = y.data_ptr() if labels else None
    a.logp, a.status = bufs["logp"].data_ptr(), bufs["status"].data_ptr()
    for k in OUTPUTS:
        setattr(a, k, bufs[k].data_ptr() + (4 * out_shift if k == "out" else 0) if k in want else None)
    rc = lib.bgcn_lstm_eval(ctypes.addressof(a), ws.data_ptr(), ws.numel(), _lib.stream_handle())
    assert rc == 0, lib.bgcn_last_error()
    torch.cuda.synchronize()
    f32 = {k: bufs[k].view(torch.float32) for k in ("logp", "out", "h_n", "loss")}
    r = SimpleNamespace(status=int(bufs["status"].view(torch.int32)[0]), out_ptr=a.out,
                        logp=f32["logp"][:B * C].view(B, C).cpu(), out=None, h_n=None, loss=None, correct=None, pred=None)
    if "out" in want:
        r.out = f32["out"][out_shift:out_shift + N * 2 * H].view(N, 2 * H).cpu()
    if "h_n" in want:
        r.h_n = f32["h_n"][:2 * L * B * H].view(2 * L, B, H).cpu()
    if "loss" in want:
        r.loss = f32["loss"][:1].cpu()
    if "correct" in want:
        r.correct = bufs["correct"].view(torch.int32)[:1].cpu()
    if "pred" in want:
        r.pred = bufs["pred"].view(torch.int64)[:B].cpu()
    return r


def _same(got, want, fields):
    for k in fields:
        assert torch.equal(getattr(got, k), getattr(want, k)), k


@functools.lru_cache(maxsize=None)
def _full(name):
    """The full call on a zeroed workspace, checked against the oracle once."""
    c = _case(name)
    r = _capi(name, "zero")
    assert r.status == 0
    for what in ("out", "h_n", "logp"):
        assert _err(getattr(r, what), getattr(c.ref, what)) <= TOL, what
    assert abs(float(r.loss) - float(c.ref.loss)) <= TOL
    assert int(r.correct) == int(r.pred.eq(c.y).sum())
    return r


# ---------------------------------------------------------------- c. what the workspace held before
@pytest.mark.parametrize("fill", ["ff", "big"])
@pytest.mark.parametrize("name", ["boundaries", "three_layers", "offset_many"])
def test_results_do_not_depend_on_what_the_workspace_held(name, fill):
    """c, G, the inner layers' outputs, (start, len), the loss rows and the predictions live in the
    caller's workspace and nothing clears it: step 0 must not read c, the head must read the layer
    outputs only at rows a step wrote, and the rows above the first start must be zeroed by the call.
    A workspace (and outputs) of 0xFF bytes - NaN as fp32, -1 as integers - or of 3.0e38 gives the
    bits of a zeroed one."""
    want = _full(name)
    got = _capi(name, fill)
    assert got.status == 0
    _same(got, want, ("out", "h_n", "logp", "pred", "loss", "correct"))


def test_a_small_batch_after_a_large_one_on_one_module():
    """bigcn_amd.LSTM keeps one workspace, sized by the largest batch so far and never cleared:
    ``boundaries`` (6 trees, 168 rows) after a batch of 300 trees and 600 rows has the bits of a fresh
    module's."""
    c = R.case("boundaries")
    g = torch.Generator().manual_seed(77)
    lengths = [1 + b % 3 for b in range(300)]
    big = SimpleNamespace(cls=torch.randn(sum(lengths), c.cfg["in_feats"], generator=g).to(DEV),
                          rootindex=torch.tensor([0] + lengths[:-1]).cumsum(0).to(DEV),
                          y=torch.randint(0, 4, (300,), generator=g).to(DEV))
    used, fresh = _new_model("boundaries"), _new_model("boundaries")
    loss, _ = used.evaluate(big, max_len=3)
    used.forward_batch(big.cls, big.rootindex, max_len=3, return_states=True)
    used.check_status()
    assert bool(torch.isfinite(loss))
    ws_before = used.__dict__["_state"]["ws"]
    x, root = _x(c), c.rootindex.to(DEV)
    res = []
    for m in (used, fresh):
        res.append(m.forward_batch(x, root, max_len=c.max_len, return_states=True) +
                   m.evaluate(_data(c), pred=True, max_len=c.max_len))
        m.check_status()
    assert used.__dict__["_state"]["ws"] is ws_before
    assert used.__dict__["_state"]["ws"].numel() > fresh.__dict__["_state"]["ws"].numel()
    for u, v in zip(*res):
        assert torch.equal(u, v)
    assert _err(res[0][0], c.ref.logp) <= TOL


# ---------------------------------------------------------------- d. optional outputs
def test_optional_outputs():
    """include/bgcn.h: h_n, out, loss, correct and pred may be NULL (without ``out`` the last layer
    stays in the workspace); without y, loss and correct are 0.  Every form gives the full call's
    logp, and the outputs it does pass, bit for bit.  Outputs are pre-filled with 0xFF bytes, so a
    value that reads 0 was written."""
    full = _full("boundaries")
    r = _capi("boundaries", "ff", want=("loss", "correct", "pred"))
    _same(r, full, ("logp", "loss", "correct", "pred"))
    r = _capi("boundaries", "ff", want=("h_n",))
    _same(r, full, ("logp", "h_n"))
    r = _capi("boundaries", "ff", want=("loss", "correct", "pred"), labels=False)
    _same(r, full, ("logp", "pred"))
    assert r.status == 0 and float(r.loss) == 0.0 and int(r.correct) == 0
    r = _capi("boundaries", "ff", want=("loss",))
    _same(r, full, ("logp", "loss"))
    r = _capi("boundaries", "ff", want=("correct",))
    _same(r, full, ("logp", "correct"))
    r = _capi("boundaries", "ff", want=("out", "h_n", "loss", "correct"))
    _same(r, full, ("logp", "out", "h_n", "loss", "correct"))
    # out with its row stride 2H at a 16-byte, not 256-byte aligned address
    r = _capi("boundaries", "ff", out_shift=4)
    assert r.out_ptr % 256 == 16
    _same(r, full, ("logp", "out", "h_n", "loss", "correct", "pred"))


# ---------------------------------------------------------------- e. exact invariances
@pytest.mark.parametrize("name", ["boundaries", "tile_plus_one"])
def test_a_tree_alone_has_the_bits_of_its_rows_in_the_batch(name):
    """The bitwise form of test_gpu_lstm.py::test_forward_of_one_tree_is_its_row_of_the_batch.  Both
    sides run below 8192 rows, on the exact-fp32 GEMM, whose rows are independent k-ordered chains;
    in the step a tree is one MFMA column and the four waves' partial sums are added in wave order;
    the head is one workgroup per tree.  Nothing a tree computes depends on its neighbours."""
    c = R.case(name)
    m = _model(name)
    x = _x(c)
    logp, out, h_n = m.forward_batch(x, c.rootindex.to(DEV), max_len=c.max_len, return_states=True)
    zero = torch.zeros(1, dtype=torch.int64, device=DEV)
    for b, (s, e) in enumerate(_ends(c)):
        l1, o1, h1 = m.forward_batch(x[s:e], zero, max_len=e - s, return_states=True)
        assert torch.equal(o1, out[s:e]), b
        assert torch.equal(h1[:, 0], h_n[:, b]), b
        assert torch.equal(l1[0], logp[b]), b
    m.check_status()


def test_the_order_of_the_trees_does_not_change_their_bits():
    """tile_plus_one with its 33 trees permuted: every tree's rows move, its MFMA column changes, and
    trees cross between sequence tile 0 and tile 1.  Columns and GEMM rows are independent and every
    sum has a fixed order, so each tree keeps its bits."""
    c = R.case("tile_plus_one")
    m = _model("tile_plus_one")
    x = _x(c)
    logp, out, h_n = m.forward_batch(x, c.rootindex.to(DEV), max_len=c.max_len, return_states=True)
    order = torch.randperm(c.B, generator=torch.Generator().manual_seed(3)).tolist()
    assert order.index(32) < 32 and order[32] != 32   # tile 1's tree moves into tile 0, and one of tile 0's out
    ends = _ends(c)
    xp = torch.cat([x[ends[o][0]:ends[o][1]] for o in order])
    lens = [ends[o][1] - ends[o][0] for o in order]
    rootp = torch.tensor([0] + lens[:-1]).cumsum(0)
    assert not torch.equal(rootp, c.rootindex)
    lp, op, hp = m.forward_batch(xp, rootp.to(DEV), max_len=c.max_len, return_states=True)
    m.check_status()
    for i, o in enumerate(order):
        s, n = int(rootp[i]), lens[i]
        assert torch.equal(op[s:s + n], out[ends[o][0]:ends[o][1]]), (i, o)
        assert torch.equal(hp[:, i], h_n[:, o]), (i, o)
        assert torch.equal(lp[i], logp[o]), (i, o)


def test_more_step_launches_than_needed_change_nothing():
    """max_len is a bound: a step launch past every tree's end returns at once."""
    c = R.case("boundaries")
    m = _model("boundaries")
    x, root = _x(c), c.rootindex.to(DEV)
    want = m.forward_batch(x, root, max_len=c.max_len, return_states=True)
    for max_len in (c.max_len + 1, 10 * c.max_len, c.N + 1000):
        got = m.forward_batch(x, root, max_len=max_len, return_states=True)
        for u, v in zip(got, want):
            assert torch.equal(u, v), max_len
    m.check_status()
    assert _err(want[0], c.ref.logp) <= TOL


def test_swapping_the_directions_mirrors_the_output():
    """L = 1: a model with the forward and reverse weights exchanged, on the batch with every tree's
    rows reversed, runs the original's reverse direction as its forward one: the same W rows against
    the same x rows in the same k order, step by step.  Its ``out`` with each tree's rows reversed
    back and the two column halves exchanged, and its h_n with the two directions exchanged, are the
    original's bits.  This pins the step's row / previous-row arithmetic and its per-direction weight,
    G-column and Y-column offsets against each other.  (Not for L >= 2 or logp: there the exchange
    permutes the k order of the next GEMM and of fc, and only a tolerance would hold.)"""
    c = R.case("one_layer")
    H = c.cfg["hid"]
    sd = dict(c.sd)
    for kind in ("ih", "hh"):
        sd[f"lstm.weight_{kind}_l0"], sd[f"lstm.weight_{kind}_l0_reverse"] = \
            c.sd[f"lstm.weight_{kind}_l0_reverse"], c.sd[f"lstm.weight_{kind}_l0"]
    m, ms = _model("one_layer"), _new_model("one_layer", sd)
    x, root = _x(c), c.rootindex.to(DEV)
    idx = torch.cat([torch.arange(e - 1, s - 1, -1) for s, e in _ends(c)]).to(DEV)   # each tree's rows reversed
    assert not torch.equal(idx.cpu(), torch.arange(c.N))
    _, out, h_n = m.forward_batch(x, root, max_len=c.max_len, return_states=True)
    _, outs, h_ns = ms.forward_batch(x[idx].contiguous(), root, max_len=c.max_len, return_states=True)
    m.check_status()
    ms.check_status()
    back = outs[idx]
    assert torch.equal(torch.cat([back[:, H:], back[:, :H]], dim=1), out)
    assert torch.equal(h_ns[0], h_n[1]) and torch.equal(h_ns[1], h_n[0])
    assert _err(out, c.ref.out) <= TOL


# ---------------------------------------------------------------- f. validity on the device
def _fault(c, kind):
    """(rootindex, y, max_len) of many_trees with one fault.  For ``max_len_one_short`` the starts of
    trees 285 and 286 move up one row first, so that tree 284 alone has four rows."""
    root, y, max_len = c.rootindex.clone(), c.y.clone(), c.max_len
    if kind == "start_280_repeats_279":
        root[280] = root[279]
    elif kind == "first_start_negative":
        root[0] = -1
    elif kind == "last_start_is_N":
        root[299] = c.N
    elif kind == "max_len_one_short":
        root[285] += 1
        root[286] += 1
        lens = [e - s for s, e in _ends(c, root)]
        assert max(lens) == 4 and lens.count(4) == 1 and lens[284] == 4 and min(lens) == 1
        max_len = 3
    elif kind == "label_minus_one_at_270":
        y[270] = -1
    elif kind == "label_C_at_2":
        y[2] = c.cfg["out"]
    else:
        raise KeyError(kind)
    return root, y, max_len


def _valid_batch_still_matches(m, c):
    logp = torch.empty(c.B, c.cfg["out"], device=DEV)
    loss, correct = m.evaluate(_data(c), logp=logp, max_len=c.max_len)
    m.check_status()
    assert _err(logp, c.ref.logp) <= TOL
    assert abs(float(loss) - float(c.ref.loss)) <= TOL


@pytest.mark.parametrize("kind", ["start_280_repeats_279", "first_start_negative", "last_start_is_N",
                                  "max_len_one_short"])
def test_a_bad_start_or_max_len_empties_the_batch(kind):
    """300 trees, the fault at an index the setup's first 256 threads' first iteration does not see
    (but for the negative first start).  The call returns normally and check_status raises; as the
    header documents, every final state is zero, so logp is log_softmax(fc.bias) in every row - also
    on a workspace and outputs of NaN bits; a valid batch on the same module then matches the oracle."""
    from bigcn_amd import _lib
    c = R.edge_case("many_trees")
    m = _model("many_trees")
    root, y, max_len = _fault(c, kind)
    loss, correct = m.evaluate(_data(c, root, y), max_len=max_len)
    with pytest.raises(IndexError):
        m.check_status()
    m.check_status()   # cleared
    _valid_batch_still_matches(m, c)
    r = _capi("many_trees", "ff", rootindex=root, max_len=max_len)
    assert r.status == _lib.BGCN_STATUS_SEQUENCE
    assert bool((r.h_n == 0.0).all())
    want = F.log_softmax(c.sd["fc.bias"], dim=0)
    assert float((r.logp.double() - want).abs().max()) <= 1e-6


@pytest.mark.parametrize("kind", ["label_minus_one_at_270", "label_C_at_2"])
def test_a_bad_label_is_flagged_and_adds_no_loss(kind):
    """logp does not depend on the labels; the loss is the valid trees' NLL summed and divided by B."""
    c = R.edge_case("many_trees")
    m = _model("many_trees")
    root, y, max_len = _fault(c, kind)
    logp = torch.empty(c.B, c.cfg["out"], device=DEV)
    loss, correct, pred = m.evaluate(_data(c, root, y), logp=logp, pred=True, max_len=max_len)
    with pytest.raises(IndexError):
        m.check_status()
    assert _err(logp, c.ref.logp) <= TOL
    valid = (y >= 0) & (y < c.cfg["out"])
    assert int(valid.sum()) == c.B - 1
    want = float(F.nll_loss(c.ref.logp[valid], y[valid], reduction="sum")) / c.B
    print(kind, "loss", float(loss), "oracle", want)
    assert abs(float(loss) - want) <= TOL
    assert int(correct) == int(pred.cpu().eq(y).sum())
    _valid_batch_still_matches(m, c)
