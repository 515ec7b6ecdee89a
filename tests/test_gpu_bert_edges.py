"""Edge-shape, path-switch and exact-invariance checks of the TreeBERT baseline (bgcn_bert_eval,
bigcn_amd.TreeBERT) beside tests/test_gpu_bert.py: the cases of ``bert_ref.EDGE_CASES`` against the
fp64 oracle, and properties that hold bit for bit by construction.

a. Parity and rankings at test_gpu_bert.py's bars (1e-4 absolute; attn_sum 1e-4 max(1, |ref|)), and
   ``pred`` equal to the oracle's (tests/test_bert.py holds every tree's top-two gap above 2e-4).  With
   BGCN_BERT_EDGES_OUT set, the records of this file go to that JSON (profiles/bert_parity_edges.json
   is such a record; run this file alone to write it).
b. Exact invariances.  Below 8192 rows every GEMM is the exact-fp32 kernel, whose rows are independent
   k-ordered chains; LayerNorm is one wave per row; attention is one wave per (sequence, head, 32
   queries) and reads its own sequence only; the column sums are added in a fixed (query tile, head)
   order; the head is one workgroup per tree.  So a tree's bits do not depend on its neighbours, its
   place in the batch, max_pos (the grids' size), ldx, the optional outputs, the stream, or what the
   module ran before.
c. The workspace and every output with guard bytes behind them, pre-filled with NaN bits or 3e38.
d. The head: a bitwise tie across waves and wave halves, and one class.
e. Validity decided on the device at B = 300 and at max_pos = 40: what include/bgcn.h promises of a
   flagged batch.  None of these inputs reads or writes out of bounds.
"""
import ctypes
import functools
import json
import os
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import bert_ref as R
from bert_gpu_util import BAR, DEV, _case, _check_rankings, _data, _err, _inputs, _model, _parity_errors

pytestmark = pytest.mark.gpu

EDGES = sorted(R.EDGE_CASES)
UNDER_SWITCH = sorted(R.CASES) + [n for n in EDGES if n != "rows_over_switch"]
_record = {"bar": BAR, "cases": {}, "exactness": {}}


def _write_record():
    out = os.environ.get("BGCN_BERT_EDGES_OUT")
    if out:
        with open(out, "w") as f:
            json.dump(_record, f, indent=1, sort_keys=True)


def _ends(c, rootindex=None):
    roots = (c.rootindex if rootindex is None else rootindex).tolist()
    return list(zip(roots, roots[1:] + [c.N]))


def _full(m, x, root):
    """(logp, hidden, hidden_sum, attn_sum) of the full form."""
    logp, hidden, (hsum, asum) = m.forward_batch(x, root, return_hidden=True, return_sums=True)
    return logp, hidden, hsum, asum


def _all_equal(got, want, what=None):
    for i, (u, v) in enumerate(zip(got, want)):
        assert torch.equal(u, v), (what, i)


# ---------------------------------------------------------------- a. parity and rankings
@pytest.mark.parametrize("name", EDGES)
def test_parity_with_the_fp64_oracle(name):
    c, m = _case(name), _model(name)
    x, root, y = _inputs(name)
    logp_root = m.forward_batch(x, root)
    logp, hidden, hsum, asum = _full(m, x, root)
    pred_root = m._run(x, root, y=y, want_pred=True)
    pred_full = m._run(x, root, y=y, want_pred=True, want_sums=True)
    m.check_status()
    errs = _parity_errors(c, logp_root, logp, hidden, hsum, asum)
    errs["loss"] = max(abs(float(r["loss"]) - float(c.ref.loss)) for r in (pred_root, pred_full))
    print(name, {k: f"{v:.3e}" for k, v in errs.items()})
    _record["cases"][name] = {"errors": errs, "margins": {k: BAR / max(v, 1e-300) for k, v in errs.items()},
                              "N": c.N, "B": c.B, "heads": c.heads, "top_score": c.ref.top_score,
                              "pred_gap": R.pred_gap(c.ref.logp)}
    _write_record()
    assert torch.isfinite(hidden).all() and torch.isfinite(asum).all()
    assert max(errs.values()) <= BAR, errs
    for r in (pred_root, pred_full):
        assert torch.equal(r["pred"].cpu(), c.ref.pred)
        assert int(r["correct"]) == c.ref.correct
    if c.first:   # rows outside any sequence
        assert float(hidden[:c.first].abs().sum()) == 0.0 and float(hsum[:c.first].abs().sum()) == 0.0
        assert float(asum[:c.first].abs().sum()) == 0.0
    if name == "classes_1":
        assert logp.shape == (c.B, 1) and bool((logp == 0.0).all()) and bool((logp_root == 0.0).all())
        assert bool((pred_root["pred"] == 0).all()) and float(pred_root["loss"]) == 0.0 and float(pred_full["loss"]) == 0.0
        assert int(pred_root["correct"]) == c.B


@pytest.mark.parametrize("name", EDGES)
def test_explain_rankings(name):
    """Values within the bar; the order equal to the oracle's wherever the oracle's sorted values are
    more than 2e-4 from both neighbours (tests/test_bert.py holds the cases to at most 5 % left out)."""
    import bigcn_amd
    c, m = _case(name), _model(name)
    res = bigcn_amd.explain(m, _data(name, drop_first=True))
    _check_rankings(c, res)


# ---------------------------------------------------------------- b. exact invariances
@pytest.mark.parametrize("name", ["heads3_tiles", "boundaries"])
def test_a_tree_alone_has_the_bits_of_its_rows_in_the_batch(name):
    c, m = _case(name), _model(name)
    x, root, _ = _inputs(name)
    logp_root = m.forward_batch(x, root)
    logp, hidden, hsum, asum = _full(m, x, root)
    zero = torch.zeros(1, dtype=torch.int64, device=DEV)
    for b, (s, e) in enumerate(_ends(c)):
        l1, h1, hs1, as1 = _full(m, x[s:e], zero)
        assert torch.equal(h1, hidden[s:e]) and torch.equal(hs1, hsum[s:e]) and torch.equal(as1, asum[s:e]), b
        assert torch.equal(l1[0], logp[b]), b
        assert torch.equal(m.forward_batch(x[s:e], zero)[0], logp_root[b]), b
    m.check_status()
    assert _err(logp, c.ref.logp) <= BAR


@pytest.mark.parametrize("name,order", [("heads3_tiles", [3, 1, 0, 2]), ("boundaries", [5, 0, 7, 2, 6, 1, 4, 3])])
def test_the_order_of_the_trees_does_not_change_their_bits(name, order):
    """Rows are moved with their trees: every tree changes its start, its workgroups and, in
    heads3_tiles, its rows' place in the partial column sums."""
    c, m = _case(name), _model(name)
    x, root, _ = _inputs(name)
    logp_root = m.forward_batch(x, root)
    logp, hidden, hsum, asum = _full(m, x, root)
    ends = _ends(c)
    xp = torch.cat([x[ends[o][0]:ends[o][1]] for o in order])
    lens = [ends[o][1] - ends[o][0] for o in order]
    rootp = torch.tensor([0] + lens[:-1]).cumsum(0)
    assert not torch.equal(rootp, c.rootindex)
    lrp = m.forward_batch(xp, rootp.to(DEV))
    lp, hp, hsp, asp = _full(m, xp, rootp.to(DEV))
    m.check_status()
    for i, o in enumerate(order):
        s, n = int(rootp[i]), lens[i]
        a, e = ends[o]
        assert torch.equal(hp[s:s + n], hidden[a:e]) and torch.equal(hsp[s:s + n], hsum[a:e]), (i, o)
        assert torch.equal(asp[s:s + n], asum[a:e]), (i, o)
        assert torch.equal(lp[i], logp[o]) and torch.equal(lrp[i], logp_root[o]), (i, o)


@pytest.mark.parametrize("name", ["heads3_tiles", "boundaries", "offset_strided"])
def test_max_pos_only_sizes_the_grids(name):
    """position_embeddings cut to the batch's longest tree (max_pos = max(lengths)): the embedding,
    attention and column-sum grids shrink to what the batch needs, nothing else changes."""
    from bigcn_amd import TreeBERT
    c, m = _case(name), _model(name)
    cfg, longest = c.cfg, max(c.cfg["lengths"])
    assert longest < cfg["max_pos"]
    sd = dict(c.sd)
    key = "BERT.embeddings.position_embeddings.weight"
    sd[key] = sd[key][:longest].clone()
    short = TreeBERT(hidden=cfg["hidden"], heads=c.heads, intermediate=cfg["intermediate"], num_layers=cfg["layers"],
                     max_pos=longest, vocab=R.VOCAB, num_classes=cfg["out"])
    short.load_state_dict(sd, strict=True)
    short = short.to(DEV).eval()
    x, root, _ = _inputs(name)
    _all_equal(_full(short, x, root), _full(m, x, root), "full")
    assert torch.equal(short.forward_batch(x, root), m.forward_batch(x, root))
    short.check_status()
    m.check_status()


@pytest.mark.parametrize("name", ["heads3_tiles", "offset_strided"])
def test_a_padded_x_and_its_contiguous_copy_agree(name):
    c, m = _case(name), _model(name)
    x, root, _ = _inputs(name)
    H = c.cfg["hidden"]
    wide = torch.full((c.N, H + 8), 7.0, device=DEV)
    wide[:, :H] = x
    xp, xc = wide[:, :H], x.contiguous()
    assert xp.stride(0) == H + 8 and xc.stride(0) == H
    _all_equal(_full(m, xp, root), _full(m, xc, root), "full")
    assert torch.equal(m.forward_batch(xp, root), m.forward_batch(xc, root))
    m.check_status()


def test_root_only_logp_has_the_bits_of_the_full_forms():
    """At position 0, P is exactly 1 for key 0 (exp(0) / 1) and 0 elsewhere, and the MFMA adds exact
    zeros to v: ctx = v + bias in both forms.  Below the 8192-row switch both forms run the exact-fp32
    GEMM, whose rows do not depend on M, so the two logp agree bit for bit.  rows_over_switch's full
    form runs the six-product kernel: there the two forms agree within the bar only (recorded)."""
    worst = 0.0
    for name in UNDER_SWITCH:
        m = _model(name)
        x, root, _ = _inputs(name)
        a, b = m.forward_batch(x, root), m.forward_batch(x, root, return_sums=True)[0]
        d = float((a - b).abs().max())
        worst = max(worst, d)
        print(name, "root-only vs full logp", d)
        m.check_status()
    m = _model("rows_over_switch")
    x, root, _ = _inputs("rows_over_switch")
    over = float((m.forward_batch(x, root) - m.forward_batch(x, root, return_sums=True)[0]).abs().max())
    m.check_status()
    _record["exactness"]["root_only_vs_full_logp"] = {"under_switch_worst": worst, "cases": len(UNDER_SWITCH),
                                                      "rows_over_switch": over}
    _write_record()
    assert worst == 0.0
    assert over <= BAR


def test_a_non_default_stream_gives_the_same_bits():
    m = _model("heads3_tiles")
    x, root, _ = _inputs("heads3_tiles")
    want = _full(m, x, root) + (m.forward_batch(x, root),)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        got = _full(m, x, root) + (m.forward_batch(x, root),)
    s.synchronize()
    m.check_status()
    _all_equal(got, want)


@pytest.mark.parametrize("large_first", [True, False])
def test_a_small_batch_after_a_large_one_on_one_module(large_first):
    """One module on rows_over_switch's batch (8217 rows, 127 trees) and on ``single``'s one row, in
    both orders, against fresh modules: the workspace never shrinks, so the small call runs over the
    large one's partial sums, sequence table and ``first``."""
    c = _case("rows_over_switch")
    big, small = _inputs("rows_over_switch")[:2], _inputs("single")[:2]
    used = R.model_for(c, DEV)
    order = (big, small) if large_first else (small, big)
    got = []
    for x, root in order:
        got.append(_full(used, x, root) + (used.forward_batch(x, root),))
    used.check_status()
    for (x, root), g in zip(order, got):
        fresh = R.model_for(c, DEV)
        _all_equal(g, _full(fresh, x, root) + (fresh.forward_batch(x, root),), int(x.size(0)))
        fresh.check_status()
    if large_first:   # the last fresh module ran the one-row batch alone
        for full in (False, True):
            assert used.__dict__["_state"]["ws"][full].numel() > fresh.__dict__["_state"]["ws"][full].numel()


# ---------------------------------------------------------------- the C ABI, called directly
GUARD = 256          # bytes behind the workspace and every output
GUARD_BYTE = 0xA5
FULL = ("hidden_out", "hidden_sum", "attn_sum")
OPTIONAL = ("y", "loss", "correct", "pred")


def _guarded(nbytes, fill):
    """``nbytes`` of zero bytes, 0xFF bytes (NaN as fp32, -1 as integers) or the fp32 3.0e38, and GUARD
    bytes of GUARD_BYTE right behind them."""
    b = torch.empty(nbytes + GUARD, dtype=torch.uint8, device=DEV)
    if fill == "zero":
        b[:nbytes].zero_()
    elif fill == "ff":
        b[:nbytes].fill_(0xFF)
    else:
        assert fill == "big" and nbytes % 4 == 0
        b[:nbytes].view(torch.float32).fill_(3.0e38)
    b[nbytes:].fill_(GUARD_BYTE)
    return b


@functools.lru_cache(maxsize=None)
def _weights(name):
    return {k: v.float().contiguous().to(DEV) for k, v in _case(name).sd.items()}


def _capi(name, full=FULL, fill="zero", want=OPTIONAL):
    """One bgcn_bert_eval call on the case: a workspace of exactly the reported size and every output,
    each pre-filled with ``fill`` and followed by guard bytes.  ``full``: which of hidden_out /
    hidden_sum / attn_sum are passed (none: the root-only form); ``want``: which of y / loss / correct /
    pred.  Returns host copies of what was passed, the status word and whether every guard byte survived."""
    from bigcn_amd import _lib
    from bigcn_amd.bert import _LAYER_FIELDS, _TOP_FIELDS, LN_EPS
    lib = _lib.lib()
    c, w = _case(name), _weights(name)
    cfg = c.cfg
    N, B, H, C, L = c.N, c.B, cfg["hidden"], cfg["out"], cfg["layers"]
    x, root, y = _inputs(name)
    need = lib.bgcn_bert_workspace_size(N, B, H, cfg["intermediate"], L, int(bool(full)))
    assert need > 0 and need % 256 == 0
    sizes = {"ws": need, "logp": 4 * B * C, "status": 4, "loss": 4, "correct": 4, "pred": 8 * B,
             "hidden_out": 4 * N * H, "hidden_sum": 4 * N, "attn_sum": 4 * N}
    bufs = {k: _guarded(v, fill) for k, v in sizes.items()}
    a = _lib.BertArgs()
    a.x, a.ldx, a.num_nodes, a.seq_start, a.num_seqs = x.data_ptr(), x.stride(0), N, root.data_ptr(), B
    a.hidden, a.heads, a.intermediate, a.num_layers = H, c.heads, cfg["intermediate"], L
    a.max_pos, a.out_feats, a.ln_eps = cfg["max_pos"], C, LN_EPS
    for field, key in _TOP_FIELDS:
        setattr(a, field, w[key].data_ptr())
    for i in range(L):
        for field, key in _LAYER_FIELDS:
            setattr(a.layer[i], field, w[f"BERT.encoder.layer.{i}.{key}"].data_ptr())
    a.y = y.data_ptr() if "y" in want else None
    a.logp, a.status = bufs["logp"].data_ptr(), bufs["status"].data_ptr()
    for k in ("loss", "correct", "pred"):
        setattr(a, k, bufs[k].data_ptr() if k in want else None)
    for k in FULL:
        setattr(a, k, bufs[k].data_ptr() if k in full else None)
    rc = lib.bgcn_bert_eval(ctypes.addressof(a), bufs["ws"].data_ptr(), need, _lib.stream_handle())
    assert rc == 0, lib.bgcn_last_error()
    torch.cuda.synchronize()
    f32 = lambda k: bufs[k][:sizes[k]].view(torch.float32)
    r = SimpleNamespace(status=int(bufs["status"][:4].view(torch.int32)[0]), logp=f32("logp").view(B, C).cpu(),
                        guards=all(bool((bufs[k][sizes[k]:] == GUARD_BYTE).all()) for k in bufs),
                        hidden_out=None, hidden_sum=None, attn_sum=None, loss=None, correct=None, pred=None)
    if "hidden_out" in full:
        r.hidden_out = f32("hidden_out").view(N, H).cpu()
    for k in ("hidden_sum", "attn_sum"):
        if k in full:
            setattr(r, k, f32(k).cpu())
    if "loss" in want:
        r.loss = f32("loss").cpu()
    if "correct" in want:
        r.correct = bufs["correct"][:4].view(torch.int32).cpu()
    if "pred" in want:
        r.pred = bufs["pred"][:8 * B].view(torch.int64).cpu()
    return r


def _same(got, want, fields):
    for k in fields:
        assert torch.equal(getattr(got, k), getattr(want, k)), k


@functools.lru_cache(maxsize=None)
def _clean(name, full):
    """The call on a zeroed workspace, checked against the oracle once."""
    c = _case(name)
    r = _capi(name, FULL if full else ())
    assert r.status == 0 and r.guards
    assert _err(r.logp, c.ref.logp) <= BAR and abs(float(r.loss) - float(c.ref.loss)) <= BAR
    assert torch.equal(r.pred, c.ref.pred) and int(r.correct) == c.ref.correct
    if full:
        assert _err(r.hidden_out, c.ref.hidden) <= BAR and _err(r.hidden_sum, c.ref.hidden_sum) <= BAR * c.cfg["hidden"]
        assert bool(((r.attn_sum.double() - c.ref.attn_sum).abs() <= BAR * c.ref.attn_sum.abs().clamp(min=1)).all())
    return r


# ---------------------------------------------------------------- c. workspace and output bounds
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("fill", ["ff", "big"])
@pytest.mark.parametrize("name", ["heads3_tiles", "offset_strided"])
def test_the_call_stays_inside_its_buffers_and_reads_nothing_stale(name, fill, full):
    """A workspace of exactly bgcn_bert_workspace_size's bytes and every output, each followed by 256
    guard bytes and pre-filled with NaN bits or 3e38: the bits of a call on zeroed buffers, and every
    guard byte unchanged.  (A correct kernel stays inside its buffers; this only looks.)"""
    want = _clean(name, full)
    got = _capi(name, FULL if full else (), fill)
    assert got.status == 0
    assert got.guards
    _same(got, want, ("logp", "loss", "correct", "pred") + (FULL if full else ()))


SUBSETS = [tuple(k for i, k in enumerate(FULL) if mask >> i & 1) for mask in range(1, 8)]


@pytest.mark.parametrize("subset", SUBSETS, ids=["+".join(s) for s in SUBSETS])
def test_every_subset_of_the_full_forms_outputs(subset):
    """include/bgcn.h: hidden_out, hidden_sum and attn_sum may each be NULL; any one of them selects
    the full form.  What a subset produces is the all-three call's, and logp is the same in all."""
    want = _clean("boundaries", True)
    got = _capi("boundaries", subset, "ff")
    assert got.status == 0 and got.guards
    _same(got, want, ("logp", "loss", "correct", "pred") + subset)


@pytest.mark.parametrize("full", [False, True])
def test_optional_labels_loss_correct_and_pred(full):
    """y, loss, correct and pred may be NULL, singly and together; without y, loss and correct are 0.
    Outputs are pre-filled with 0xFF bytes, so a value that reads 0 was written."""
    want = _clean("boundaries", full)
    outs = FULL if full else ()
    for drop in ("loss", "correct", "pred"):
        keep = tuple(k for k in OPTIONAL if k != drop)
        got = _capi("boundaries", outs, "ff", keep)
        assert got.status == 0 and got.guards
        _same(got, want, ("logp",) + tuple(k for k in keep if k != "y") + outs)
    got = _capi("boundaries", outs, "ff", ("loss", "correct", "pred"))     # no labels
    assert got.status == 0 and got.guards
    _same(got, want, ("logp", "pred") + outs)
    assert float(got.loss) == 0.0 and int(got.correct) == 0
    got = _capi("boundaries", outs, "ff", ())                               # none of the four
    assert got.status == 0 and got.guards
    _same(got, want, ("logp",) + outs)
    got = _capi("boundaries", outs, "ff", ("y",))                           # labels, nowhere to report
    assert got.status == 0 and got.guards
    _same(got, want, ("logp",) + outs)


# ---------------------------------------------------------------- d. the head
def test_argmax_takes_the_first_of_two_equal_classes_across_waves():
    """Classes 5 and 38 get the same fc row and bias: each logit is one wave's fixed-order sum of the
    same numbers (class 5 on wave 1, class 38 on wave 2), so the two are bitwise equal; + 50 on both
    biases puts them on top.  In seq_head_tail they sit in different halves of the wave (lanes 5 and
    38).  torch's max returns the first maximal index: 5."""
    c = _case("classes_64")
    sd = {k: v.clone() for k, v in c.sd.items()}
    sd["fc.weight"][38] = sd["fc.weight"][5]
    sd["fc.bias"][38] = sd["fc.bias"][5]
    sd["fc.bias"][5] += 50.0
    sd["fc.bias"][38] += 50.0
    tied = R.model_for(SimpleNamespace(cfg=c.cfg, heads=c.heads, sd=sd), DEV)
    x, root, y = _inputs("classes_64")
    for full in (False, True):
        r = tied._run(x, root, y=y, want_pred=True, want_sums=full)
        logp = r["logp"]
        assert torch.equal(logp[:, 5], logp[:, 38])
        others = torch.cat((logp[:, :5], logp[:, 6:38], logp[:, 39:]), 1)
        assert bool((others.max(1).values < logp[:, 5]).all())
        assert r["pred"].tolist() == [5] * c.B
        assert int(r["correct"]) == int(c.y.eq(5).sum())
    tied.check_status()


# ---------------------------------------------------------------- e. validity on the device
def _out(r):
    return [r[k] for k in ("logp", "loss", "correct", "pred")] + ([r["hidden"], r["sums"]] if r["hidden"] is not None else [])


@functools.lru_cache(maxsize=None)
def _fresh(name):
    """Both forms of the valid batch on a module that never saw anything else."""
    c = _case(name)
    m = R.model_for(c, DEV)
    x, root, y = _inputs(name)
    res = {full: _out(m._run(x, root, y=y, want_pred=True, want_hidden=full, want_sums=full)) for full in (False, True)}
    m.check_status()
    assert _err(res[True][0], c.ref.logp) <= BAR and _err(res[False][0], c.ref.logp) <= BAR
    return res


def _fault(c, kind):
    """(rootindex, y) of the case with one fault; at B = 300 at indices past the first 256."""
    root, y, B = c.rootindex.clone(), c.y.clone(), c.B
    if kind == "first_start_negative":
        root[0] = -1
    elif kind == "last_start_is_N":
        root[B - 1] = c.N
    elif kind == "equal_starts":
        i = 280 if B > 281 else B - 2
        root[i + 1] = root[i]
    elif kind == "last_tree_one_too_long":      # short_pos: 39, 7 and max_pos + 1 = 41 rows
        assert c.cfg["max_pos"] == 40 and c.N == 87
        root = torch.tensor([0, 39, 46])
        lens = [e - s for s, e in _ends(c, root)]
        assert lens == [39, 7, 41]
    elif kind == "label_C":
        y[290 if B > 290 else 1] = c.cfg["out"]
    elif kind == "label_minus_one":
        y[B // 2] = -1
    else:
        raise KeyError(kind)
    return root, y


def _poison_workspaces(m):
    for ws in m.__dict__["_state"]["ws"].values():
        ws.fill_(0xFF)


def _module_with_workspaces(name):
    m = _model(name)
    x, root, y = _inputs(name)
    m._run(x, root, y=y)
    m._run(x, root, y=y, want_sums=True)
    m.check_status()
    return m


@pytest.mark.parametrize("name,kind", [("many_trees", "first_start_negative"), ("many_trees", "last_start_is_N"),
                                       ("many_trees", "equal_starts"), ("short_pos", "first_start_negative"),
                                       ("short_pos", "last_start_is_N"), ("short_pos", "equal_starts"),
                                       ("short_pos", "last_tree_one_too_long")])
def test_a_bad_start_or_length_empties_the_batch(name, kind):
    """include/bgcn.h: a fault in seq_start or a length empties every sequence and every row counts as
    outside any sequence: check_status raises, the full form's hidden, hidden_sum and attn_sum are
    exactly zero in every row, and logp is finite in both forms - over a workspace and a ``hidden`` of
    NaN bits.  The next valid call on the module has a fresh module's bits."""
    c, m = _case(name), _module_with_workspaces(name)
    x, root, y = _inputs(name)
    broot, by = _fault(c, kind)
    fresh = _fresh(name)
    for full in (False, True):
        _poison_workspaces(m)
        hidden = torch.full((c.N, c.cfg["hidden"]), float("nan"), device=DEV) if full else None
        r = m._run(x, broot.to(DEV), y=by.to(DEV), want_pred=True, want_sums=full, hidden=hidden)
        with pytest.raises(IndexError):
            m.check_status()
        m.check_status()   # cleared
        assert bool(torch.isfinite(r["logp"]).all()), full
        if full:
            assert bool((r["hidden"] == 0.0).all()) and bool((r["sums"] == 0.0).all())
        good = m._run(x, root, y=y, want_pred=True, want_hidden=full, want_sums=full)
        m.check_status()
        _all_equal(_out(good), fresh[full], (kind, full))


@pytest.mark.parametrize("name,kind", [("many_trees", "label_C"), ("many_trees", "label_minus_one"),
                                       ("short_pos", "label_C"), ("short_pos", "label_minus_one")])
def test_a_bad_label_is_flagged_and_adds_no_loss(name, kind):
    """logp, pred and the full form's outputs do not depend on the labels: the good run's bits.  The
    loss is what seq_finish defines: the valid trees' NLL terms summed and divided by B (all the trees,
    the flagged one included), here restated on the oracle's logp."""
    c, m = _case(name), _module_with_workspaces(name)
    x, root, y = _inputs(name)
    broot, by = _fault(c, kind)
    assert torch.equal(broot, c.rootindex)
    valid = (by >= 0) & (by < c.cfg["out"])
    assert int(valid.sum()) == c.B - 1
    want_loss = float(F.nll_loss(c.ref.logp[valid], by[valid], reduction="sum")) / c.B
    fresh = _fresh(name)
    for full in (False, True):
        _poison_workspaces(m)
        r = m._run(x, root, y=by.to(DEV), want_pred=True, want_hidden=full, want_sums=full)
        with pytest.raises(IndexError):
            m.check_status()
        got = _out(r)
        assert torch.equal(got[0], fresh[full][0]) and torch.equal(got[3], fresh[full][3])
        _all_equal(got[4:], fresh[full][4:], (kind, full))
        print(name, kind, "loss", float(r["loss"]), "oracle", want_loss)
        assert abs(float(r["loss"]) - want_loss) <= BAR
        assert int(r["correct"]) == int(r["pred"].cpu().eq(by).sum())
        good = m._run(x, root, y=y, want_pred=True, want_hidden=full, want_sums=full)
        m.check_status()
        _all_equal(_out(good), fresh[full], (kind, full))
