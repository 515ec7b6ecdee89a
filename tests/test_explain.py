"""CPU checks of the explain path: the plain-torch restatement (tests/explain_ref.py) reproduces
what the reference's own analysis functions computed (fixtures of tools/gen_explain_golden.py), its
ordering rule agrees with the reference's topk wherever that is determined, the fixtures keep the
gap that makes it determined, the record of to_reference_dict has the reference's keys, and the
new C entry points refuse bad arguments before any device work."""
import glob
import os

import numpy as np
import pytest
import torch

import explain_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "explain_*.npz")))
NAMES = [os.path.basename(p)[len("explain_"):-len(".npz")] for p in FIXTURES]
DIRECTIONS = (("td", "TDrumorGCN", "edge_index"), ("bu", "BUrumorGCN", "BU_edge_index"))

# Restatement (fp32) vs the reference-produced fp32 fixtures.  Measured once over the four
# fixtures: max |restatement - fixture| is 0 for the BiGCN cases (the same torch ops in the same
# order) and 7.63e-6 for the EBGCN ones (sums up to 50.6; the BatchNorm terms are folded in
# another order), 2.38e-7 for the log-probs; the bar is ten times the largest.
RESTATEMENT_BAR = 7.63e-5


def test_fixture_set():
    assert NAMES == ["bigcn_mixed", "bigcn_single", "ebgcn_mixed", "ebgcn_single"]
    for p in FIXTURES:
        assert os.path.getsize(p) < 400 * 1024


def _restated(path, dtype=torch.float32):
    sd, b, cfg, exp = X.load_fixture(path, dtype)
    out = {}
    for d, prefix, ek in DIRECTIONS:
        names, sums, gcn, _, _ = X.direction(sd, prefix, b["x"], b[ek], b["batch"], b["rootindex"], bool(cfg["ebgcn"]))
        out[d] = (names, sums, gcn)
    return sd, b, cfg, exp, out


@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_restatement_matches_reference_fixture(path):
    """Measured maxima: sums / gcn_output 7.63e-6, log-probs 2.38e-7; bar 7.63e-5 (10x)."""
    sd, b, cfg, exp, out = _restated(path)
    worst = 0.0
    for d, _, _ in DIRECTIONS:
        names, sums, gcn = out[d]
        assert names == (X.STAGES_EBGCN if cfg["ebgcn"] else X.STAGES_BIGCN)
        # the fixture holds exactly the reference's stages, and gcn_output
        assert sorted(k for k in exp if k.startswith(d + "/")) == sorted(
            [f"{d}/{n}_topk/{w}" for n in names for w in ("indices", "values")] + [f"{d}/gcn_output"])
        for s, n in enumerate(names):
            want = X.values_in_node_order(exp[f"{d}/{n}_topk/indices"], exp[f"{d}/{n}_topk/values"])
            worst = max(worst, float(np.abs(sums[s].numpy() - want).max()))
        assert gcn.shape == exp[f"{d}/gcn_output"].shape == (len(b["rootindex"]), 128)
        worst = max(worst, float(np.abs(gcn.numpy() - exp[f"{d}/gcn_output"]).max()))
    worst = max(worst, float(np.abs(X.log_probs(sd, b, cfg).numpy() - exp["logp"]).max()))
    print(f"max |restatement - fixture| {worst:.3e}")
    assert worst <= RESTATEMENT_BAR


@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_fixture_gaps_and_orders(path):
    """Inside every tree and stage adjacent sorted values are at least GAP_FLOOR apart (so the
    reference's topk order is determined); the reference's own index lists are descending orders
    of its values; on a single-tree batch the restated rule gives exactly the reference's list."""
    sd, b, cfg, exp, out = _restated(path)
    batch = b["batch"].numpy()
    B = len(b["rootindex"])
    p = X.tree_ptr(batch, B)
    assert max(np.diff(p)) <= 24
    for d, _, _ in DIRECTIONS:
        names, sums, _ = out[d]
        for s, n in enumerate(names):
            idx, vals = exp[f"{d}/{n}_topk/indices"], exp[f"{d}/{n}_topk/values"]
            node_vals = X.values_in_node_order(idx, vals)
            assert X.is_descending_order(node_vals, idx)
            for t in range(B):
                v = np.sort(node_vals[p[t]:p[t + 1]])
                assert v.size < 2 or float(np.diff(v).min()) >= X.GAP_FLOOR, (d, n, t)
            if B == 1:
                assert X.rank_segment(sums[s].numpy()).tolist() == idx.tolist(), (d, n)
            else:   # the reference's batch-wide order, restricted to a tree, is that tree's order
                order, _ = X.segment_rank(sums[s:s + 1].numpy(), batch, B)
                for t in range(B):
                    in_tree = idx[(idx >= p[t]) & (idx < p[t + 1])] - p[t]
                    assert order[0, p[t]:p[t + 1]].tolist() == in_tree.tolist(), (d, n, t)
    # x_sum of bag-of-words rows ties by construction: the reference's list must be A valid order
    x_sum = b["x"].sum(-1).numpy()
    assert np.array_equal(X.values_in_node_order(exp["x_sum_indices"], exp["x_sum_values"]), x_sum)
    assert X.is_descending_order(x_sum, exp["x_sum_indices"])
    assert len(np.unique(x_sum)) < len(x_sum)      # (it does tie)


def test_ordering_rule():
    v = np.array([1.0, np.nan, -0.0, 0.0, np.inf, 1.0, -np.inf, np.nan, -2.0], dtype=np.float32)
    assert X.rank_segment(v).tolist() == [1, 7, 4, 0, 5, 2, 3, 8, 6]
    assert X.is_descending_order(v, np.array([7, 1, 4, 5, 0, 3, 2, 8, 6]))
    assert not X.is_descending_order(v, np.array([4, 1, 7, 0, 5, 2, 3, 8, 6]))


def test_value_bar_is_measured_and_below_half_the_gap_floor():
    """The GPU tests' value bar (explain_ref.VALUE_BAR): 10x the fp32 restatement's error against
    its own fp64 run.  Re-measured here; it must stay below half the fixtures' gap floor, or a sum
    inside the bar could still change a fixture's ranking."""
    worst = {}
    for F_in, name, with_bn in X.sums_cases():
        a = X.sums_from(*X.sums_case(F_in, X.SUMS_TREES[name], with_bn, torch.float32))
        w = X.sums_from(*X.sums_case(F_in, X.SUMS_TREES[name], with_bn, torch.float64))
        worst[F_in] = max(worst.get(F_in, 0.0), float((a.double() - w).abs().max()))
    for path in FIXTURES:
        a, w = _restated(path, torch.float32)[4], _restated(path, torch.float64)[4]
        for d, _, _ in DIRECTIONS:
            worst["fixtures"] = max(worst.get("fixtures", 0.0), float((a[d][1].double() - w[d][1]).abs().max()))
    print({k: f"{v:.3e}" for k, v in worst.items()})
    for k, v in worst.items():
        # the recorded figure is of the same size as what this machine measures (fp32 summation
        # order differs between CPUs): within the factor of ten the bar allows
        assert v <= X.VALUE_BAR[k] and v >= X.FP32_RESTATEMENT_ERR[k] / 10.0, (k, v)
    assert max(X.VALUE_BAR.values()) < X.GAP_FLOOR / 2


def _fake_explanation(names, n_nodes=(3, 2)):
    from bigcn_amd.explain import DirectionExplanation, Explanation
    N, B, S = sum(n_nodes), len(n_nodes), len(names)
    batch = torch.repeat_interleave(torch.arange(B), torch.tensor(n_nodes))
    sums = torch.arange(S * N, dtype=torch.float32).view(S, N)
    order, srt = X.segment_rank(sums.numpy(), batch.numpy(), B)
    d = DirectionExplanation(sums, torch.from_numpy(order), torch.from_numpy(srt), names, torch.zeros(B, 128))
    xo, xs = X.segment_rank(sums[:1].numpy(), batch.numpy(), B)
    return Explanation(sums[0], torch.from_numpy(xo[0]), torch.from_numpy(xs[0]), d, d, torch.zeros(B, 4),
                       torch.tensor([1, 3]), batch, torch.tensor([1, 3]))


@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_reference_dict_keys_match_the_fixture(path):
    import json
    from bigcn_amd import ops
    _, _, cfg, exp = X.load_fixture(path)
    names = ops.STAGES_EBGCN if cfg["ebgcn"] else ops.STAGES_BIGCN
    assert names == (X.STAGES_EBGCN if cfg["ebgcn"] else X.STAGES_BIGCN)
    rec = _fake_explanation(names).to_reference_dict(1)
    assert set(rec) == {"x_sum_top_k", "td_gcn_explanations", "bu_gcn_explanations", "rootindex", "prediction"}
    want = {k.split("/")[1] for k in exp if k.startswith("td/")}
    assert set(rec["td_gcn_explanations"]) == set(rec["bu_gcn_explanations"]) == want
    assert rec["rootindex"] == 0 and rec["prediction"] == 3     # node 3 is tree 1's first node
    top = rec["td_gcn_explanations"][names[0] + "_topk"]
    assert top == [[1, 0], [4.0, 3.0]]                            # local indices, descending
    assert np.asarray(rec["td_gcn_explanations"]["gcn_output"]).shape == (1, 128)
    assert json.loads(json.dumps(rec)) == rec


def test_exports():
    import bigcn_amd
    from bigcn_amd import _lib
    from bigcn_amd.explain import explain, explain_direction, segment_rank   # noqa: F401
    assert "explain" in bigcn_amd.__all__ and "segment_rank" in bigcn_amd.__all__
    for name in ("bgcn_explain_sums_workspace_size", "bgcn_explain_sums", "bgcn_segment_rank_workspace_size",
                 "bgcn_segment_rank"):
        assert name in _lib.EXPORTED_SYMBOLS and name in _lib._SIGS
    text = open(os.path.join(ROOT, "include", "bgcn.h")).read()
    assert f"#define BGCN_SEGMENT_RANK_LDS {_lib.BGCN_SEGMENT_RANK_LDS}\n" in text
    lib = _lib.load_library()
    assert lib.bgcn_explain_sums_workspace_size(8) > 0 and lib.bgcn_segment_rank_workspace_size(8) >= 4 * 10
    assert lib.bgcn_abi_version() == 12


def test_invalid_arguments_fail_before_any_device_work():
    from bigcn_amd import _lib
    lib = _lib.load_library()

    def sums(N=10, B=2, F=8, hid=64):
        return lib.bgcn_explain_sums(None, 64, None, 64, None, F, None, None, N, B, F, hid, None, None, None, N, None,
                                     None, None, 0, None)
    assert sums(hid=32) == -1 and b"hidden size" in lib.bgcn_last_error()
    assert sums(F=6) == -1 and b"multiple of 4" in lib.bgcn_last_error()
    assert sums(N=-1) == -1 and b"negative" in lib.bgcn_last_error()
    assert sums() == -1 and b"null pointer" in lib.bgcn_last_error()
    assert sums(N=0) == 0                                         # nothing to do
    assert lib.bgcn_segment_rank(None, 10, 1, None, -1, 2, None, None, None, None, 0, None) == -1
    assert b"negative" in lib.bgcn_last_error()
    assert lib.bgcn_segment_rank(None, 4, 1, None, 10, 2, None, None, None, None, 0, None) == -1
    assert b"leading dimension" in lib.bgcn_last_error()
    assert lib.bgcn_segment_rank(None, 10, 1, None, 10, 0, None, None, None, None, 0, None) == -1
    assert lib.bgcn_segment_rank(None, 0, 3, None, 0, 0, None, None, None, None, 0, None) == 0
