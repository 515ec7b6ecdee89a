"""GPU checks of the compare path against fixtures only (tools/gen_compare_golden.py wrote them on
a CPU with networkx and scipy) and the exact numpy restatement tests/compare_ref.py, which
tests/test_compare.py pins to the same fixtures.

Bars.  Centralities: bit-equal to the restatement (the same integers, the same single fp64 division
rounded once to fp32) and within two fp32 ulps (2.4e-7 relative; exact zeros stay zero) of
networkx's fp64 values.  Kendall, Somers, Jaccard: bit-equal to the restatement (exact rationals
rounded once).  Pearson, Spearman: within max(16 x restatement_err, 1e-12) of scipy's stored values
(restatement_err: the restatement's own distance from scipy, measured when the fixture was written,
4.4e-16; the floor is 32 terms of fp64 rounding with a wide margin)."""
import argparse
import functools
import glob
import os

import numpy as np
import pytest
import torch

import compare_ref as C
import explain_ref as X

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "compare_*.npz")))
NAMES = [os.path.basename(p)[len("compare_"):-len(".npz")] for p in FIXTURES]
DEV = "cuda:0"
ULP2, cases_of, similarity_bar = C.ULP2, C.cases_of, C.similarity_bar


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


@functools.lru_cache(maxsize=None)
def _fixture(path):
    """The fixture and the restatement's centralities, computed once."""
    z = np.load(path)
    ei, batch, B = z["edge_index"], z["batch"], int(z["num_graphs"])
    return z, ei, batch, B, C.centrality(ei, batch, B)


def _data(ei, batch, B):
    from bigcn_amd.data import Batch
    return Batch(edge_index=torch.from_numpy(ei), batch=torch.from_numpy(batch), num_graphs=B).to(DEV)


# ------------------------------------------------------------------ tree_centrality
@pytest.mark.parametrize("path", [p for p, n in zip(FIXTURES, NAMES) if n != "lists"], ids=[n for n in NAMES if n != "lists"])
def test_tree_centrality_is_the_closed_form_exactly(path):
    from bigcn_amd import compare, tree_centrality
    z, ei, batch, B, want = _fixture(path)
    ei_d, batch_d = torch.from_numpy(ei).to(DEV), torch.from_numpy(batch).to(DEV)
    cent = tree_centrality(ei_d, batch_d, B, validate=True)
    assert cent.dtype == torch.float32 and cent.shape == (3, len(batch))
    got = cent.cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want))
    nxc = z["nx_centrality"]
    zero = nxc == 0
    assert np.all(got[zero] == 0)
    rel = np.abs(got[~zero].astype(np.float64) - nxc[~zero]) / np.abs(nxc[~zero])
    print(f"vs networkx: max relative {rel.max():.3e} (bar {ULP2:.1e})")
    assert rel.max() <= ULP2
    assert torch.equal(tree_centrality(ei_d, batch_d), cent)       # num_graphs from batch; deterministic
    # compare() with no model: the three centrality rankings, which are the stored closed-form orders
    k = int(z["k"])
    s = compare(_data(ei, batch, B), {}, k=k)
    assert s.names == C.CENTRALITY_NAMES and s.k == k
    assert np.array_equal(s.centrality_order.cpu().numpy(), z["order"])
    assert np.array_equal(_bits(s.centrality.cpu().numpy()), _bits(want))
    assert np.array_equal(_bits(s.centrality_sorted.cpu().numpy()), _bits(X.segment_rank(want, batch, B)[1]))
    assert np.array_equal(s.valid.cpu().numpy(), z["valid"])
    p = X.tree_ptr(batch, B)
    for t in range(B):
        rec = s.centrality_dict(t)
        assert rec["betweenness"][0] == z["order"][1, p[t]:p[t + 1]].tolist()


# ------------------------------------------------------------------ rank_similarity
def _similarity_cases():
    out = []
    for path, name in zip(FIXTURES, NAMES):
        z = np.load(path)
        out += [pytest.param(path, i, id=f"{name}-k{k}-V{V}") for i, (k, V, *_) in enumerate(cases_of(z))]
    return out


@pytest.mark.parametrize("path,case", _similarity_cases())
def test_rank_similarity_matches_restatement_and_scipy(path, case):
    from bigcn_amd import rank_similarity
    z, ei, batch, B, _ = _fixture(path)
    k, V, sim, valid, _ = cases_of(z)[case]
    orders = z["orders"][:V]
    want, want_valid = C.rank_similarity(orders, batch, B, k)
    got, got_valid = rank_similarity(torch.from_numpy(orders).to(DEV), torch.from_numpy(batch).to(DEV), k, B)
    assert got.dtype == torch.float64 and got.shape == (B, 5, V, V) and got_valid.dtype == torch.bool
    got, got_valid = got.cpu().numpy(), got_valid.cpu().numpy()
    assert np.array_equal(got_valid, valid) and np.array_equal(got_valid, want_valid)
    assert np.array_equal(_bits(got[:, 2:]), _bits(want[:, 2:]))            # exact rationals rounded once
    bar = similarity_bar(z)
    err = float(np.abs(got[:, :2] - sim[:, :2]).max())
    print(f"Pearson / Spearman vs scipy: max err {err:.3e} (bar {bar:.3e})")
    assert err <= bar
    assert np.all(got[~valid] == 0)                                         # skipped trees: zeros
    kept = got[valid]
    assert np.array_equal(_bits(kept), _bits(kept.transpose(0, 1, 3, 2)))   # symmetric bit for bit
    diag = np.diagonal(kept, axis1=2, axis2=3)
    assert np.all(diag[:, 2:] == 1.0)
    # metrics 0 and 1 on the diagonal: a product, a square root and a division, each within an ulp
    assert np.all(np.abs(diag[:, :2] - 1.0) <= 4 * 2.0 ** -52)


# ------------------------------------------------------------------ compare(), end to end
def _models_and_batches():
    """Both explain_*_mixed fixtures' models, and both their batches."""
    from bigcn_amd import EBGCN, BiGCN
    from bigcn_amd.data import Batch
    models, batches = {}, []
    for name in ("bigcn", "ebgcn"):
        sd, b, cfg, _ = X.load_fixture(os.path.join(ROOT, "tests", "golden", f"explain_{name}_mixed.npz"))
        F_in = b["x"].size(1)
        if cfg["ebgcn"]:
            model = EBGCN(argparse.Namespace(input_features=F_in, hidden_features=64, output_features=64,
                                             num_class=cfg["num_class"], edge_num=cfg["edge_num"], edge_infer_td=True,
                                             edge_infer_bu=True, device=DEV))
        else:
            model = BiGCN(F_in, 64, 64, DEV)
        model.load_state_dict(sd, strict=True)
        models[name] = model.eval().to(DEV)
        batches.append((b, Batch(num_graphs=len(b["rootindex"]), **b).to(DEV)))
    return models, batches


def test_compare_end_to_end_on_the_explain_fixtures():
    from bigcn_amd import compare, explain
    from bigcn_amd.compare import Similarity
    models, batches = _models_and_batches()
    parts = []
    for b, data in batches:
        batch, B, N = b["batch"].numpy(), len(b["rootindex"]), len(b["batch"])
        x_sum = data.x.sum(-1)
        s = compare(data, models, k=5, extra={"x_sum": x_sum})
        assert s.names[:11] == C.REFERENCE_NAMES and s.names[11:] == ("x_sum",) and s.k == 5
        ex = {name: explain(m, data) for name, m in models.items()}
        rows = [C.centrality_orders(C.centrality(b["edge_index"].numpy(), batch, B), batch, B)]
        for name in ("bigcn", "ebgcn"):
            for d in (ex[name].td, ex[name].bu):
                rows += [d.order[d.stage_names.index(st)].cpu().numpy()[None] for st in ("conv1_output_sum", "conv2_output_sum")]
        rows.append(ex["bigcn"].x_order.cpu().numpy()[None])
        orders = np.concatenate(rows)
        assert orders.shape == (12, N)
        want, want_valid = C.rank_similarity(orders, batch, B, 5)
        got = s.matrix.cpu().numpy()
        assert want_valid.tolist() == (np.bincount(batch) > 5).tolist() and want_valid.sum() >= 3
        assert np.array_equal(s.valid.cpu().numpy(), want_valid)
        assert np.array_equal(_bits(got[:, 2:]), _bits(want[:, 2:]))
        assert float(np.abs(got[:, :2] - want[:, :2]).max()) <= 1e-12
        # Explanation objects instead of models, and the call is deterministic: bit-equal
        again = compare(data, ex, k=5, extra={"x_sum": x_sum})
        assert again.names == s.names and torch.equal(again.matrix.view(torch.int64), s.matrix.view(torch.int64))
        assert torch.equal(again.centrality_order, s.centrality_order)
        parts.append(s)
    fold = Similarity.cat(parts)
    assert fold.matrix.shape[0] == sum(p.matrix.shape[0] for p in parts)
    # ten terms of at most 1 summed in another order: well inside 1e-14; the counts are integers
    assert np.allclose(fold.summarise().cpu().numpy(), C.summarise(fold.matrix.cpu().numpy()), rtol=0, atol=1e-14,
                       equal_nan=True)
    with pytest.raises(ValueError):
        compare(batches[0][1], {"bigcn": models["bigcn"]}, stages=("conv1_output_cat_x_bn1_sum",))


# ------------------------------------------------------------------ refusals
# Each is a small well-formed launch: the kernels report through status and read nothing out of range.
N_REF, B_REF = 9, 2
BATCH_REF = [0, 0, 0, 0, 1, 1, 1, 1, 1]
GOOD_EDGES = [[0, 0, 1, 4, 4, 5], [1, 2, 3, 5, 6, 7]]      # node 8: a second root of tree 1


def _centrality_status(edges, batch=BATCH_REF, B=B_REF):
    from bigcn_amd import ops
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    cent = ops.tree_centrality(torch.tensor(edges, device=DEV), torch.tensor(batch, device=DEV), B, status=status)
    return int(status.item()), cent.cpu().numpy()


def _with(extra):
    return [GOOD_EDGES[0] + [e[0] for e in extra], GOOD_EDGES[1] + [e[1] for e in extra]]


def test_tree_centrality_refusals():
    from bigcn_amd import _lib, tree_centrality
    want = C.centrality(np.array(GOOD_EDGES), np.array(BATCH_REF), B_REF)
    st, cent = _centrality_status(GOOD_EDGES)
    assert st == 0 and np.array_equal(_bits(cent), _bits(want))
    cases = {
        "two parents": (_with([(2, 3)]), _lib.BGCN_STATUS_TWO_PARENTS, ValueError, [0]),
        "3-cycle": ([[0, 0, 1, 5, 6, 7], [1, 2, 3, 6, 7, 5]], _lib.BGCN_STATUS_CYCLE, ValueError, [1]),
        "across trees": (_with([(3, 8)]), _lib.BGCN_STATUS_CROSS_TREE, ValueError, [0, 1]),
        "endpoint N": (_with([(6, N_REF)]), 0, IndexError, [1]),
    }
    for name, (edges, bit, exc, refused) in cases.items():
        st, cent = _centrality_status(edges)
        assert st & 1 and (st & ~1) == bit, name
        for t in range(B_REF):
            in_tree = np.array(BATCH_REF) == t
            if t in refused:
                assert np.all(cent[:, in_tree] == 0), name           # left unwritten (the wrapper's zeros)
            else:
                assert np.array_equal(_bits(cent[:, in_tree]), _bits(want[:, in_tree])), name
        with pytest.raises(exc):
            tree_centrality(torch.tensor(edges, device=DEV), torch.tensor(BATCH_REF, device=DEV), B_REF, validate=True)
    for bad in ([0, 0, 1, 1, 0, 1, 1, 1, 1], [0, 0, 0, 0, 1, 1, 1, 1, 2], [0, 0, 0, -1, 1, 1, 1, 1, 1]):
        st, cent = _centrality_status(GOOD_EDGES, bad)
        assert st & 1 and np.all(cent == 0)
        with pytest.raises(IndexError):
            tree_centrality(torch.tensor(GOOD_EDGES, device=DEV), torch.tensor(bad, device=DEV), B_REF, validate=True)
    st, cent = _centrality_status(GOOD_EDGES)                          # and still works after
    assert st == 0 and np.array_equal(_bits(cent), _bits(want))


def test_compare_raises_on_a_bad_tree():
    from bigcn_amd import compare
    with pytest.raises(ValueError, match="more than one incoming edge"):
        compare(_data(np.array(_with([(2, 3)])), np.array(BATCH_REF), B_REF), {}, k=2)
    with pytest.raises(IndexError):
        compare(_data(np.array(GOOD_EDGES), np.array([0, 0, 1, 1, 0, 1, 1, 1, 1]), B_REF), {}, k=2)


def test_rank_similarity_refuses_a_list_that_repeats_an_index():
    from bigcn_amd import ops, rank_similarity
    batch = torch.tensor(BATCH_REF, device=DEV)
    good = [[3, 1, 0, 2, 4, 2, 0, 1, 3], [0, 1, 2, 3, 0, 1, 2, 3, 4]]
    orders = torch.tensor(good, dtype=torch.int32, device=DEV)
    sim, valid = rank_similarity(orders, batch, 3, B_REF)
    want, want_valid = C.rank_similarity(np.array(good), np.array(BATCH_REF), B_REF, 3)
    assert np.array_equal(_bits(sim.cpu().numpy()[:, 2:]), _bits(want[:, 2:])) and valid.cpu().tolist() == [True, True]
    for value in (4, 7):       # tree 1's first list starts [4, 2, 0]: a repeat; an index outside the tree's 5 nodes
        bad = [good[0][:5] + [value] + good[0][6:], good[1]]
        orders = torch.tensor(bad, dtype=torch.int32, device=DEV)
        with pytest.raises(ValueError, match="not a ranking"):
            rank_similarity(orders, batch, 3, B_REF)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        sim, valid = ops._rank_similarity(orders, batch, 3, B_REF, status)
        assert int(status.item()) == 2 and valid.cpu().tolist() == [1, 0]
        sim = sim.cpu().numpy()
        assert np.all(np.isnan(sim[1])) and np.array_equal(_bits(sim[0, 2:]), _bits(want[0, 2:]))
    # a repeat past the first k is not looked at
    late = [good[0][:7] + [0, 0], good[1]]
    sim, valid = rank_similarity(torch.tensor(late, dtype=torch.int32, device=DEV), batch, 3, B_REF)
    assert np.array_equal(_bits(sim.cpu().numpy()[:, 2:]), _bits(want[:, 2:]))
    with pytest.raises(IndexError):
        rank_similarity(orders, torch.tensor([0, 0, 1, 1, 0, 1, 1, 1, 1], device=DEV), 3, B_REF)
