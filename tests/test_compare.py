"""CPU checks of the compare path: the numpy restatement (tests/compare_ref.py) reproduces what
networkx and scipy computed (fixtures of tools/gen_compare_golden.py, and live where the two import),
the name list is the reference's, Similarity's host side (summarise, cat, centrality_dict) follows
compare_similarity.py, and the new C entry points refuse bad arguments before any device work."""
import glob
import json
import os

import numpy as np
import pytest
import torch

import compare_ref as C
import explain_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "compare_*.npz")))
NAMES = [os.path.basename(p)[len("compare_"):-len(".npz")] for p in FIXTURES]
ULP2, cases_of, similarity_bar = C.ULP2, C.cases_of, C.similarity_bar
def test_fixture_set():
    from bigcn_amd import _lib
    assert NAMES == ["forest", "lists", "long", "mixed"]
    for p in FIXTURES:
        assert os.path.getsize(p) < 200 * 1024
    z = np.load(FIXTURES[NAMES.index("long")])
    n = np.bincount(z["batch"])
    assert n.tolist() == [_lib.BGCN_TREE_CENTRALITY_LDS + 5, 12, _lib.BGCN_TREE_CENTRALITY_LDS + 5]
    z = np.load(FIXTURES[NAMES.index("mixed")])
    assert np.bincount(z["batch"], minlength=int(z["num_graphs"])).tolist() == [1, 2, 3, 0, 41, 70, 33]
    z = np.load(FIXTURES[NAMES.index("lists")])
    assert sorted({int(k) for k, _ in z["cases"]}) == [2, 5, 10, 32]
    assert sorted({int(v) for _, v in z["cases"]}) == [1, 15, 32]
    n = set(np.bincount(z["batch"]).tolist())
    assert all({k, k + 1} <= n for k in (2, 5, 10, 32))        # a skipped and a kept tree for every k


@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_restatement_matches_networkx_and_scipy_fixture(path):
    z = np.load(path)
    ei, batch, B = z["edge_index"], z["batch"], int(z["num_graphs"])
    cent = C.centrality(ei, batch, B)
    nxc = z["nx_centrality"]
    assert cent.dtype == np.float32 and cent.shape == nxc.shape == (3, len(batch))
    zero = nxc == 0
    assert np.all(cent[zero] == 0)
    rel = np.abs(cent[~zero].astype(np.float64) - nxc[~zero]) / np.abs(nxc[~zero])
    print(f"closed form vs networkx: max relative {rel.max():.3e}")
    assert rel.max() <= ULP2
    assert np.array_equal(C.centrality_orders(cent, batch, B), z["order"])
    assert np.array_equal(z["orders"][:3], z["order"])
    bar = similarity_bar(z)
    for k, V, sim, valid, summary in cases_of(z):
        got, got_valid = C.rank_similarity(z["orders"][:V], batch, B, k)
        assert np.array_equal(got_valid, valid) and got.shape == sim.shape == (B, 5, V, V)
        err = float(np.abs(got - sim).max())
        print(f"k={k} V={V}: max |restatement - scipy| {err:.3e} (recorded {float(z['restatement_err']):.3e})")
        assert err <= bar
        assert np.all(sim[~valid] == 0) and np.all(got[~valid] == 0)
        assert np.allclose(C.summarise(sim), summary, rtol=0, atol=0, equal_nan=True)
    # the lists hold what their builder promises: identical, reversed and disjoint top-k lists
    if "cases" in z.files:
        p = X.tree_ptr(batch, B)
        o = z["orders"]
        a = int(p[np.bincount(batch).tolist().index(64)])
        assert np.array_equal(o[3], o[0]) and not set(o[0, a:a + 32]) & set(o[4, a:a + 32])
        assert np.array_equal(o[6, a:a + 5], o[0, a:a + 5][::-1])


def _random_forest(rng, n, drop):
    e = [(int(rng.integers(0, i)), i) for i in range(1, n)]
    perm = rng.permutation(n)
    e = [(int(perm[a]), int(perm[b])) for a, b in e if rng.random() >= drop]
    return np.array(e, dtype=np.int64).reshape(-1, 2).T


def test_closed_forms_match_networkx_live():
    nx = pytest.importorskip("networkx")
    rng = np.random.default_rng(3)
    worst = 0.0
    for trial in range(50):
        n = int(rng.choice([1, 2, 3, 9, 40]))
        ei = _random_forest(rng, n, 0.3 if trial % 3 == 0 else 0.0)
        g = nx.DiGraph()
        g.add_nodes_from(range(n))
        g.add_edges_from(ei.T.tolist())
        want = np.array([[f(g)[v] for v in range(n)] for f in
                         (nx.out_degree_centrality, nx.betweenness_centrality, nx.closeness_centrality)])
        c, d, s, nn = C.tree_integers(ei, np.zeros(n, dtype=np.int64), 1)
        n1 = max(n - 1, 1)
        exact = np.array([c / n1 if n > 1 else np.ones(n), d * (s - 1) / max(n1 * (n - 2), 1),
                          2 * d / ((d + 1) * n1)], dtype=np.float64)
        worst = max(worst, float(np.abs(exact - want).max()))
        got = C.centrality(ei, np.zeros(n, dtype=np.int64), 1)
        assert np.all(np.abs(got - want) <= ULP2 * np.abs(want)), trial
    print(f"closed forms (fp64) vs networkx: max abs {worst:.3e}")
    assert worst <= 1e-15


def test_tie_free_identities_match_scipy_live():
    st = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(4)
    for k in (2, 5, 10, 32):
        for _ in range(5):
            x, y = rng.permutation(3 * k)[:k].tolist(), rng.permutation(3 * k)[:k].tolist()
            m = C.pair_metrics(x, y)
            tau_b = st.kendalltau(x, y)[0]
            tau_a = sum(np.sign(x[a] - x[b]) * np.sign(y[a] - y[b]) for a in range(k) for b in range(a)) / (k * (k - 1) / 2)
            assert abs(tau_b - tau_a) <= 1e-15 and abs(st.somersd(x, y).statistic - tau_a) <= 1e-15
            assert m[2] == m[3] and abs(m[2] - tau_a) <= 1e-15
            assert abs(m[0] - st.pearsonr(x, y)[0]) <= 1e-12 and abs(m[1] - st.spearmanr(x, y)[0]) <= 1e-12
            assert np.array_equal(C.pair_metrics(y, x), m)          # symmetric bit for bit
    assert np.array_equal(C.pair_metrics([4, 1, 7], [4, 1, 7]), np.ones(5))
    assert C.pair_metrics([1, 2, 3], [3, 2, 1])[:4].tolist() == [-1.0] * 4
    assert C.pair_metrics([1, 2, 3], [4, 5, 6])[4] == 0.0


def test_names_are_the_references():
    from bigcn_amd.compare import CENTRALITY_NAMES, METRIC_NAMES, ranking_names
    assert CENTRALITY_NAMES == C.CENTRALITY_NAMES == C.REFERENCE_NAMES[:3]
    assert METRIC_NAMES == C.METRIC_NAMES
    assert ranking_names(("bigcn", "ebgcn")) == C.REFERENCE_NAMES
    names = ranking_names(("bigcn", "ebgcn"), extra=("maxbert_hidden", "maxbert_attn"))
    assert names[:11] == C.REFERENCE_NAMES and names[11:] == ("maxbert_hidden", "maxbert_attn")
    assert ranking_names(("m",), stages=("conv2_output_sum",)) == C.CENTRALITY_NAMES + ("m_td_conv2", "m_bu_conv2")
    with pytest.raises(ValueError):
        ranking_names(("bigcn", "bigcn"))


def _similarity(mat, names=("a", "b"), k=2, **kw):
    from bigcn_amd.compare import Similarity
    mat = torch.as_tensor(mat, dtype=torch.float64)
    return Similarity(names, mat, mat.abs().sum((1, 2, 3)) > 0, k, **kw)


def test_summarise_counts_nonzero_entries_only():
    mat = np.zeros((4, 5, 2, 2))
    mat[0, :, 0, 1], mat[1, :, 0, 1], mat[3, :, 0, 1] = 0.5, -0.25, 0.0       # tree 2 skipped, tree 3 an exact 0
    mat[0, :, 1, 1] = mat[1, :, 1, 1] = 1.0
    s = _similarity(mat).summarise().numpy()
    assert s.shape == (5, 2, 2)
    assert np.all(s[:, 0, 1] == 0.125) and np.all(s[:, 1, 1] == 1.0)            # 0.25 / 2, not / 3 or / 4
    assert np.all(np.isnan(s[:, 0, 0])) and np.all(np.isnan(s[:, 1, 0]))        # 0 / 0
    assert np.array_equal(s, C.summarise(mat), equal_nan=True)


def test_similarity_cat():
    from bigcn_amd.compare import Similarity
    rng = np.random.default_rng(0)
    a, b = _similarity(rng.random((3, 5, 2, 2))), _similarity(rng.random((2, 5, 2, 2)))
    both = Similarity.cat([a, b])
    assert both.matrix.shape == (5, 5, 2, 2) and both.valid.shape == (5,) and both.k == 2 and both.names == a.names
    assert torch.equal(both.matrix[3:], b.matrix) and both.centrality is None
    assert torch.allclose(both.summarise(), torch.cat([a.matrix, b.matrix]).mean(0), rtol=1e-14, atol=0)
    with pytest.raises(ValueError):
        Similarity.cat([a, _similarity(rng.random((2, 5, 2, 2)), k=3)])
    with pytest.raises(ValueError):
        Similarity.cat([a, _similarity(rng.random((2, 5, 2, 2)), names=("a", "c"))])
    with pytest.raises(ValueError):
        Similarity.cat([])
    with pytest.raises(ValueError):
        both.centrality_dict(0)


def test_centrality_dict_is_the_record_the_reference_reads():
    z = np.load(FIXTURES[NAMES.index("mixed")])
    batch, B = z["batch"], int(z["num_graphs"])
    cent = C.centrality(z["edge_index"], batch, B)
    order, srt = X.segment_rank(cent, batch, B)
    s = _similarity(np.zeros((B, 5, 3, 3)), names=C.CENTRALITY_NAMES, centrality=torch.from_numpy(cent),
                    centrality_order=torch.from_numpy(order), centrality_sorted=torch.from_numpy(srt),
                    batch=torch.from_numpy(batch))
    rec = s.centrality_dict(4)                                   # the 40-leaf star
    assert list(rec) == ["out_degree", "betweenness", "closeness"]
    assert json.loads(json.dumps(rec)) == rec
    root = int(z["edge_index"][0][np.isin(z["edge_index"][0], np.nonzero(batch == 4)[0])][0]) - 6
    assert rec["out_degree"][0][0] == root and rec["out_degree"][1][:2] == [1.0, 0.0]
    leaves = [i for i in range(41) if i != root]
    assert rec["out_degree"][0][1:] == leaves                    # ties by ascending node index
    assert rec["closeness"][0] == leaves + [root]
    assert s.centrality_dict(3) == {n: [[], []] for n in C.CENTRALITY_NAMES}     # the id without nodes
    with pytest.raises(IndexError):
        s.centrality_dict(B)


def test_exports():
    import bigcn_amd
    from bigcn_amd import _lib, ops
    from bigcn_amd.compare import Similarity, compare, rank_similarity, tree_centrality   # noqa: F401
    for name in ("compare", "tree_centrality", "rank_similarity"):
        assert name in bigcn_amd.__all__ and callable(getattr(bigcn_amd, name))
    for name in ("bgcn_tree_centrality_workspace_size", "bgcn_tree_centrality", "bgcn_rank_similarity_workspace_size",
                 "bgcn_rank_similarity"):
        assert name in _lib.EXPORTED_SYMBOLS and name in _lib._SIGS
    text = open(os.path.join(ROOT, "include", "bgcn.h")).read()
    for name in ("BGCN_TREE_CENTRALITY_LDS", "BGCN_RANK_SIMILARITY_MAX", "BGCN_STATUS_TWO_PARENTS", "BGCN_STATUS_CYCLE"):
        assert f"#define {name} {getattr(_lib, name)}\n" in text
    assert ops.TREE_CENTRALITY_LDS == _lib.BGCN_TREE_CENTRALITY_LDS
    # seven int32 arrays per node within 64 KiB of LDS: two workgroups per CU
    assert 7 * 4 * _lib.BGCN_TREE_CENTRALITY_LDS <= 64 * 1024
    lib = _lib.load_library()
    assert lib.bgcn_abi_version() == 12
    assert lib.bgcn_tree_centrality_workspace_size(100, 8) >= 4 * (8 * 100 + 2 * 8 + 2)
    assert lib.bgcn_tree_centrality_workspace_size(1000, 8) > lib.bgcn_tree_centrality_workspace_size(100, 8)
    assert lib.bgcn_rank_similarity_workspace_size(8) >= 4 * 10
    assert lib.bgcn_tree_centrality_workspace_size(-1, 8) == 0 and lib.bgcn_rank_similarity_workspace_size(-1) == 0


def test_invalid_arguments_fail_before_any_device_work():
    """Fake 16-byte-aligned addresses stand for the device pointers: a refused call never reads them."""
    from bigcn_amd import _lib
    lib = _lib.load_library()
    fake = 0x10000

    def cent(ei=fake, E=9, batch=fake + 0x100, N=10, B=2, out=fake + 0x200, ld=10, status=fake + 0x300,
             ws=fake + 0x1000, ws_bytes=1 << 20):
        return lib.bgcn_tree_centrality(ei, E, batch, N, B, out, ld, status, ws, ws_bytes, None)

    def sim(orders=fake, ld=10, V=3, batch=fake + 0x100, N=10, B=2, k=5, out=fake + 0x200, valid=fake + 0x300,
            status=fake + 0x400, ws=fake + 0x1000, ws_bytes=1 << 20):
        return lib.bgcn_rank_similarity(orders, ld, V, batch, N, B, k, out, valid, status, ws, ws_bytes, None)

    def refused(rc, text):
        assert rc == -1
        assert text in lib.bgcn_last_error(), lib.bgcn_last_error()

    for kw in (dict(N=-1), dict(B=-1), dict(E=-1)):
        refused(cent(**kw), b"negative size")
    for kw in (dict(ei=None), dict(batch=None), dict(out=None), dict(status=None)):
        refused(cent(**kw), b"null pointer")
    refused(cent(B=0), b"nodes without a tree")
    refused(cent(ld=9), b"leading dimension")
    refused(cent(ws=None), b"workspace too small")
    refused(cent(ws_bytes=lib.bgcn_tree_centrality_workspace_size(10, 2) // 2), b"workspace too small")
    assert cent(N=0, E=0, ei=None, batch=None, out=None) == 0          # nothing to do

    for kw in (dict(N=-1), dict(B=-1)):
        refused(sim(**kw), b"negative size")
    for k in (1, 33, 0, -5):
        refused(sim(k=k), b"k must be in [2, 32]")
    for V in (0, 33, -1):
        refused(sim(V=V), b"must be in [1, 32]")
    for kw in (dict(orders=None), dict(batch=None), dict(out=None), dict(valid=None), dict(status=None)):
        refused(sim(**kw), b"null pointer")
    refused(sim(ld=9), b"leading dimension")
    refused(sim(N=1 << 26, ld=1 << 26), b"too many nodes")
    refused(sim(ws=None), b"workspace too small")
    refused(sim(ws_bytes=8), b"workspace too small")
    assert sim(B=0, N=0, ld=0) == 0
