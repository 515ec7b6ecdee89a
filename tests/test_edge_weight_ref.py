"""CPU self-check of tests/edge_weight_ref.py: the restated formula of d edge_weight agrees with
autograd through the oracle's gcn_conv, the exact class is exact (a round trip through fp32 and
any summation order in fp32 leave the result unchanged), and every mutant of the formula shows on
the very inputs tests/test_gpu_edge_weight.py uses - so its torch.equal fails for a kernel with a
wrong degree key, a missing term or a feature loop that stops after one trip."""
import numpy as np
import pytest
import torch

import edge_weight_ref as R
from oracle import bigcn_oracle as O


def autograd_dw(ei, w, N, degree_on, h, dout):
    """d <dout, gcn_conv(h, identity weight, edge_weight = w)> / d w by autograd, float64."""
    wt = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    x = torch.tensor(h, dtype=torch.float64)
    out = O.gcn_conv(x, torch.tensor(ei), torch.eye(x.size(1), dtype=torch.float64), None,
                     edge_weight=wt, degree_on=degree_on)
    out.backward(torch.tensor(dout, dtype=torch.float64))
    return out.detach().numpy(), wt.grad.numpy()


# At a node of degree 0 autograd returns NaN: deg.pow(-0.5) is inf there, the masked_fill stops
# the value but its backward multiplies a zero gradient by pow's inf slope (0 * inf).  The kernel
# documents 0 (dL/ddeg = 0 where dis = 0), so that case is pinned by the formula alone
# (test_zero_degree_follows_the_formula) and the comparison below keeps every degree positive.
@pytest.mark.parametrize("degree_on", ["col", "row"])
@pytest.mark.parametrize("F", [8, 70])
@pytest.mark.parametrize("star", [False, True])
def test_formula_agrees_with_autograd(degree_on, F, star):
    rng = np.random.default_rng(5 + F + star)
    ei, w, N, h, dout = R.general_case(rng, [1, 2, 7, 40, 90], F, star=star)   # a loop and a duplicate
    p = R.ew_parts_ref(ei, w, N, degree_on, h, dout)
    assert int(p["loop"].sum()) == 1 and bool((p["deg"] > 0).all())
    assert (ei[:, -2] == ei[:, 0]).all() and w[-2] != w[0]
    out, dw = autograd_dw(ei, w, N, degree_on, h, dout)
    assert np.abs(p["agg"] - out).max() <= 1e-12 * np.abs(out).max()
    assert np.abs(p["dw"] - dw).max() <= 1e-12 * np.abs(dw).max()
    assert np.abs(dw).min() > 0


def test_autograd_is_nan_at_a_zero_degree():
    ei, w = np.array([[0, 1], [1, 2]]), np.array([-1.0, 0.5])        # deg[1] = -1 + 1 under 'col'
    h, dout = np.ones((3, 4)), np.ones((3, 4))
    assert np.isnan(autograd_dw(ei, w, 3, "col", h, dout)[1]).any()


def test_zero_degree_follows_the_formula():
    ei, w = np.array([[0, 1, 1], [1, 2, 0]]), np.array([-1.0, 0.5, 0.25])
    rng = np.random.default_rng(0)
    h, dout = rng.standard_normal((3, 8)), rng.standard_normal((3, 8))
    p = R.ew_parts_ref(ei, w, 3, "col", h, dout)
    assert p["dis"][1] == 0 and not p["agg"][1].any() and p["dldeg"][1] == 0 and p["lgrad"][1] == 0
    assert np.isfinite(p["dw"]).all()
    # edge 0 ends at the dead node: no direct term, no degree term; edge 1 leaves it: no direct term
    assert p["dw"][0] == 0 and p["dw"][1] == p["dldeg"][2] != 0


def test_out_of_range_and_loops():
    ei = np.array([[0, 9, 1, 2, 2, -1], [1, 0, 2, 2, 2, 1]])
    w = np.array([0.5, 7.0, 0.25, 3.0, 5.0, 2.0])
    g = R.gcn_norm_ref(ei, w, 3, "col")
    assert g["valid"].tolist() == [True, False, True, True, True, False]
    assert g["lw"].tolist() == [1.0, 1.0, 5.0]                       # the later loop's weight
    assert g["deg"].tolist() == [1.0, 1.5, 5.25]
    rng = np.random.default_rng(1)
    h, dout = rng.standard_normal((3, 4)), rng.standard_normal((3, 4))
    dw = R.ew_grad_ref(ei, w, 3, "col", h, dout)
    assert dw[1] == 0 and dw[5] == 0
    keep = [0, 2, 4]                                                 # the same graph without them
    assert np.array_equal(dw[keep], R.ew_grad_ref(ei[:, keep], w[keep], 3, "col", h, dout))
    c = R.csr_ref(ei, w, 3, "col")
    assert c["t_ptr"].tolist() == [0, 1, 3, 5] and c["t_col"].tolist() == [0, 0, 1, 1, 2]
    assert c["s_ptr"].tolist() == [0, 2, 4, 5] and c["s_col"].tolist() == [1, 0, 2, 1, 2]


# ------------------------------------------------------------------------- the exact class
EXACT = [(d, F, loop) for d in ("col", "row") for F in R.GPU_WIDTHS for loop in R.GPU_LOOPS]
EXACT_IDS = [f"{d}-{F}-{loop}" for d, F, loop in EXACT]


def test_exact_graphs_are_as_described():
    for degree_on in ("col", "row"):
        for loop in R.GPU_LOOPS:
            ei, w, N, h, dout, p = R.gpu_exact_case(degree_on, R.F_MAX, loop)
            assert set(np.unique(p["deg"])) <= {1.0, 4.0, 16.0}, np.unique(p["deg"])
            assert {1.0, 4.0, 16.0} == set(np.unique(p["deg"]))
            assert (w == np.round(w)).all() and (w == 0).sum() == 1 and w.min() == 0
            assert np.abs(h).max() == R.VMAX == np.abs(dout).max()
            assert (np.bincount(np.concatenate([ei[0], ei[1]]), minlength=N) == 0).sum() == 3   # isolated
            assert int(p["loop"].sum()) == (loop is not None)
            if loop:
                k = int(ei[0][p["loop"]][0])
                assert p["lw"][k] > 1 and p["deg"][k] in (4.0, 16.0)
                e = int(np.flatnonzero(p["loop"])[0])
                inside = e + 1 < ei.shape[1] and k in ei[:, e + 1]
                assert inside == (loop == "inside") and (e == ei.shape[1] - 1) == (loop == "tail")
    # the stars of the build test: unit weights, degree 256 and 1024 under 'row'
    for n in (256, 1024):
        ei, w, N = R.exact_graph(np.random.default_rng(n), [n], "row", star=True, max_children=None,
                                 zero_weight=False, unit=True)
        g = R.gcn_norm_ref(ei, w, N, "row")
        assert (w == 1).all() and g["deg"][0] == n and g["dis"][0] == n ** -0.5


@pytest.mark.parametrize("degree_on,F,loop", EXACT, ids=EXACT_IDS)
def test_exact_class_is_exact(degree_on, F, loop):
    ei, w, N, h, dout, p = R.gpu_exact_case(degree_on, F, loop)       # (asserts the class's bound)
    assert np.abs(p["dw"]).max() > 0
    for k in ("dw", "agg", "dz", "dis", "norm", "loop_norm"):
        assert np.array_equal(p[k].astype(np.float32).astype(np.float64), p[k]), k
    # fp32 arithmetic, every sum in a random order: the same bits
    for seed in range(2):
        q = R.ew_parts_ref(ei, w, N, degree_on, h, dout, dtype=np.float32, rng=np.random.default_rng(seed))
        for k in ("dw", "agg", "dz"):
            assert q[k].dtype == np.float32 and np.array_equal(q[k], p[k].astype(np.float32)), k


def test_general_class_is_not_exact():
    """The same check tells the classes apart: fp32 arithmetic moves the general class."""
    ei, w, N, h, dout = R.general_case(np.random.default_rng(2), R.GPU_SIZES, 68)
    p = R.ew_parts_ref(ei, w, N, "col", h, dout)
    q = R.ew_parts_ref(ei, w, N, "col", h, dout, dtype=np.float32)
    assert not np.array_equal(q["dw"], p["dw"].astype(np.float32))
    with pytest.raises(AssertionError):
        R.ew_parts_ref(ei, w, N, "col", h, dout, exact=True)


@pytest.mark.parametrize("degree_on,F,loop", EXACT, ids=EXACT_IDS)
def test_each_mutant_is_seen(degree_on, F, loop):
    ei, w, N, h, dout, p = R.gpu_exact_case(degree_on, F, loop)
    want = p["dw"].astype(np.float32)
    for m in R.MUTANTS:
        got = R.ew_grad_ref(ei, w, N, degree_on, h, dout, mutant=m).astype(np.float32)
        differs = not np.array_equal(got, want)
        if m == "loop_as_edge":
            # the loop line of the formula is the kept-edge line at s = d = k: no input can tell
            assert not differs
        elif m.startswith("loop"):
            assert differs == (loop is not None), m
            if loop:
                assert got[p["loop"]] != want[p["loop"]], m
        elif m == "cols_lt_64":
            assert differs == (F > 64), m
        else:
            assert differs, m
            assert (got != want).mean() > 0.5, m
