"""Host-side API contracts that need no GPU: argument validation of the drop-in
modules and the fused step (no kernel is launched)."""
import pytest
import torch

from bigcn_amd import BiGCN, GCNConv, Net
from bigcn_amd.ops import degree_code


def test_degree_on_values_are_validated():
    assert degree_code("col") == 0 and degree_code("row") == 1
    for bad in ("rows", "COL", "target", ""):
        with pytest.raises(ValueError):
            degree_code(bad)
        with pytest.raises(ValueError):
            GCNConv(8, 4, degree_on=bad)
        with pytest.raises(ValueError):
            BiGCN(8, 64, 64, degree_on=bad)


def test_degree_on_is_model_wide():
    m = Net(16, 64, 64, degree_on="row")
    assert m.degree_on == "row"
    convs = (m.TDrumorGCN.conv1, m.TDrumorGCN.conv2, m.BUrumorGCN.conv1, m.BUrumorGCN.conv2)
    assert all(c.degree_on == "row" for c in convs)
    m.degree_on = "col"
    assert all(c.degree_on == "col" for c in convs)
    with pytest.raises(ValueError):
        m.degree_on = "source"
    m.TDrumorGCN.conv2.degree_on = "row"          # edited behind the model's back
    with pytest.raises(ValueError, match="disagree"):
        _ = m.degree_on


def test_fused_step_takes_the_models_degree_convention():
    from bigcn_amd import FusedTrainStep
    m = BiGCN(16, 64, 64, degree_on="row")
    assert FusedTrainStep(m).degree_on == 1
    assert FusedTrainStep(m, degree_on="row").degree_on == 1
    with pytest.raises(ValueError, match="model"):
        FusedTrainStep(m, degree_on="col")


def _cpu_batch(dtype=torch.float32, awkward=False):
    """Trees of 1, 2 and 40 nodes, F = 16; awkward: the index tensors arrive as int32
    (batch, edge_index) or non-contiguous (rootindex, BU_edge_index) and must be converted."""
    import numpy as np
    from bigcn_amd.data import synth_batch
    b = synth_batch(np.random.default_rng(3), [1, 2, 40], 16, 4, 0.0, 0.0, dtype=dtype)
    if awkward:
        b.batch, b.edge_index = b.batch.to(torch.int32), b.edge_index.to(torch.int32)
        b.rootindex = torch.stack([b.rootindex, b.rootindex], 1)[:, 0]
        b.BU_edge_index = b.BU_edge_index.t().contiguous().t()
        assert not b.rootindex.is_contiguous() and not b.BU_edge_index.is_contiguous()
    return b


def _dense_fields(d):
    return {k: getattr(d, k) for k in ("x", "ldx", "num_nodes", "num_graphs", "x_dtype", "batch", "rootindex",
                                       "td_edge_index", "td_num_edges", "bu_edge_index", "bu_num_edges")}


@pytest.mark.parametrize("case", ["fp32", "bf16", "converted"])
def test_dense_batch_descriptor(case):
    """ops.dense_batch_desc (the one place a dense batch's bgcn_batch is filled, for the fused
    step and prepare_batch alike): every field, and the keep-alive tuple owns every pointer."""
    from bigcn_amd import _lib
    from bigcn_amd.ops import dense_batch_desc
    b = _cpu_batch(torch.bfloat16 if case == "bf16" else torch.float32, awkward=case == "converted")
    d, keep = dense_batch_desc(b)
    x, td, bu, batch, root = keep
    assert _dense_fields(d) == {
        "x": x.data_ptr(), "ldx": 16, "num_nodes": 43, "num_graphs": 3,
        "x_dtype": _lib.BGCN_DTYPE_BF16 if case == "bf16" else _lib.BGCN_DTYPE_F32,
        "batch": batch.data_ptr(), "rootindex": root.data_ptr(),
        "td_edge_index": td.data_ptr(), "td_num_edges": 40, "bu_edge_index": bu.data_ptr(), "bu_num_edges": 40}
    assert (d.td_droprate, d.bu_droprate, d.drop_seed) == (0.0, 0.0, 0)
    assert not d.x_row_ptr and not d.x_col and not d.x_val
    assert x.dtype == b.x.dtype and x.is_contiguous() and x.shape == (43, 16)
    for t, src in ((td, b.edge_index), (bu, b.BU_edge_index), (batch, b.batch), (root, b.rootindex)):
        assert t.dtype == torch.int64 and t.is_contiguous() and torch.equal(t, src.to(torch.int64))
        assert (t is src) == (case != "converted")     # converted only when it has to be
    assert x.data_ptr() == b.x.data_ptr()


def test_fused_step_desc_is_the_dense_descriptor_plus_dropedge():
    """FusedTrainStep._desc = dense_batch_desc + the DropEdge fields: batch k described with
    drop=True under model.training and a non-zero rate uses drop seed drop_seed + k; no draw
    (and no increment) with drop=False, in eval mode, or with both rates 0."""
    from bigcn_amd import FusedTrainStep
    from bigcn_amd.ops import dense_batch_desc
    b = _cpu_batch()
    want = _dense_fields(dense_batch_desc(b)[0])
    m = BiGCN(16, 64, 64)
    st = FusedTrainStep(m, tddroprate=0.25, budroprate=0.5, drop_seed=2**64 - 2)
    m.train()
    seeds = []
    for drop, training in ((True, True), (False, True), (True, False), (True, True), (True, True)):
        m.train(training)
        d, keep = st._desc(b) if drop else st._desc(b, drop=False)
        assert _dense_fields(d) == want and len(keep) == 5 and keep[0].data_ptr() == b.x.data_ptr()
        if drop and training:
            assert (d.td_droprate, d.bu_droprate) == (0.25, 0.5)
            seeds.append(int(d.drop_seed))
        else:
            assert (d.td_droprate, d.bu_droprate, d.drop_seed) == (0.0, 0.0, 0)
    assert seeds == [2**64 - 2, 2**64 - 1, 0] and st._drop_count == 3      # (the seed wraps at 2^64)
    m.train()
    plain = FusedTrainStep(m)
    d, _ = plain._desc(b)
    assert (d.td_droprate, d.bu_droprate, d.drop_seed) == (0.0, 0.0, 0) and plain._drop_count == 0
    b.rootindex = b.rootindex[:2]
    with pytest.raises(ValueError, match="one entry per tree"):
        st._desc(b)


def test_fused_step_bucket_carries_the_status_slot():
    """Layout [early gradients | status slot | conv1 weight gradients]: part a (flat_a)
    holds every gradient the deferred-dW1 step finishes first and the status slot, part b
    (flat_b) exactly the two conv1 weight gradients."""
    from bigcn_amd import FusedTrainStep
    m = BiGCN(16, 64, 64)
    st = FusedTrainStep(m)
    b = st.bucket
    n = sum(p.numel() for p in m.parameters())
    assert b.flag.numel() == 1
    assert b.flat_a.numel() + b.flat_b.numel() == b.flat.numel()
    assert b.flat_a.data_ptr() <= b.flag.data_ptr() < b.flat_a.data_ptr() + 4 * b.flat_a.numel()
    enc = list(m.encoder_params())
    late = {id(enc[0]), id(enc[4])}
    lo, hi = b.flat_b.data_ptr(), b.flat_b.data_ptr() + 4 * b.flat_b.numel()
    for p, v in zip(b.params, b.views()):
        inside = lo <= v.data_ptr() < hi
        assert inside == (id(p) in late), tuple(p.shape)
    assert b.flat_b.numel() == enc[0].numel() + enc[4].numel()
    assert sum(v.numel() for v in b.views()) == n


def test_bucket_views_are_16_byte_aligned():
    """Net's 2-class head bias would misalign every later view of a packed bucket: the
    views start on 16-byte boundaries (float4 paths of the step and the fused Adam), the
    gaps stay zero, reduce_sum fills the views."""
    from bigcn_amd import FusedTrainStep, Net
    m = Net(16, 64, 64)
    st = FusedTrainStep(m)
    b = st.bucket
    assert all(v.data_ptr() % 16 == 0 for v in b.views())
    for p in b.params:
        p.grad = torch.full_like(p, 2.0)
    views = b.reduce_sum()
    assert all(bool((v == 2.0).all()) for v in views)
    assert float(b.flat.sum()) - float(b.flag.sum()) == 2.0 * sum(p.numel() for p in b.params)
