"""GPU parity of the fused evaluation step (FusedTrainStep.evaluate -> bgcn_eval_step): the
reference's test loop body (model/Twitter/BiGCN_Twitter.py:207-222: model.eval(); val_out =
model(Batch_data); val_loss = F.nll_loss(val_out, y); _, val_pred = val_out.max(dim=1);
correct = val_pred.eq(y).sum()) on the device with no host sync.

Tolerance: the fp32 HIP path vs the fp64 oracle, |a - b| <= 1e-4 * max|b| per tensor (log-
probabilities, loss); predictions and the correct count exactly (the argmax of the oracle's
log-probabilities, where no two classes are within the tolerance of each other)."""
import numpy as np
import pytest
import torch

from conftest import golden_batch, golden_params, load_golden
from oracle import bigcn_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-4
EVAL_GOLDEN = ["bigcn_eval_mixed.npz", "bigcn_eval_stars_rowdeg.npz", "bigcn_eval_single.npz"]


def close(a, b, tol=TOL, what=""):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = float(b.abs().max()) if b.numel() else 1.0
    err = float((a - b).abs().max()) if b.numel() else 0.0
    assert err <= tol * max(scale, 1e-12), f"{what}: max err {err:.3e} vs scale {scale:.3e}"


def _model(p, F, classes=4, degree_on="col", feat_mode="auto"):
    from bigcn_amd import BiGCN, Net
    m = (BiGCN if classes == 4 else Net)(F, 64, 64).to(DEV)
    m.load_state_dict({k: torch.as_tensor(v).float() for k, v in p.items()})
    m.degree_on = degree_on
    m.feat_mode = feat_mode
    return m


def _check_argmax(pred, correct, rlogp, y):
    """pred must be the oracle's argmax wherever the oracle's top two classes are further
    apart than the log-probabilities' tolerance; where they are within it (a near-tie) any
    class within the tolerance of the maximum is right.  correct counts pred == y."""
    rl = torch.as_tensor(rlogp).double().cpu()
    pred = pred.cpu()
    tol = 2 * TOL * float(rl.abs().max())
    top = rl.max(1).values
    chosen = rl.gather(1, pred.view(-1, 1)).view(-1)
    assert bool(((top - chosen) <= tol).all()), (pred, rl.argmax(1))
    near = (rl >= (top - tol).view(-1, 1)).sum(1) > 1
    want = rl.argmax(1)
    assert torch.equal(pred[~near], want[~near]), (pred, want)
    assert int(correct) == int((pred == y.cpu()).sum())


@pytest.mark.parametrize("mode", ["auto", "dense"])
@pytest.mark.parametrize("name", EVAL_GOLDEN)
def test_eval_step_matches_golden(name, mode):
    from bigcn_amd import FusedTrainStep
    g = load_golden(name)
    assert not bool(g["training"])
    b = golden_batch(g, DEV)
    p = golden_params(g)
    m = _model(p, int(g["in_feats"]), degree_on=str(g["degree_on"]), feat_mode=mode)
    m.train()      # evaluate() runs eval semantics whatever the module's mode
    st = FusedTrainStep(m, tddroprate=0.2, budroprate=0.2, drop_seed=1)
    logp = torch.empty(b.num_graphs, 4, device=DEV)
    loss, correct, pred = st.evaluate(b, logp=logp, pred=True)
    torch.cuda.synchronize()
    st.check_status()
    close(logp, g["logp"], what="logp")
    close(loss, g["loss"], what="loss")
    _check_argmax(pred, correct, g["logp"], b.y)


def _oracle_eval(b, p, degree_on="col"):
    batch = {"x": b.x.double().cpu(), "edge_index": b.edge_index.cpu(), "BU_edge_index": b.BU_edge_index.cpu(),
             "batch": b.batch.cpu(), "rootindex": b.rootindex.cpu(), "y": b.y.cpu()}
    pd = {k: v.double() for k, v in p.items()}
    loss, logp, _ = O.reference_grads(pd, batch, False, None, None, degree_on)
    return loss, logp


@pytest.mark.parametrize("workload", ["twitter15", "weibo_bf16"])
def test_eval_step_full_size_vs_oracle(workload):
    """A full-size evaluation batch (BASELINE workloads: 128 trees, 5000-dim features; the
    Weibo shape with bf16 x and the 2-class head) vs the fp64 oracle in eval mode, with the
    next batch prefetched on the side lane; a second evaluation of the same batch is
    bitwise identical."""
    import bench
    from bigcn_amd import FusedTrainStep
    wl = bench.WORKLOADS[workload]
    pool = bench.make_pool(wl, 0, 2, DEV, (0.0, 0.0))
    classes = wl["classes"]
    p = O.make_params(wl["feats"], 64, 64, classes, seed=31)
    m = _model(p, wl["feats"], classes)
    m.eval()
    st = FusedTrainStep(m)
    loss, correct, pred = st.evaluate(pool[0], next_data=pool[1], pred=True)
    loss1, correct1, pred1 = st.evaluate(pool[1], pred=True)
    loss0, correct0 = st.evaluate(pool[0])
    torch.cuda.synchronize()
    st.check_status()
    assert st.run_report()["status"] == 0
    for b, (ls, cr, pr) in zip(pool, [(loss, correct, pred), (loss1, correct1, pred1)]):
        rloss, rlogp = _oracle_eval(b, p)
        close(ls, rloss, what=f"{workload} loss")
        _check_argmax(pr, cr, rlogp, b.y)
    assert torch.equal(loss, loss0) and torch.equal(correct, correct0)


def _small(seed):
    """Trees of 1, 2 and 40 nodes, F = 64, 4 classes, one row of 33 non-zeros (one entry in
    the spill pool)."""
    from bigcn_amd.data import synth_batch
    b = synth_batch(np.random.default_rng(seed), [1, 2, 40], 64, 4, 0.0, 0.0, device=DEV)
    b.x[17].zero_()
    b.x[17, 5:38] = 1.0
    assert int((b.x[17] != 0).sum()) == 33
    return b


def test_eval_step_preparing_its_own_batch_matches_a_batch_prepared_ahead():
    """An evaluation step that prepares its batch inside the call (prepared_ready = 0, no next
    batch: K1 on the side lane beside the pass over X and the CSC of X as separate launches)
    gives the bits of the same batch evaluated from a buffer bgcn_prepare_batch filled ahead
    (the merged launches).  Trees of 1, 2 and 40 nodes, F = 64, one row of 33 non-zeros (one
    entry in the spill pool).  Both preparations build the same lists in the same order, so
    loss, log-probabilities and predictions are compared bit for bit."""
    from bigcn_amd import FusedTrainStep
    from bigcn_amd.ops import prepare_batch
    from bigcn_amd.train import _Prefetch
    b = _small(7)
    m = _model(O.make_params(64, 64, 64, 4, seed=33), 64)
    m.eval()
    st = FusedTrainStep(m)
    logp = torch.empty(3, 4, device=DEV)
    loss, correct, pred = st.evaluate(b, logp=logp, pred=True)
    assert st._args.prepared_ready == 0 and not st._args.next
    ahead = prepare_batch(b, m.degree_on, "auto")
    d, keep = st._desc(b, drop=False)
    # as a previous call's prefetch leaves it
    st._pending = _Prefetch(batch=b, buf=ahead.buf, key=(False, False), keep=keep, desc=d)
    logp1 = torch.empty(3, 4, device=DEV)
    loss1, correct1, pred1 = st.evaluate(b, logp=logp1, pred=True)
    assert st._args.prepared_ready == 1 and st._args.prepared == ahead.buf.data_ptr()
    torch.cuda.synchronize()
    st.check_status()
    assert torch.equal(loss, loss1) and torch.equal(logp, logp1)
    assert torch.equal(pred, pred1) and torch.equal(correct, correct1)
    rloss, rlogp = _oracle_eval(b, O.make_params(64, 64, 64, 4, seed=33))
    close(logp, rlogp, what="logp")
    close(loss, rloss, what="loss")


def test_prefetch_made_for_a_training_step_is_not_consumed_by_an_evaluation():
    """forward_backward(b0, next_data=b1) in training mode prepares b1 with its DropEdge draw;
    evaluate(b1) must not take that preparation (the record's key differs in `training`): it
    prepares b1 itself, undropped, and gives the bits of a fresh object's evaluate(b1).  The
    discarded preparation still consumed one drop seed: batch k prepared by the object uses
    drop_seed + k, whether a step consumes the preparation or not."""
    from bigcn_amd import FusedTrainStep
    b0, b1 = _small(7), _small(8)
    p = O.make_params(64, 64, 64, 4, seed=33)
    out = []
    for prefetch in (True, False):
        m = _model(p, 64)
        m.train()
        st = FusedTrainStep(m, tddroprate=0.2, budroprate=0.2, drop_seed=100)
        if prefetch:
            st.forward_backward(b0, seed=1, next_data=b1)
            assert st.last_drop_seed == 100 and st._pending is not None
        logp = torch.empty(3, 4, device=DEV)
        loss, correct, pred = st.evaluate(b1, logp=logp, pred=True)
        assert st._args.prepared_ready == 0 and st._pending is None
        torch.cuda.synchronize()
        st.check_status()
        out.append((loss.clone(), logp, pred, correct.clone()))
        if prefetch:
            st.forward_backward(b1, seed=2)
            assert st.last_drop_seed == 102      # b0: 100, the discarded preparation of b1: 101
            torch.cuda.synchronize()
            st.check_status()
    for got, want in zip(*out):
        assert torch.equal(got, want)


def test_rejected_step_call_leaves_no_state_behind():
    """A step call the library rejects at its argument checks (the current batch's x is not
    16-byte aligned: check_batch, before any launch) raises BGCNError and leaves neither the
    next batch's prefetch record nor the deferred-dW1 buffers behind; the next step on the
    object gives the bits of that step on a fresh object."""
    from bigcn_amd import FusedTrainStep
    from bigcn_amd._lib import BGCNError
    from bigcn_amd.data import Batch
    b0, b1 = _small(7), _small(8)
    bad = Batch(**b0.__dict__)
    bad.x = torch.empty(b0.x.numel() + 1, device=DEV)[1:].view_as(b0.x).copy_(b0.x)
    assert bad.x.is_contiguous() and bad.x.data_ptr() % 16 == 4
    p = O.make_params(64, 64, 64, 4, seed=33)
    out = []
    for reject in (True, False):
        m = _model(p, 64)
        m.train()
        st = FusedTrainStep(m)
        if reject:
            with pytest.raises(BGCNError, match="16-byte aligned"):
                st.forward_backward(bad, seed=3, next_data=b1, defer_dw1=True)
            assert st._pending is None and st._dw1_pending is None
        loss = st.forward_backward(b0, seed=5)
        torch.cuda.synchronize()
        st.check_status()
        out.append([loss.clone()] + [g.clone() for g in st.grads().values()])
    assert len(out[0]) == 11
    for got, want in zip(*out):
        assert torch.equal(got, want)


def test_eval_step_matches_per_op_model_and_training_loss():
    """The evaluation step's log-probabilities equal the drop-in modules' model(data) in
    eval mode (the same kernels, 1e-5), and with dropout off its loss equals the training
    step's forward loss on the same batch bit for bit (the same head and loss order)."""
    import torch.nn.functional as F
    from bigcn_amd import FusedTrainStep
    from bigcn_amd.data import synth_batch, synth_tree_sizes
    rng = np.random.default_rng(41)
    b = synth_batch(rng, synth_tree_sizes(rng, 32, 120), 5000, 4, 0.0, 0.0, device=DEV)
    p = O.make_params(5000, 64, 64, 4, seed=32)
    m = _model(p, 5000)
    m.eval()
    st = FusedTrainStep(m)
    logp = torch.empty(32, 4, device=DEV)
    loss, _ = st.evaluate(b, logp=logp)
    with torch.no_grad():
        ref = m(b)
    close(logp, ref, 1e-5, "logp vs model(data)")
    close(loss, F.nll_loss(ref, b.y), 1e-5, "loss vs F.nll_loss(model(data))")
    tl = st.forward_backward(b)        # eval mode: the training step without dropout
    torch.cuda.synchronize()
    assert torch.equal(tl, loss)
