"""conv2's forward on the sparse path (k_conv2_item): a block per (work item, direction),
one 32-node tile per wave, the B operand - the split W2 image and the root's slots - filled
once per block.

What can go wrong there is at the edges of its decomposition: a wave whose tile lies past
the item's end (trees of 1 ... 256 nodes), a half-empty last tile, several items per tree,
and the root row's slots (none, one, a full ELL list, one and two spill rounds, a spilling
root that is its tree's only node).  Each case is one small batch (features 64 or 200 wide,
hidden width 64) and is checked three ways:

* one fused training step, dropout on, fixed seed, against ``oracle.bigcn_oracle`` (fp64):
  loss, all ten gradients and the saved H1 / H2, ``|a-b| <= 1e-4 max|b|`` per tensor (the
  bar of ``test_gpu_train.py``); the oracle takes the device's relu' decisions
  (``relu_masks``, as ``test_gpu_spill.py``), so a tie at zero is not an error;
* the same step run twice is bit-equal;
* the sparse path equals the dense feature path (``feat_mode="dense"``, which never reads
  the root slots or the stored root keep masks) at the same 1e-4 (``test_gpu_fullsize.TOL``).

The oracle and both device runs of a case are computed once and shared by its three tests.
"""
import numpy as np
import pytest
import torch

from oracle import bigcn_oracle as O
from test_gpu_bigcn import DEV, _oracle, close
from test_gpu_fullsize import TOL
from test_gpu_train import KEYS, _model

pytestmark = pytest.mark.gpu

# name -> (tree sizes, features, {tree: non-zeros of its root row}, degree_on)
CASES = {
    # one item per tree: idle waves (1 ... 7 of the block's 8) and a half-empty last tile
    "tile_edges": ([1, 2, 31, 32, 33, 127, 128, 129, 255, 256], 200, {}, "col"),
    # several items per tree (2 and 3), the last one short
    "multi_item": ([257, 600], 200, {}, "col"),
    # a one-node item between two full ones
    "mixed": ([256, 1, 256], 200, {}, "col"),
    # the root's slots: none, one, the ELL list one short and full, one and two spill rounds,
    # and a spilling root that is the whole tree
    "roots": ([5, 40, 130, 256, 33, 70, 1], 200, {0: 0, 1: 1, 2: 31, 3: 32, 4: 33, 5: 65, 6: 33}, "col"),
    # the other degree convention, both directions, with spilling roots and several items
    "degree_row": ([1, 33, 129, 257], 200, {0: 33, 1: 5, 2: 65, 3: 12}, "row"),
    # the narrowest feature width (every root column inside the first 64)
    "feats64": ([1, 32, 129, 300], 64, {0: 0, 1: 32, 2: 33, 3: 64}, "col"),
}
SEED = 20240


def _batch(name):
    from bigcn_amd.data import synth_batch
    sizes, F, roots, _ = CASES[name]
    rng = np.random.default_rng(sum(sizes) + F)
    b = synth_batch(rng, sizes, F, 4, 0.2, 0.2, device=DEV, root_random=True)
    g = torch.Generator().manual_seed(7)
    for tree, n in roots.items():
        row = torch.zeros(F, dtype=b.x.dtype)
        cols = torch.randperm(F, generator=g)[:n]
        row[cols] = torch.randint(1, 4, (n,), generator=g).to(b.x.dtype)
        b.x[int(b.rootindex[tree])] = row.to(DEV)
    nnz = (b.x != 0).sum(1)
    for tree, n in roots.items():
        assert int(nnz[b.rootindex[tree]]) == n
    b.set_x_nnz_max(int(nnz.max()), int((nnz - 32).clamp_min(0).sum()))
    return b


def _run(b, p, mode, degree_on):
    """One fused step (dropout on): loss, the ten gradients, H1, H2 - all cloned."""
    from bigcn_amd import FusedTrainStep
    m = _model(p, mode)
    m.degree_on = degree_on
    m.train()
    step = FusedTrainStep(m)
    loss = step.forward_backward(b, seed=SEED).clone()
    grads = [step.grads()[prm].clone() for prm in step.step_params]
    h1, h2 = (t.clone() for t in step.saved_activations())
    torch.cuda.synchronize()
    step.check_status()
    return step, (loss, grads, h1, h2)


_DONE = {}


def _case(name):
    if name not in _DONE:
        from bigcn_amd.ops import keep_words, unpack_keep
        sizes, F, _, degree_on = CASES[name]
        b = _batch(name)
        p = O.make_params(F, 64, 64, 4, seed=17)
        step, first = _run(b, p, "sparse", degree_on)
        loss2 = step.forward_backward(b, seed=SEED).clone()       # the same step once more
        second = (loss2, [step.grads()[prm].clone() for prm in step.step_params],
                  *(t.clone() for t in step.saved_activations()))
        torch.cuda.synchronize()
        step.check_status()
        _, dense = _run(b, p, "dense", degree_on)
        N = b.x.size(0)
        assert N == sum(sizes)
        mk = unpack_keep(keep_words(SEED, N, F, DEV), 64 + F).cpu()
        h1, h2 = first[2].cpu(), first[3].cpu()
        masks = {d: (h1[:, 64 * k:64 * (k + 1)] > 0, h2[:, 64 * k:64 * (k + 1)] > 0)
                 for k, d in enumerate(("TDrumorGCN", "BUrumorGCN"))}
        _, rloss, rgrads, st = _oracle(b, p, True, mk[0], mk[1], degree_on=degree_on, relu_masks=masks)
        _DONE[name] = (first, second, dense, (rloss, rgrads, st))
    return _DONE[name]


@pytest.mark.parametrize("name", CASES)
def test_step_matches_oracle(name):
    (loss, grads, h1, h2), _, _, (rloss, rgrads, st) = _case(name)
    close(loss, rloss, what="loss")
    for k, g in zip(KEYS, grads):
        close(g, rgrads[k], what=k)
    for k, d in enumerate(("TDrumorGCN", "BUrumorGCN")):
        close(h1[:, 64 * k:64 * (k + 1)], st[f"{d}.h1"], what=f"{d}.h1")
        close(h2[:, 64 * k:64 * (k + 1)], st[f"{d}.h2"], what=f"{d}.h2")


@pytest.mark.parametrize("name", CASES)
def test_step_is_deterministic(name):
    first, second, _, _ = _case(name)
    assert torch.equal(first[0], second[0]), "loss"
    for k, a, c in zip(KEYS, first[1], second[1]):
        assert torch.equal(a, c), k
    assert torch.equal(first[2], second[2]), "H1"
    assert torch.equal(first[3], second[3]), "H2"


@pytest.mark.parametrize("name", CASES)
def test_sparse_equals_dense_feature_path(name):
    sparse, _, dense, _ = _case(name)
    close(sparse[0], dense[0], tol=TOL, what="loss")
    for k, a, c in zip(KEYS, sparse[1], dense[1]):
        close(a, c, tol=TOL, what=k)
    close(sparse[2], dense[2], tol=TOL, what="H1")
    close(sparse[3], dense[3], tol=TOL, what="H2")
