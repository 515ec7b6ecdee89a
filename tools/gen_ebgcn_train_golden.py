"""Write tests/golden/train_ebgcn_*.npz: EBGCN TRAINING-mode fixtures produced by the REFERENCE's
own classes (model/Twitter/EBGCN.py of the cwkd/BiGCN checkout given with --reference).

Runs on a CPU machine that has the reference checkout; the test suite only reads the files.
Nothing of the reference is copied: its module is loaded from its path (with the stubs of
tools/gen_ebgcn_golden.py for its two third-party imports) and run in train() mode, fp32.  For the
duration of a run ``torch.normal(mean, std)`` is replaced by ``mean + std * noise`` for a recorded
standard-normal ``noise``, so the Bayesian draw is part of the fixture.

(The files are named train_ebgcn_*, not ebgcn_train_*: tests/test_ebgcn.py globs ebgcn_*.npz for
the eval-mode fixtures.)

Edge fixtures (train_ebgcn_edge_*.npz), one direction's ``edge_infer(h, edge_index)``:
  sd/<key>      the direction's state_dict before the forward, keys prefixed "TDrumorGCN."
  h, edge_index, noise, c [E], g []       inputs and the cotangents
  edge_pred, edge_loss                    what the reference returned
  grad_h, grad/<key>                      gradients of sum(c * edge_pred) + g * edge_loss
  none_grad, zero_grad                    the parameters whose grad is None / all zeros (torch.normal's
                                          derivative is zeros: the four Bayesian networks)
  after/<key>                             the five norm0 modules' buffers after the forward
Model fixture (train_ebgcn_model.npz, F = 64), the reference's ``EBGCN.forward`` in train mode:
  sd/<key>, the batch (x, edge_index, BU_edge_index, batch, rootindex, y), noise_td, noise_bu,
  logp, td_loss, bu_loss, grad/<key> and none_grad of nll_loss + 0.2 (TD + BU), after/<key> (every
  buffer of the model).

Parameters are randomised as in tools/gen_ebgcn_golden.py.  The seeds below were chosen so that
the reference alone meets the conditions asserted at the end of each edge fixture (and re-asserted
by tests/test_ebgcn_train.py), so that a wrong kernel cannot pass.

    python tools/gen_ebgcn_train_golden.py --reference /path/to/BiGCN
"""
import argparse
import os
from unittest import mock

import numpy as np
import torch
import torch.nn.functional as F

from gen_ebgcn_golden import F_IN, ROOT, _load_reference, make_batch, randomise


class Recorder:
    """Stands in for torch.normal while the reference runs: the recorded draws, in call order."""

    def __init__(self, noises):
        self.noises = list(noises)
        self.std = []

    def __call__(self, mean, std):
        self.std.append(std.detach().clone())
        # like torch.normal itself, whose derivative w.r.t. mean and std is zeros
        return mean * 0 + std * 0 + (mean + std * self.noises.pop(0).view_as(mean)).detach()


def _args(knum, itd=True, ibu=True):
    return argparse.Namespace(input_features=F_IN, hidden_features=64, output_features=64, num_class=4,
                              edge_num=knum, edge_infer_td=itd, edge_infer_bu=ibu, dropout=0.5,
                              device=torch.device("cpu"))


def _norm_buffers(module, prefix):
    return {prefix + k: v.clone() for k, v in module.state_dict().items()
            if "norm0" in k and ("running" in k or "num_batches" in k)}


EDGE_CASES = {
    # name: (N, E, edge_num, model seed, data seed)
    "k2": (40, 70, 2, 3, 21),
    "k3": (12, 33, 3, 9, 22),
}


def edge_case(ref, name, N, E, knum, mseed, dseed, out_dir):
    torch.manual_seed(mseed)
    sub = ref.TDrumorGCN(_args(knum)).float().train()
    randomise(sub, mseed)
    g = torch.Generator().manual_seed(dseed)
    h = (torch.randn(N, 64, generator=g) * 0.7).requires_grad_(True)
    ei = torch.randint(0, N, (2, E), generator=g)
    ei[0, 0] = 0                       # an index 0: reads the LAST node
    ei[1, 1] = 0
    ei[1, 2] = ei[0, 2]                # row == col: D has zeros (on its diagonal)
    noise = torch.randn(E, 64, generator=g)
    c, gl = torch.randn(E, generator=g), torch.randn((), generator=g)
    before = {"TDrumorGCN." + k: v.clone() for k, v in sub.state_dict().items()}
    seen = {}
    sub.sim_network.sim_valnorm0.register_forward_hook(lambda m, i, o: seen.__setitem__("pre", o.detach().clone()))
    sub.eval_loss.register_forward_hook(          # its inputs are (log_softmax(p), p_y)
        lambda m, i, o: seen.update(softmax_p=i[0].detach().exp(), p_y=i[1].detach().clone()))
    rec = Recorder([noise])
    with mock.patch.object(torch, "normal", rec):
        loss, pred = sub.edge_infer(h, ei)
    (c * pred).sum().add(gl * loss).backward()
    out = {"h": h.detach(), "edge_index": ei, "noise": noise, "c": c, "g": gl, "edge_num": torch.tensor(knum),
           "edge_pred": pred.detach(), "edge_loss": loss.detach(), "grad_h": h.grad}
    none = []
    for k, p in sub.named_parameters():
        if p.grad is None:
            none.append("TDrumorGCN." + k)
        else:
            out["grad/TDrumorGCN." + k] = p.grad
    out.update({"sd/" + k: v for k, v in before.items()})
    out.update({"after/" + k: v for k, v in _norm_buffers(sub, "TDrumorGCN.").items()})
    # the conditions (tests/test_ebgcn_train.py asserts them again on the stored values)
    std = rec.std[0]
    out["std"] = std.reshape(E, 64)
    out["pre_sign_counts"] = torch.tensor([int((seen["pre"] > 0).sum()), int((seen["pre"] < 0).sum())])
    out["target_gap"] = (seen["p_y"] - seen["softmax_p"]).abs().max()
    zero, pos = float((std == 0).float().mean()), float((std > 0).float().mean())
    print(f"edge_{name}: N={N} E={E} K={knum} pred span ({float(pred.min()):.3f}, {float(pred.max()):.3f}) "
          f"std zero {zero:.2f} positive {pos:.2f} pre signs {out['pre_sign_counts'].tolist()} "
          f"target gap {float(out['target_gap']):.3f} loss {float(loss):.4f}")
    assert float(pred.min()) <= 0.2 and float(pred.max()) >= 0.8, "choose another seed: edge_pred too flat"
    assert zero >= 0.1 and pos >= 0.1, "choose another seed: std needs exact zeros and positive entries"
    assert min(out["pre_sign_counts"].tolist()) > 0, "choose another seed: the pre-activation has one sign"
    assert float(out["target_gap"]) > 0.05, "choose another seed: p_y equals softmax(p)"
    assert bool((ei[0] == ei[1]).any()) and bool((ei == 0).any())
    assert all(torch.isfinite(v.float()).all() for v in out.values() if torch.is_tensor(v))
    # torch.normal's derivative is zeros, not None: the four Bayesian networks end with all-zero grads
    zeros = [k[5:] for k, v in out.items() if k.startswith("grad/") and not bool(v.any())]
    assert len(zeros) == 20 and all(".W_" in k or ".B_" in k for k in zeros)
    out["zero_grad"] = np.asarray(sorted(zeros))
    out["none_grad"] = np.asarray(sorted(none))
    np.savez_compressed(os.path.join(out_dir, f"train_ebgcn_edge_{name}.npz"),
                        **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in out.items()})


def model_case(ref, out_dir, mseed=17, bseed=11, knum=2):
    spec = [("chain", 6), ("star", 9), ("random", 17), ("chain", 2), ("random", 12)]
    torch.manual_seed(mseed)
    model = ref.EBGCN(_args(knum)).float().train()
    randomise(model, mseed)
    b = make_batch(spec, np.random.default_rng(bseed), (2, 4))
    data = argparse.Namespace(**{k: torch.from_numpy(v) for k, v in b.items()})
    E = data.edge_index.size(1)
    g = torch.Generator().manual_seed(bseed)
    noise_td, noise_bu = torch.randn(E, 64, generator=g), torch.randn(E, 64, generator=g)
    y = torch.randint(0, 4, (len(spec),), generator=g)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    rec = Recorder([noise_td, noise_bu])          # TD runs first (EBGCN.py:224-225)
    with mock.patch.object(torch, "normal", rec):
        logp, td_loss, bu_loss = model(data)
    (F.nll_loss(logp, y) + 0.2 * (td_loss + bu_loss)).backward()
    out = dict(b)
    out.update(y=y, noise_td=noise_td, noise_bu=noise_bu, edge_num=torch.tensor(knum), logp=logp.detach(),
               td_loss=td_loss.detach(), bu_loss=bu_loss.detach())
    none = []
    for k, p in model.named_parameters():
        if p.grad is None:
            none.append(k)
        else:
            out["grad/" + k] = p.grad
    out.update({"sd/" + k: v for k, v in before.items()})
    out.update({"after/" + k: v.clone() for k, v in model.state_dict().items()
                if "running" in k or "num_batches" in k})
    print(f"model: N={b['x'].shape[0]} E={E} losses {float(td_loss):.4f} {float(bu_loss):.4f} "
          f"{len(none)} parameters without a gradient")
    zeros = [k[5:] for k, v in out.items() if k.startswith("grad/") and not bool(v.any())]
    assert len(none) == 0 and len(zeros) == 40 and np.isfinite(logp.detach().numpy()).all()
    out["zero_grad"] = np.asarray(sorted(zeros))
    out["none_grad"] = np.asarray(sorted(none))
    np.savez_compressed(os.path.join(out_dir, "train_ebgcn_model.npz"),
                        **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in out.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the cwkd/BiGCN checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    ref = _load_reference(os.path.abspath(a.reference))
    for name, case in EDGE_CASES.items():
        edge_case(ref, name, *case, a.out)
    model_case(ref, a.out)


if __name__ == "__main__":
    main()
