"""Write tests/golden/ebgcn_*.npz: EBGCN eval-mode fixtures produced by the REFERENCE's own
classes (model/Twitter/EBGCN.py of the cwkd/BiGCN checkout given with --reference).

Runs on a CPU machine that has the reference checkout; the test suite only reads the files.
Nothing of the reference is copied: its module is loaded from its path and run.  Its two
third-party imports that are not installed are stubbed with the oracle's restatements
(oracle/bigcn_oracle.py: gcn_conv, scatter_mean) - everything EBGCN adds over BiGCN (edge_infer,
bn1, the five per-edge networks) is plain torch and runs as the reference wrote it, in eval()
and fp32.

Each file holds: the batch (x, edge_index, BU_edge_index, batch, rootindex), the settings
(edge_num, num_class, edge_infer_td, edge_infer_bu), the full state_dict by key ("sd/<key>"),
the per-direction edge_pred the reference computed (td_edge_pred, bu_edge_pred; empty when that
direction's inference is off) and the log-probs.

Parameters are NOT the default init (with it every edge_pred is ~0.506 and a broken kernel
would pass): BatchNorm statistics and affine terms, the conv weights' and fc1's scale and bn1 are
randomised.  The seeds below were chosen so that the reference's edge_pred spans [0.2, 0.8] in
every fixture with edges and every log-prob row's top two classes are more than 1e-3 apart
(tests/test_ebgcn.py asserts both).

    python tools/gen_ebgcn_golden.py --reference /path/to/BiGCN
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F_IN = 64


def _stub_third_party():
    from oracle import bigcn_oracle as O

    class _Lin(torch.nn.Module):
        def __init__(self, i, o):
            super().__init__()
            a = (6.0 / (i + o)) ** 0.5
            self.weight = torch.nn.Parameter(torch.empty(o, i).uniform_(-a, a))

    class GCNConv(torch.nn.Module):
        def __init__(self, i, o):
            super().__init__()
            self.lin = _Lin(i, o)
            self.bias = torch.nn.Parameter(torch.zeros(o))

        def forward(self, x, edge_index, edge_weight=None):
            return O.gcn_conv(x, edge_index, self.lin.weight, self.bias, edge_weight)

    def scatter_mean(src, index, dim=0, **kw):
        return O.scatter_mean(src, index, dim)

    tg = types.ModuleType("torch_geometric")
    tg.nn = types.ModuleType("torch_geometric.nn")
    tg.nn.GCNConv = GCNConv
    tg.data = types.ModuleType("torch_geometric.data")
    tg.data.DataLoader = tg.data.Data = tg.data.Batch = object
    ts = types.ModuleType("torch_scatter")
    ts.scatter_mean = scatter_mean
    sys.modules.update({"torch_geometric": tg, "torch_geometric.nn": tg.nn, "torch_geometric.data": tg.data,
                        "torch_scatter": ts})


def _load_reference(ref_root):
    # the reference's `tools` / `Process` packages must win over this repository's
    sys.path.insert(0, ref_root)
    sys.path.append(ROOT)           # for `oracle` only
    _stub_third_party()
    cwd = os.getcwd()
    os.chdir(ref_root)
    try:
        spec = importlib.util.spec_from_file_location("ref_ebgcn", os.path.join(ref_root, "model", "Twitter", "EBGCN.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        os.chdir(cwd)
    return mod


# ---- batches: (parent, child) edges in global ids, trees collated PyG style
def _tree(kind, n, rng):
    if kind == "chain":
        return [(i, i + 1) for i in range(n - 1)]
    if kind == "star":
        return [(0, i) for i in range(1, n)]
    return [(int(rng.integers(0, i)), i) for i in range(1, n)]   # random recursive tree


def make_batch(spec, rng, root_mid=()):
    xs, td, batch, roots, off = [], [], [], [], 0
    for t, (kind, n) in enumerate(spec):
        e = np.asarray(_tree(kind, n, rng), dtype=np.int64).reshape(-1, 2)
        root = 0
        if t in root_mid and n > 2:     # a root that is not its tree's first node: relabel 0 <-> n // 2
            root = n // 2
            sw = e.copy()
            sw[e == 0], sw[e == root] = root, 0
            e = sw
        td.append(e + off)
        # bag-of-words-like rows: a few small counts
        x = np.zeros((n, F_IN), dtype=np.float32)
        for i in range(n):
            cols = rng.choice(F_IN, size=int(rng.integers(3, 9)), replace=False)
            x[i, cols] = rng.integers(1, 4, size=cols.size)
        xs.append(x)
        batch += [t] * n
        roots.append(off + root)
        off += n
    td = np.concatenate(td, 0).T.reshape(2, -1)
    return {"x": np.concatenate(xs, 0), "edge_index": td, "BU_edge_index": td[::-1].copy(),
            "batch": np.asarray(batch, dtype=np.int64), "rootindex": np.asarray(roots, dtype=np.int64)}


def randomise(model, seed):
    g = torch.Generator().manual_seed(seed)

    def rnd(*shape):
        return torch.randn(*shape, generator=g)

    def uni(lo, hi, *shape):
        return torch.rand(*shape, generator=g) * (hi - lo) + lo

    with torch.no_grad():
        for name, m in model.named_modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                c = m.num_features
                m.running_mean.copy_(rnd(c) * 0.3)
                m.running_var.copy_(uni(0.5, 2.0, c))
                m.weight.copy_(uni(0.5, 1.5, c))
                m.bias.copy_(rnd(c) * 0.3)
                m.num_batches_tracked.fill_(seed + 17)
            elif isinstance(m, torch.nn.Conv1d):
                m.weight.mul_(3.0)
                if m.bias is not None:
                    m.bias.copy_(rnd(*m.bias.shape) * 0.2)
            elif name.endswith("fc1") or name.endswith("fc2"):
                m.weight.mul_(6.0)
            elif name.endswith("conv1") or name.endswith("conv2"):
                m.bias.copy_(rnd(*m.bias.shape) * 0.1)


CASES = {
    # name: (trees, roots moved off node 0, model seed, batch seed, edge_infer_td, edge_infer_bu, edge_num)
    "mixed": ([("chain", 6), ("star", 9), ("random", 17), ("chain", 2), ("random", 12)], (2, 4), 17, 11, True, True, 2),
    "star40": ([("star", 41)], (), 10, 12, True, True, 3),
    "single": ([("chain", 1)], (), 3, 13, True, True, 2),
    "nobu": ([("chain", 6), ("star", 9), ("random", 17), ("chain", 2), ("random", 12)], (2, 4), 8, 14, True, False, 1),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the cwkd/BiGCN checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    ref = _load_reference(os.path.abspath(a.reference))
    for name, (spec, mid, mseed, bseed, itd, ibu, knum) in CASES.items():
        args = argparse.Namespace(input_features=F_IN, hidden_features=64, output_features=64, num_class=4,
                                  edge_num=knum, edge_infer_td=itd, edge_infer_bu=ibu, dropout=0.5,
                                  device=torch.device("cpu"))
        torch.manual_seed(mseed)
        model = ref.EBGCN(args).float().eval()
        randomise(model, mseed)
        b = make_batch(spec, np.random.default_rng(bseed), mid)
        data = argparse.Namespace(**{k: torch.from_numpy(v) for k, v in b.items()})
        preds = {}
        for d, flag in (("TDrumorGCN", itd), ("BUrumorGCN", ibu)):
            sub = getattr(model, d)
            orig = sub.edge_infer

            def spy(x, ei, _orig=orig, _d=d):
                loss, pred = _orig(x, ei)
                preds[_d] = pred.detach().clone()
                return loss, pred
            sub.edge_infer = spy
        with torch.no_grad():
            logp, _, _ = model(data)
        empty = torch.zeros(0)
        out = dict(b)
        out.update(edge_num=np.int64(knum), num_class=np.int64(4), edge_infer_td=np.int64(itd),
                   edge_infer_bu=np.int64(ibu), logp=logp.numpy(),
                   td_edge_pred=preds.get("TDrumorGCN", empty).numpy().astype(np.float32),
                   bu_edge_pred=preds.get("BUrumorGCN", empty).numpy().astype(np.float32))
        sd = model.state_dict()
        assert len(sd) == 104, len(sd)
        out.update({"sd/" + k: v.numpy() for k, v in sd.items()})
        allp = np.concatenate([out["td_edge_pred"], out["bu_edge_pred"]])
        top = np.sort(logp.numpy(), 1)
        gap = float((top[:, -1] - top[:, -2]).min())
        span = (float(allp.min()), float(allp.max())) if allp.size else None
        print(f"{name}: N={b['x'].shape[0]} E={b['edge_index'].shape[1]} edge_pred span {span} top-two gap {gap:.4f}")
        assert gap > 1e-3, "choose another seed: a log-prob row is nearly tied"
        assert span is None or (span[0] <= 0.2 and span[1] >= 0.8), "choose another seed: edge_pred too flat"
        assert np.isfinite(logp.numpy()).all()
        np.savez_compressed(os.path.join(a.out, f"ebgcn_{name}.npz"), **out)


if __name__ == "__main__":
    main()
