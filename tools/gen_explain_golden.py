"""Write tests/golden/explain_*.npz: the stage rankings the REFERENCE's own analysis code produces
(explain_PHEME.py of the cwkd/BiGCN checkout given with --reference: extract_intermediates_bigcn,
extract_intermediates_ebgcn), on CPU in fp32.

Runs on a CPU machine that has the reference checkout; the test suite only reads the files.
Nothing of the reference is copied: its module is loaded from its path (the `__main__` guard keeps
its script body from running) and its two functions are called.  Third-party imports that are not
installed are stubbed: torch_geometric / torch_scatter with the oracle's restatements, exactly as
tools/gen_ebgcn_golden.py does, plus empty modules for what the analysis functions never touch
(lrp_pytorch.modules.utils, torch_geometric.nn.conv.gcn_conv, transformers if absent).

Each file holds arrays only: the batch (x, edge_index, BU_edge_index, batch, rootindex), the
settings (ebgcn, edge_num, num_class, edge_infer_td, edge_infer_bu), the state_dict by key
("sd/<key>"), and per direction d in (td, bu) and stage the reference's whole-batch topk
("<d>/<stage>_topk/indices", ".../values") and "<d>/gcn_output"; x_sum's topk and the log-probs
of the reference model's normal forward.

The reference's topk ranks the whole batch; only for a single-tree batch is that a per-tree
ranking.  For the multi-tree cases the tests derive each tree's expectation from the values.
torch.topk leaves the order of equal values unspecified, so every case must keep adjacent sorted
values of a tree at least GAP_FLOOR apart in every stage (x_sum excepted: bag-of-words rows tie
by construction); the generator asserts it, prints the smallest gap, and `--search K` tries the
next K model seeds of a case that fails.

    python tools/gen_explain_golden.py --reference /path/to/BiGCN
"""
import argparse
import importlib.machinery
import importlib.util
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_ebgcn_golden as G   # noqa: E402  (the batches, the stubs and the parameter randomisation)

ROOT = G.ROOT
F_IN = G.F_IN
GAP_FLOOR = 1e-3


def _empty_module(name, **attrs):
    m = types.ModuleType(name)
    m.__spec__ = importlib.machinery.ModuleSpec(name, None)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def _load_reference(ref_root):
    sys.path.insert(0, ref_root)    # the reference's `tools` / `Process` / `model` packages
    sys.path.append(ROOT)           # for `oracle` only
    G._stub_third_party()
    conv = _empty_module("torch_geometric.nn.conv", gcn_conv=types.ModuleType("gcn_conv"))
    sys.modules["torch_geometric.nn"].conv = conv
    _empty_module("lrp_pytorch")
    _empty_module("lrp_pytorch.modules")
    _empty_module("lrp_pytorch.modules.utils")
    if importlib.util.find_spec("transformers") is None:
        _empty_module("transformers", BertModel=object, BertTokenizer=object)
    cwd = os.getcwd()
    os.chdir(ref_root)
    try:
        spec = importlib.util.spec_from_file_location("ref_explain", os.path.join(ref_root, "explain_PHEME.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        os.chdir(cwd)
    return mod


CASES = {
    # name: (ebgcn, trees, roots moved off node 0, model seed, batch seed, edge_num)
    "bigcn_mixed": (False, [("chain", 6), ("star", 9), ("random", 24), ("chain", 2), ("random", 12)], (2, 4), 1, 21, 0),
    "bigcn_single": (False, [("random", 17)], (0,), 2, 22, 0),
    "ebgcn_mixed": (True, [("random", 11), ("star", 8), ("chain", 5), ("random", 24), ("chain", 2)], (0, 3), 1003, 23, 2),
    "ebgcn_single": (True, [("random", 19)], (), 4, 24, 3),
}


def _tree_gaps(values, batch):
    """Smallest gap between adjacent sorted values inside a tree."""
    gap = np.inf
    for t in np.unique(batch):
        v = np.sort(values[batch == t])
        if v.size > 1:
            gap = min(gap, float(np.diff(v).min()))
    return gap


def _build(ref, ebgcn, spec, mid, mseed, bseed, knum):
    dev = torch.device("cpu")
    torch.manual_seed(mseed)
    if ebgcn:
        args = argparse.Namespace(input_features=F_IN, hidden_features=64, output_features=64, num_class=4,
                                  edge_num=knum, edge_infer_td=True, edge_infer_bu=True, dropout=0.5, device=dev)
        model = ref.EBGCN(args).float().eval()
    else:
        model = ref.BiGCN(F_IN, 64, 64, dev).float().eval()
    G.randomise(model, mseed)
    b = G.make_batch(spec, np.random.default_rng(bseed), mid)
    data = argparse.Namespace(**{k: torch.from_numpy(v) for k, v in b.items()})
    out = dict(b)
    gap = np.inf
    with torch.no_grad():
        x_sum = torch.sum(data.x, dim=-1)
        top = torch.topk(x_sum, k=x_sum.shape[0])
        out["x_sum_indices"], out["x_sum_values"] = top.indices.numpy(), top.values.numpy()
        for d, sub, ei in (("td", model.TDrumorGCN, data.edge_index), ("bu", model.BUrumorGCN, data.BU_edge_index)):
            if ebgcn:
                rec = ref.extract_intermediates_ebgcn(sub, data.x, ei, data, dev)
            else:
                rec = ref.extract_intermediates_bigcn(sub.conv1, sub.conv2, data.x, ei, data, dev)
            for key, val in rec.items():
                if key == "gcn_output":
                    out[f"{d}/gcn_output"] = np.asarray(val, dtype=np.float32)
                    continue
                idx, vals = np.asarray(val[0], dtype=np.int64), np.asarray(val[1], dtype=np.float32)
                out[f"{d}/{key}/indices"], out[f"{d}/{key}/values"] = idx, vals
                node_vals = np.empty_like(vals)
                node_vals[idx] = vals
                gap = min(gap, _tree_gaps(node_vals, b["batch"]))
        res = model(data)
        out["logp"] = (res[0] if isinstance(res, tuple) else res).numpy()
    out.update(ebgcn=np.int64(ebgcn), edge_num=np.int64(knum), num_class=np.int64(4), edge_infer_td=np.int64(1),
               edge_infer_bu=np.int64(1))
    out.update({"sd/" + k: v.numpy() for k, v in model.state_dict().items()})
    return out, gap


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the cwkd/BiGCN checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--search", type=int, default=0, help="on a gap below the floor, try this many further model seeds")
    a = ap.parse_args()
    ref = _load_reference(os.path.abspath(a.reference))
    for name, (ebgcn, spec, mid, mseed, bseed, knum) in CASES.items():
        assert max(n for _, n in spec) <= 24
        for seed in range(mseed, mseed + 1000 * (a.search + 1), 1000):
            out, gap = _build(ref, ebgcn, spec, mid, seed, bseed, knum)
            print(f"{name}: model seed {seed} N={out['x'].shape[0]} smallest gap inside a tree {gap:.3e}")
            if gap >= GAP_FLOOR:
                break
        assert gap >= GAP_FLOOR, "choose another seed: two nodes of a tree are nearly tied in some stage"
        assert seed == mseed, f"put model seed {seed} into CASES['{name}']"
        assert np.isfinite(out["logp"]).all()
        np.savez_compressed(os.path.join(a.out, f"explain_{name}.npz"), **out)


if __name__ == "__main__":
    main()
