"""Helpers shared by the GPU tests of the LSTM baseline (test_gpu_lstm.py, test_gpu_lstm_edges.py,
test_gpu_lstm_train.py).  A case ``c`` is one of lstm_ref.case / edge_case or lstm_train_ref.case."""
import functools
from types import SimpleNamespace

import torch

DEV = "cuda:0"


def _new_model(c, sd=None, train=False, version=2, pooling='max'):
    from bigcn_amd import LSTM
    m = LSTM(c.cfg["in_feats"], c.cfg["hid"], c.cfg["out"], c.cfg["layers"], version=version, pooling=pooling)
    m.load_state_dict({k: v.float() for k, v in (sd or c.sd).items()}, strict=True)
    m = m.to(DEV)
    return m.train() if train else m.eval()


def _x(c):
    """The case's rows on the device; with pad_cols a column slice of a wider tensor (ldx > in_feats)."""
    pad = c.cfg.get("pad_cols", 0)
    if not pad:
        return c.x.float().contiguous().to(DEV)
    wide = torch.full((c.N, c.cfg["in_feats"] + pad), 7.0, device=DEV)
    wide[:, :c.cfg["in_feats"]] = c.x.float().to(DEV)
    return wide[:, :c.cfg["in_feats"]]


def _data(c, rootindex=None, y=None):
    return SimpleNamespace(cls=_x(c), rootindex=(c.rootindex if rootindex is None else rootindex).to(DEV),
                           y=(c.y if y is None else y).to(DEV))


def _ends(c, rootindex=None):
    roots = (c.rootindex if rootindex is None else rootindex).tolist()
    return list(zip(roots, roots[1:] + [c.N]))


@functools.lru_cache(maxsize=None)
def _weights(name, case):
    """The weights of ``case(name)`` on the device, as the C ABI reads them."""
    return {k: v.float().contiguous().to(DEV) for k, v in case(name).sd.items()}


def _buf(nbytes, fill):
    """A device buffer of at least ``nbytes`` holding zero bytes, 0xFF bytes (NaN as fp32) or the fp32 3.0e38."""
    b = torch.empty((max(int(nbytes), 16) + 15) // 16 * 16, dtype=torch.uint8, device=DEV)
    if fill == "zero":
        b.zero_()
    elif fill == "ff":
        b.fill_(0xFF)
    else:
        assert fill == "big"
        b.view(torch.float32).fill_(3.0e38)
    return b


def _fwd_args(a, c, w, x, root, max_len=None):
    """The inputs of an ``LstmArgs``: the shape, x, the sequences and the weights ``w`` (:func:`_weights`).
    The labels and every output stay with the caller."""
    L = c.cfg["layers"]
    a.x, a.ldx, a.num_nodes, a.in_feats, a.hid, a.num_layers, a.out_feats = x.data_ptr(), x.stride(0), c.N, \
        c.cfg["in_feats"], c.cfg["hid"], L, c.cfg["out"]
    a.seq_start, a.num_seqs, a.max_len = root.data_ptr(), c.B, c.max_len if max_len is None else max_len
    for l in range(L):
        for d in range(2):
            rev = "_reverse" if d else ""
            a.w_ih[l][d] = w[f"lstm.weight_ih_l{l}{rev}"].data_ptr()
            a.w_hh[l][d] = w[f"lstm.weight_hh_l{l}{rev}"].data_ptr()
    a.fc_w, a.fc_b = w["fc.weight"].data_ptr(), w["fc.bias"].data_ptr()
