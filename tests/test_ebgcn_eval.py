"""CPU checks of the EBGCN evaluation step's boundary: the header, the exports, the ctypes
mirrors' layout, the workspace query and the argument checks (which run before any HIP call, so
fake 16-byte-aligned addresses are never dereferenced), and the Python surface."""
import argparse
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bgcn.h")
NAMES = ("bgcn_ebgcn_eval_workspace_size", "bgcn_ebgcn_eval_step", "bgcn_ebgcn_eval_saved")


def test_header_declares_and_library_exports():
    from bigcn_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = _lib.load_library()
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", src), name
        assert name in _lib.EXPORTED_SYMBOLS and name in _lib._SIGS
        assert hasattr(lib, name), name
    assert lib.bgcn_abi_version() == 12
    assert re.search(r"#define BGCN_ABI_VERSION 12\b", src)
    m = re.search(r"#define BGCN_STATUS_BATCH_UNSORTED (\d+)", src)
    assert m and int(m.group(1)) == _lib.BGCN_STATUS_BATCH_UNSORTED


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_ctypes_structs_match_the_header(tmp_path):
    from bigcn_amd import _lib
    structs = {"bgcn_ebgcn_dir": _lib.EbgcnDir, "bgcn_ebgcn_eval_args": _lib.EbgcnEvalArgs,
               "bgcn_ebgcn_eval_view": _lib.EbgcnEvalView}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {"]
    for cname, py in structs.items():
        lines.append(f'printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for fname, _ in py._fields_:
            lines.append(f'printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0; }")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(c)], check=True)
    got = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n"):
        if line:
            s, f, v = line.split()
            got[(s, f)] = int(v)
    for cname, py in structs.items():
        assert got[(cname, "sizeof")] == ctypes.sizeof(py), cname
        for fname, _ in py._fields_:
            assert got[(cname, fname)] == getattr(py, fname).offset, (cname, fname)


def test_workspace_size_grows_with_nodes_and_edges():
    from bigcn_amd import _lib
    size = _lib.load_library().bgcn_ebgcn_eval_workspace_size
    base = size(100, 4, 36, 96, 96, 2)
    assert base > 0
    assert size(1000, 4, 36, 96, 96, 2) > base
    assert size(100, 4, 36, 5000, 96, 2) > base and size(100, 4, 36, 96, 5000, 2) > base
    assert size(0, 4, 36, 96, 96, 2) == 0 and size(100, 4, 36, -1, 96, 2) == 0 and size(100, 4, 36, 96, 96, 9) == 0


def test_argument_checks_report_the_first_failure():
    from bigcn_amd import _lib
    lib = _lib.load_library()
    fake = 0x10000
    N, B, F, C, E, K = 43, 3, 64, 4, 40, 2

    def plausible():
        a = _lib.EbgcnEvalArgs()
        b = a.batch
        b.x, b.ldx, b.num_nodes, b.num_graphs = fake, F, N, B
        b.batch, b.rootindex = fake + 0x100, fake + 0x200
        b.td_edge_index, b.td_num_edges, b.bu_edge_index, b.bu_num_edges = fake + 0x300, E, fake + 0x400, E
        b.x_dtype = _lib.BGCN_DTYPE_F32
        for k, d in enumerate((a.td, a.bu)):
            for j, (name, _) in enumerate(_lib.EbgcnDir._fields_[:16]):
                setattr(d, name, fake + 0x10000 * (k + 1) + 0x100 * j)
            d.bn1_eps = d.sim_norm_eps = 1e-5
            d.infer = 1
        a.fc_w, a.fc_b = fake + 0x500, fake + 0x600
        a.in_feats, a.num_classes, a.edge_num, a.degree_on = F, C, K, 0
        a.y, a.loss, a.correct, a.status = fake + 0x700, fake + 0x800, fake + 0x900, fake + 0xa00
        return a

    def call(a, ws=None, ws_bytes=0):
        return lib.bgcn_ebgcn_eval_step(ctypes.addressof(a), ws, ws_bytes, None)

    def rejected(rc, text):
        assert rc == -1
        assert text in lib.bgcn_last_error(), lib.bgcn_last_error()

    rejected(call(_lib.EbgcnEvalArgs()), b"bad sizes")
    a = plausible()
    a.batch.td_num_edges = -1
    rejected(call(a), b"bad sizes")
    for c in (0, 17):
        a = plausible()
        a.num_classes = c
        rejected(call(a), b"num_classes must be in [1, 16]")
    for k in (0, 9):
        a = plausible()
        a.edge_num = k
        rejected(call(a), b"edge_num must be in [1, 8]")
    a = plausible()
    a.batch.bu_droprate = 0.25
    rejected(call(a), b"drops no edges")
    for name in ("conv1_w", "bn1_var", "sim_out_b", "fc1_w"):
        a = plausible()
        setattr(a.bu, name, None)
        rejected(call(a), b"null parameter pointer")
    a = plausible()
    a.fc_b = None
    rejected(call(a), b"null parameter pointer")
    # the workspace is checked last: a complete call without one, and with one a byte short
    rejected(call(plausible()), b"workspace too small")
    need = lib.bgcn_ebgcn_eval_workspace_size(N, B, F, E, E, K)
    rejected(call(plausible(), fake + 0x100000, need - 1), b"workspace too small")


def _args(F=36):
    return argparse.Namespace(input_features=F, hidden_features=64, output_features=64, num_class=4, edge_num=2,
                              edge_infer_td=True, edge_infer_bu=True, device="cpu")


def test_python_surface_and_training_mode_still_refused():
    from bigcn_amd import EBGCN
    from bigcn_amd.data import Batch
    model = EBGCN(_args())
    for name in ("evaluate", "validate", "check_status"):
        assert callable(getattr(model, name))
    model.check_status()     # nothing evaluated: nothing to report
    data = Batch(x=torch.zeros(3, 36), edge_index=torch.tensor([[0, 0], [1, 2]]),
                 BU_edge_index=torch.tensor([[1, 2], [0, 0]]), batch=torch.zeros(3, dtype=torch.int64),
                 rootindex=torch.zeros(1, dtype=torch.int64), y=torch.zeros(1, dtype=torch.int64), num_graphs=1)
    with pytest.raises(NotImplementedError, match="inference-only"):
        model.train()(data)
    with pytest.raises(ValueError, match="at least one batch"):
        model.validate([])
