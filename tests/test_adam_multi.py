"""CPU checks of the many-tensor Adam (bgcn_adam_multi_*), the EBGCN training-loss entry point's
refusals, MultiAdam's limits and ebgcn_adam's groups.  Nothing here touches a device: every refusal
is decided on the host before a launch, and the plan fills a host image."""
import argparse
import ctypes
import os
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 4096   # a non-null, 16-byte aligned stand-in for a device pointer (never dereferenced)
CHUNK = 1024


def _lib():
    from bigcn_amd import _lib
    return _lib, _lib.load_library()


def _entries(sizes, groups=None, p=P):
    L, _ = _lib()
    ents = (L.AdamMultiTensor * len(sizes))()
    for k, n in enumerate(sizes):
        e = ents[k]
        e.param = e.exp_avg = e.exp_avg_sq = p
        e.numel = n
        e.group = 0 if groups is None else groups[k]
        e.first_block = -7   # the plan overwrites it
    return ents


def _plan(ents, count=None, table="auto", table_bytes=None):
    L, lib = _lib()
    count = len(ents) if count is None else count
    need = max(count, 1) * ctypes.sizeof(L.AdamMultiTensor)
    buf = (ctypes.c_uint8 * need)()
    blocks = ctypes.c_int64(-1)
    rc = lib.bgcn_adam_multi_plan(ctypes.addressof(ents), count, ctypes.addressof(buf) if table == "auto" else table,
                                  need if table_bytes is None else table_bytes, ctypes.byref(blocks))
    return rc, blocks.value, (L.AdamMultiTensor * max(count, 1)).from_buffer(buf)


def test_header_declares_and_lib_binds_the_new_entry_points():
    L, lib = _lib()
    header = open(os.path.join(ROOT, "include", "bgcn.h")).read()
    for name in ("bgcn_adam_multi_table_size", "bgcn_adam_multi_plan", "bgcn_adam_multi_step",
                 "bgcn_ebgcn_train_loss"):
        assert name + "(" in header, name
        assert name in L.EXPORTED_SYMBOLS and name in L._SIGS and getattr(lib, name) is not None
    assert "#define BGCN_ABI_VERSION 12" in header and lib.bgcn_abi_version() == 12 and L.ABI_VERSION == 12
    assert f"#define BGCN_ADAM_MULTI_MAX_TENSORS {L.BGCN_ADAM_MULTI_MAX_TENSORS}" in header
    assert f"#define BGCN_ADAM_MULTI_MAX_GROUPS {L.BGCN_ADAM_MULTI_MAX_GROUPS}" in header
    assert f"#define BGCN_ADAM_MULTI_CHUNK {L.BGCN_ADAM_MULTI_CHUNK}" in header and L.BGCN_ADAM_MULTI_CHUNK == CHUNK
    assert "#define BGCN_ADAM_MAX_TENSORS 16" in header   # the 16-tensor entry point is as it was
    assert lib.bgcn_adam_multi_table_size(0) == 0 and lib.bgcn_adam_multi_table_size(129) == 0
    assert lib.bgcn_adam_multi_table_size(68) == 68 * ctypes.sizeof(L.AdamMultiTensor)
    # the per-step kernel arguments stay far below the 4 KB limit
    assert ctypes.sizeof(L.AdamMultiArgs) < 2048


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_ctypes_structs_match_the_header(tmp_path):
    L, _ = _lib()
    structs = {"bgcn_adam_multi_tensor": L.AdamMultiTensor, "bgcn_adam_multi_args": L.AdamMultiArgs}
    header = os.path.join(ROOT, "include", "bgcn.h")
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{header}"', "int main(void) {"]
    for cname, py in structs.items():
        lines.append(f'printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for fname, _ in py._fields_:
            lines.append(f'printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0; }")
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {tuple(line.split()[:2]): int(line.split()[2]) for line in out if line}
    for cname, py in structs.items():
        assert got[(cname, "sizeof")] == ctypes.sizeof(py), cname
        for fname, _ in py._fields_:
            assert got[(cname, fname)] == getattr(py, fname).offset, (cname, fname)


def test_plan_refusals():
    L, lib = _lib()

    def refused(text, rc):
        assert rc == -1 and text in lib.bgcn_last_error(), (text, rc, lib.bgcn_last_error())

    ok = _entries([5, 0, 2000])
    assert _plan(ok)[0] == 0
    refused(b"1..BGCN_ADAM_MULTI_MAX_TENSORS", _plan(ok, count=0)[0])
    refused(b"1..BGCN_ADAM_MULTI_MAX_TENSORS", _plan(_entries([1] * 129))[0])
    assert _plan(_entries([1] * 128))[0] == 0
    refused(b"group outside [0, 8)", _plan(_entries([5, 5], groups=[0, 8]))[0])
    refused(b"group outside [0, 8)", _plan(_entries([5, 5], groups=[-1, 0]))[0])
    assert _plan(_entries([5, 5], groups=[7, 0]))[0] == 0
    refused(b"numel < 0", _plan(_entries([5, -1]))[0])
    refused(b"null table", _plan(ok, table=None)[0])
    refused(b"table buffer too small", _plan(ok, table_bytes=3 * ctypes.sizeof(L.AdamMultiTensor) - 1)[0])
    for field in ("param", "exp_avg", "exp_avg_sq"):
        bad = _entries([5, 0, 7])
        setattr(bad[2], field, None)
        refused(b"null param / exp_avg / exp_avg_sq", _plan(bad)[0])
        empty = _entries([5, 0, 7])
        setattr(empty[1], field, None)      # a null pointer of an empty tensor is fine
        assert _plan(empty)[0] == 0


def test_step_refusals():
    L, lib = _lib()

    def step(count=3, table=P, blocks=1, null=False):
        a = L.AdamMultiArgs()
        a.table, a.count, a.blocks = table, count, blocks
        return lib.bgcn_adam_multi_step(None if null else ctypes.addressof(a), None)

    for count in (0, -1, 129):
        assert step(count=count) == -1 and b"1..BGCN_ADAM_MULTI_MAX_TENSORS" in lib.bgcn_last_error()
    assert step(table=None) == -1 and b"null table" in lib.bgcn_last_error()
    assert step(blocks=-1) == -1 and b"bad block count" in lib.bgcn_last_error()
    assert step(null=True) == -1 and b"null args" in lib.bgcn_last_error()
    assert step(blocks=0) == 0   # nothing to update: no launch


def test_train_loss_refusals():
    _, lib = _lib()
    names = ("logp", "y", "td", "bu", "loss", "correct", "pred", "dlogp", "status", "skip_flag", "seen")

    def call(B=3, C=4, **null):
        q = {n: (None if null.get(n) else P) for n in names}
        return lib.bgcn_ebgcn_train_loss(q["logp"], q["y"], B, C, q["td"], q["bu"], 0.2, 0.2, q["loss"], q["correct"],
                                         q["pred"], q["dlogp"], q["status"], q["skip_flag"], q["seen"], None)

    assert call(B=0) == -1 and b"at least one tree" in lib.bgcn_last_error()
    assert call(B=-2) == -1 and b"at least one tree" in lib.bgcn_last_error()
    for C in (0, 17):
        assert call(C=C) == -1 and b"num_classes must be in [1, 16]" in lib.bgcn_last_error()
    for n in ("logp", "y", "loss", "correct", "dlogp", "status", "skip_flag"):
        assert call(**{n: True}) == -1 and b"null pointer" in lib.bgcn_last_error(), n


def test_plan_block_starts_equal_a_restatement():
    sizes = [0, 1, CHUNK - 1, CHUNK, 0, 0, CHUNK + 1, 5 * CHUNK + 3, 64, 0]
    groups = [k % 8 for k in range(len(sizes))]
    ents = _entries(sizes, groups)
    for k, e in enumerate(ents):
        e.param, e.exp_avg, e.exp_avg_sq = P + 16 * k, 2 * P + 16 * k, 3 * P + 16 * k
    rc, blocks, table = _plan(ents)
    assert rc == 0
    start = 0
    for k, n in enumerate(sizes):
        t = table[k]
        assert t.first_block == start, (k, t.first_block, start)
        assert (t.param, t.exp_avg, t.exp_avg_sq) == (P + 16 * k, 2 * P + 16 * k, 3 * P + 16 * k)
        assert t.numel == n and t.group == groups[k]
        start += (n + CHUNK - 1) // CHUNK
    assert blocks == start == 0 + 1 + 1 + 1 + 2 + 6 + 1
    # every block's tensor, found as the kernel finds it: the last entry whose first block is not after it
    owner = []
    for k, n in enumerate(sizes):
        owner += [k] * ((n + CHUNK - 1) // CHUNK)
    for b in range(blocks):
        lo, hi = 0, len(sizes) - 1
        while lo < hi:
            mid = (lo + hi + 1) >> 1
            if table[mid].first_block <= b:
                lo = mid
            else:
                hi = mid - 1
        assert lo == owner[b], (b, lo, owner[b])


def _args(**kw):
    base = dict(input_features=32, hidden_features=64, output_features=64, num_class=4, edge_num=2,
                edge_infer_td=True, edge_infer_bu=True, device="cpu", lr=5e-4, lr_scale_bu=5, lr_scale_td=1,
                l2=1e-4, edge_loss_td=0.2, edge_loss_bu=0.2)
    base.update(kw)
    return argparse.Namespace(**base)


def test_multi_adam_limits():
    from bigcn_amd import MultiAdam

    def ps(n):
        return [torch.nn.Parameter(torch.zeros(3)) for _ in range(n)]

    MultiAdam([{"params": ps(100)}, {"params": ps(28), "lr": 0.1}])
    with pytest.raises(ValueError, match="at most 128 tensors"):
        MultiAdam([{"params": ps(100)}, {"params": ps(29)}])
    MultiAdam([{"params": ps(1)} for _ in range(8)])
    with pytest.raises(ValueError, match="at most 8 parameter groups"):
        MultiAdam([{"params": ps(1)} for _ in range(9)])
    with pytest.raises(ValueError, match="contiguous fp32"):
        MultiAdam([{"params": [torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))]}])
    with pytest.raises(ValueError, match="contiguous fp32"):
        MultiAdam([{"params": [torch.nn.Parameter(torch.zeros(4, 6).t())]}])
    opt = MultiAdam([{"params": ps(2)}, {"params": ps(1), "lr": 0.25}], lr=0.5, weight_decay=0.1)
    assert [g["lr"] for g in opt.param_groups] == [0.5, 0.25] and opt.step_count == 0 and len(opt.state) == 3
    for p in opt.params():
        p.grad = torch.ones(3)
    opt.zero_grad()
    assert all(p.grad is None for p in opt.params())


def test_ebgcn_adam_groups_on_a_cpu_model():
    import bigcn_amd
    from bigcn_amd import EBGCN, MultiAdam, ebgcn_adam
    for name in ("MultiAdam", "ebgcn_adam", "EBGCNTrainStep"):
        assert name in bigcn_amd.__all__ and getattr(bigcn_amd, name) is not None
    args = _args(lr=3e-3, lr_scale_bu=5, lr_scale_td=2, l2=1e-3)
    model = EBGCN(args)
    opt = ebgcn_adam(model, args)
    assert isinstance(opt, MultiAdam) and opt.weight_decay == 1e-3 and opt.betas == (0.9, 0.999) and opt.eps == 1e-8
    assert len(list(model.parameters())) == 68
    assert [len(g["params"]) for g in opt.param_groups] == [60, 2, 2, 2, 2]
    assert [g["lr"] for g in opt.param_groups] == [3e-3, 3e-3 / 5, 3e-3 / 5, 3e-3 / 2, 3e-3 / 2]
    td, bu = model.TDrumorGCN, model.BUrumorGCN
    for g, conv in zip(opt.param_groups[1:], (bu.conv1, bu.conv2, td.conv1, td.conv2)):   # the reference's order
        assert [id(p) for p in g["params"]] == [id(p) for p in conv.parameters()]
    conv_ids = {id(p) for c in (bu.conv1, bu.conv2, td.conv1, td.conv2) for p in c.parameters()}
    assert [id(p) for p in opt.param_groups[0]["params"]] == [id(p) for p in model.parameters()
                                                             if id(p) not in conv_ids]
    assert len({id(p) for p in opt.params()}) == 68
    # the limits hold here too
    model.extra = torch.nn.ParameterList([torch.nn.Parameter(torch.zeros(2)) for _ in range(61)])
    with pytest.raises(ValueError, match="at most 128 tensors"):
        ebgcn_adam(model, args)
    del model.extra
    model.fc.weight = torch.nn.Parameter(model.fc.weight.detach().double())
    with pytest.raises(ValueError, match="contiguous fp32"):
        ebgcn_adam(model, args)
    model.fc.weight = torch.nn.Parameter(torch.zeros(256, 4).t())
    with pytest.raises(ValueError, match="contiguous fp32"):
        ebgcn_adam(model, args)
