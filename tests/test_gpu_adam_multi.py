"""Bit-exact tests of the many-tensor Adam (bgcn_adam_multi_step, driven through bigcn_amd.MultiAdam)
against tests/adam_ref.py (imported, not copied): adam_elem in correctly rounded fp32 operations with the
constants as k_adam forms them.  Parameters and both moments must equal the restatement bit for bit.

As in tests/test_gpu_adam.py every array is a view into a device buffer of its own, otherwise filled with
a NaN-payload sentinel, GUARD floats on either side: after the launches every word outside the views must
be what it was, and so must every gradient.  Values keep (1 - beta2) g^2 a normal fp32 number.

Paths (k_adam_multi): a workgroup finds its tensor by binary search over the table's first blocks and
updates one 1024-element chunk of it: float4 when all four arrays are 16-byte aligned and the quad lies
inside the tensor, else the scalar loop; a tensor whose gradient pointer is null is left alone.
"""
import numpy as np
import pytest
import torch

import adam_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 0x7FC5A5A5       # a quiet NaN with a payload, as an int32 word
GUARD = 64              # sentinel floats on either side of every array
LR, WD = 5e-4, 1e-4
CHUNK = 1024            # BGCN_ADAM_MULTI_CHUNK


class Arr:
    """`data` (fp32) at float offset GUARD + lead of a sentinel-filled device buffer of its own; `.t` is the
    fp32 view (lead = 1: four bytes off the 16-byte grid)."""

    def __init__(self, data, lead=0):
        data = np.ascontiguousarray(data, dtype=np.float32)
        self.n, self.at = data.size, GUARD + lead
        self.buf = torch.full((self.at + self.n + GUARD + 4,), SENT, dtype=torch.int32, device=DEV)
        assert self.buf.data_ptr() % 256 == 0
        self.t = self.buf[self.at:self.at + self.n].view(torch.float32)
        self.t.copy_(torch.from_numpy(data))

    def check(self, want, what):
        got = self.buf.cpu().numpy()
        exp = np.full_like(got, SENT)
        exp[self.at:self.at + self.n] = np.ascontiguousarray(want, dtype=np.float32).ravel().view(np.int32)
        inside = int((got != exp)[self.at:self.at + self.n].sum())
        assert np.array_equal(got, exp), (f"{what}: {inside} of {self.n} elements differ, "
                                          f"{int((got != exp).sum()) - inside} guard words overwritten")


def values(n, seed):
    """(p, m, v) at the model's scales with moments from two prior restated steps, and a gradient maker."""
    rng = np.random.default_rng(seed)
    p = (0.1 * rng.standard_normal(n)).astype(np.float32)
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    for t in (1, 2):
        g = (1e-3 * rng.standard_normal(n)).astype(np.float32)
        p, m, v = R.adam_elem(p, g, m, v, R.AdamConst(LR, t, weight_decay=WD))
    return p, m, v, lambda: (1e-3 * rng.standard_normal(n)).astype(np.float32)


class Case:
    """Tensors of `sizes` in groups `groups` (one index per tensor) with learning rates `lrs` (one per
    group) on MultiAdam, and their restated state."""

    def __init__(self, sizes, groups=None, lrs=(LR,), leads=(0, 0, 0, 0), wd=WD, seed=0, cls=None):
        from bigcn_amd import MultiAdam
        self.sizes, self.groups = list(sizes), list(groups) if groups is not None else [0] * len(sizes)
        self.lrs, self.leads, self.wd = list(lrs), leads, wd
        self.p, self.m, self.v, self.gen, self.P, self.M, self.V = [], [], [], [], [], [], []
        for k, n in enumerate(self.sizes):
            p, m, v, gen = values(n, 1000 * seed + 7 * k + n)
            self.p.append(p), self.m.append(m), self.v.append(v), self.gen.append(gen)
            self.P.append(Arr(p, leads[0])), self.M.append(Arr(m, leads[2])), self.V.append(Arr(v, leads[3]))
        per_group = [[self.P[k].t for k in range(len(self.sizes)) if self.groups[k] == gi]
                     for gi in range(len(self.lrs))]
        # MultiAdam orders its table group by group: keep our tensors in that order
        self.order = [k for gi in range(len(self.lrs)) for k in range(len(self.sizes)) if self.groups[k] == gi]
        self.opt = (cls or MultiAdam)([{"params": ps, "lr": lr} for ps, lr in zip(per_group, self.lrs)], lr=LR,
                                      weight_decay=wd)
        for k in range(len(self.sizes)):
            self.opt.state[self.P[k].t] = (self.M[k].t, self.V[k].t)
        self.t = 0

    def step(self, absent=(), gs=1.0, skip_flag=None, skip_count=None, expect_update=True, **kw):
        """One launch; the tensors in `absent` have no gradient.  Checks every bit afterwards."""
        self.t += 1
        G, g0 = {}, {}
        for k, n in enumerate(self.sizes):
            g0[k] = self.gen[k]()
            G[k] = None if k in absent else Arr(g0[k], self.leads[1])
        grads = [None if G[k] is None else G[k].t for k in self.order]
        extra = {} if skip_flag is None else {"skip_flag": skip_flag, "skip_count": skip_count}
        self.opt.step(grads=grads, grad_scale=gs, **extra, **kw)
        assert self.opt.step_count == self.t
        for k, n in enumerate(self.sizes):
            if expect_update and k not in absent:
                lr = self.opt.param_groups[self.groups[k]]["lr"]
                c = R.AdamConst(lr, self.t, weight_decay=self.wd, grad_scale=gs)
                self.p[k], self.m[k], self.v[k] = R.adam_elem(self.p[k], g0[k], self.m[k], self.v[k], c)
            what = f"tensor {k} of {n} elements, step {self.t}, leads {self.leads}"
            self.M[k].check(self.m[k], what + " exp_avg")
            self.V[k].check(self.v[k], what + " exp_avg_sq")
            self.P[k].check(self.p[k], what + " param")
            if G[k] is not None:
                G[k].check(g0[k], what + " grad")


EDGE_SIZES = [0, 1, 3, 4, 5, 64, CHUNK - 1, CHUNK, CHUNK + 1]
ALIGNMENTS = [(0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)]


@pytest.mark.parametrize("leads", ALIGNMENTS, ids=["aligned", "param+1", "grad+1", "exp_avg+1", "exp_avg_sq+1"])
@pytest.mark.parametrize("n", EDGE_SIZES)
def test_single_tensor_chunk_vector_and_alignment_edges(n, leads):
    """Three consecutive steps (t = 1..3) of one tensor: the quad, the chunk, and each of the four arrays in
    turn one element off a 16-byte boundary (the scalar loop)."""
    c = Case([n], leads=leads, seed=1)
    for _ in range(3):
        c.step()


def _mixed_sizes(count, seed):
    rng = np.random.default_rng(seed)
    pool = [0, 64, 64, 1, 5, 256, 832, 4096, CHUNK - 1, CHUNK + 1, 2 * CHUNK + 3, 0, 64]
    sizes = [pool[k % len(pool)] for k in range(count)]
    sizes[0], sizes[-1] = 0, 64          # an empty first tensor, a 64-element last one
    sizes[count // 2] = 5 * CHUNK + 7    # one that spans several blocks
    mid = sizes[1:-1]
    rng.shuffle(mid)
    return sizes[:1] + mid + sizes[-1:]


@pytest.mark.parametrize("count,ngroups", [(68, 5), (128, 8)])
def test_largest_tables_mixed_groups(count, ngroups):
    """68 tensors in 5 groups (an EBGCN) and the limits, 128 in 8, with distinct learning rates, mixed sizes,
    64-element and empty tensors among them; the settings grad_scale = 0.5 and weight_decay = 1e-4."""
    sizes = _mixed_sizes(count, count)
    assert sizes.count(0) >= 2 and sizes.count(64) >= 2
    groups = [(3 * k + k // 7) % ngroups for k in range(count)]
    assert len(set(groups)) == ngroups
    lrs = [LR / (1 + g) for g in range(ngroups)]
    c = Case(sizes, groups, lrs, wd=1e-4, seed=2)
    c.step(gs=0.5)
    c.step(gs=0.5)


def test_a_learning_rate_edited_between_steps_takes_effect():
    c = Case([5, CHUNK + 1, 64], [0, 1, 1], [LR, LR / 5], seed=3)
    c.step()
    before = [p.copy() for p in c.p]
    c.opt.param_groups[1]["lr"] = LR * 3      # Case.step restates with the edited value
    c.step()
    # and the edit matters: the same step at the old rate gives other bits
    assert not np.array_equal(c.p[1], before[1])
    old = Case([5, CHUNK + 1, 64], [0, 1, 1], [LR, LR / 5], seed=3)
    old.step()
    old.step()
    assert np.array_equal(old.p[0], c.p[0]) and not np.array_equal(old.p[1], c.p[1])


def test_absent_gradients_leave_their_tensors_alone():
    """The first, a middle and the last tensor without a gradient: parameter and both moments keep their bits
    (no weight decay either), the others update; then everything updates again."""
    sizes = [CHUNK + 5, 64, 2 * CHUNK, 7, 0, 300, CHUNK]
    c = Case(sizes, [0, 0, 1, 1, 2, 2, 2], [LR, LR / 2, LR / 5], wd=1e-2, seed=4)
    keep = {k: (c.p[k].copy(), c.m[k].copy(), c.v[k].copy()) for k in (0, 3, 6)}
    c.step(absent=(0, 3, 6))
    for k, (p, m, v) in keep.items():
        assert np.array_equal(c.p[k], p) and np.array_equal(c.m[k], m) and np.array_equal(c.v[k], v)
    c.step()
    c.step(absent=(2,))


def test_skip_flag_and_skip_count():
    c = Case([5, CHUNK + 1, 64, 0], [0, 1, 1, 0], [LR, LR / 5], seed=5)
    flag = torch.ones(1, dtype=torch.float32, device=DEV)
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    c.step(skip_flag=flag, skip_count=count, expect_update=False)     # Case.step checks: nothing changed
    assert int(count.item()) == 1
    flag.zero_()
    c.step(skip_flag=flag, skip_count=count)                          # t = 2: updates
    assert int(count.item()) == 1
    flag.fill_(3.0)
    c.step(skip_flag=flag, skip_count=count, expect_update=False)
    assert int(count.item()) == 2


def test_sixteen_or_fewer_tensors_agree_with_fused_adam():
    """The same tensors and gradients through FusedAdam (bgcn_adam_step) and MultiAdam: equal bits (both are
    checked against the restatement, and against each other)."""
    from bigcn_amd import FusedAdam
    sizes = [0, 1, 64, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 2, 5, 4, 3, 832, 4096, 64, 7, 256, 2 * CHUNK]
    groups = [k % 3 for k in range(16)]
    lrs = [LR, LR / 5, LR / 2]
    a = Case(sizes, groups, lrs, seed=6)
    b = Case(sizes, groups, lrs, seed=6, cls=FusedAdam)
    for _ in range(2):
        a.step(gs=0.5)
        b.step(gs=0.5)
    for k in range(16):
        for x, y in ((a.P[k], b.P[k]), (a.M[k], b.M[k]), (a.V[k], b.V[k])):
            assert torch.equal(x.t.view(torch.int32), y.t.view(torch.int32)), k
