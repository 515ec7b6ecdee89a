"""Bit-exact tests of the fused Adam (bgcn_adam_step, driven through bigcn_amd.optim.FusedAdam) and
of the weight images its tile epilogue writes.

The reference is tests/adam_ref.py, a CPU restatement of adam_elem (bgcn_internal.h) in correctly
rounded fp32 operations, checked on the CPU by tests/test_adam_ref.py.  The kernel spells out every
operation and the build has no fast-math, so parameters, both moments and every defined image byte
must equal the restatement bit for bit.  Finding on the MI355X: they do, the parameters included,
so the device's sqrtf and division are the correctly rounded ones and no comparison is widened.

Every array (param, grad, exp_avg, exp_avg_sq) is a view into a device buffer of its own that is
otherwise filled with a NaN-payload sentinel, GUARD floats on either side; the image buffer is
filled with the same sentinel.  After a launch every word outside the views, every image byte
outside the mask of adam_ref.images() (w2s columns 64..103, w2d columns 64..71, the alignment gaps,
the trailing 256 bytes) and every gradient must be what it was.

Values: the squared gradient times 1 - beta2 stays a normal fp32 number (|g| >= 1e-15 or exactly 0,
grad_scale >= 0.125), so the comparison does not depend on how subnormal intermediates are treated.

Paths (k_adam): a tensor without an image role takes the float4 path when all four arrays are
16-byte aligned and the quad lies inside it, else the scalar loop; a tensor with an image role runs
adam_image_tile, float4 when aligned and the quad lies inside the row (always, K % 4 == 0), else
adam_chunk's scalar loop.
"""
import ctypes

import numpy as np
import pytest
import torch

import adam_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 0x7FC5A5A5       # a quiet NaN with a payload, as an int32 word
GUARD = 64              # sentinel floats on either side of every array
LR, WD = 5e-4, 1e-4     # the reference's optimiser (betas 0.9 / 0.999 and eps 1e-8 are the defaults)


class Arr:
    """`data` (fp32) at float offset GUARD + lead of a sentinel-filled device buffer of its own;
    `.t` is the fp32 view (lead = 1: four bytes off the 16-byte grid)."""

    def __init__(self, data, lead=0, shape=None):
        data = np.ascontiguousarray(data, dtype=np.float32)
        self.n, self.at = data.size, GUARD + lead
        self.buf = torch.full((self.at + self.n + GUARD + 4,), SENT, dtype=torch.int32, device=DEV)
        assert self.buf.data_ptr() % 256 == 0
        self.t = self.buf[self.at:self.at + self.n].view(torch.float32).view(shape or data.shape)
        self.t.copy_(torch.from_numpy(data).view(self.t.shape))
        # (an empty view has no address: torch reports 0, which the C API accepts for numel 0)
        assert self.t.is_contiguous() and (self.n == 0 or self.t.data_ptr() - self.buf.data_ptr() == 4 * self.at)

    def check(self, want, what):
        """The array equals `want` bit for bit and the guards still hold the sentinel."""
        got = self.buf.cpu().numpy()
        exp = np.full_like(got, SENT)
        exp[self.at:self.at + self.n] = np.ascontiguousarray(want, dtype=np.float32).ravel().view(np.int32)
        inside = int((got != exp)[self.at:self.at + self.n].sum())
        assert np.array_equal(got, exp), (f"{what}: {inside} of {self.n} elements differ, "
                                          f"{int((got != exp).sum()) - inside} guard words overwritten")


def model_values(n, seed, cls="randn"):
    """(p, g, m, v) of n elements.  randn: the model's scales (p ~ 0.1, g ~ 1e-3), moments from two
    prior restated steps; p_zero: the same with p = 0; zero_grad: g = m = v = 0; huge_grad: |g|
    log-uniform in [1e-15, 1e10]."""
    rng = np.random.default_rng(seed)
    p = (0.1 * rng.standard_normal(n)).astype(np.float32)
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    for t in (1, 2):
        g = (1e-3 * rng.standard_normal(n)).astype(np.float32)
        p, m, v = R.adam_elem(p, g, m, v, R.AdamConst(LR, t, weight_decay=WD))
    g = (1e-3 * rng.standard_normal(n)).astype(np.float32)
    if cls == "p_zero":
        p = np.zeros(n, np.float32)
    elif cls == "zero_grad":
        g, m, v = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    elif cls == "huge_grad":
        g = (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-15, 10, n)).astype(np.float32)
        assert n == 0 or (1e-15 * (1 - 1e-6) <= np.abs(g).min() and np.abs(g).max() <= 1e10 * (1 + 1e-6))
    else:
        assert cls == "randn"
    return p, g, m, v


def run_plain(n, leads=(0, 0, 0, 0), cls="randn", wd=WD, gs=1.0, t=1, seed=0, strided_grad=False):
    """One tensor of n elements, one launch, against the restatement."""
    from bigcn_amd.optim import FusedAdam
    p0, g0, m0, v0 = model_values(n, seed + n, cls)
    P, M, V = Arr(p0, leads[0]), Arr(m0, leads[2]), Arr(v0, leads[3])
    if strided_grad:       # every other element of an array twice as long (the rest: 1e30, finite)
        both = np.full(2 * n, 1e30, np.float32)
        both[::2] = g0
        G = Arr(both, leads[1])
        grad = G.t[::2]
        assert n < 2 or not grad.is_contiguous()
    else:
        G, both = Arr(g0, leads[1]), g0
        grad = G.t
    opt = FusedAdam([{"params": [P.t]}], lr=LR, weight_decay=wd)
    opt.state[P.t] = (M.t, V.t)
    opt.step_count = t - 1
    opt.step(grads=[grad], grad_scale=gs)
    assert opt.step_count == t
    p1, m1, v1 = R.adam_elem(p0, g0, m0, v0, R.AdamConst(LR, t, weight_decay=wd, grad_scale=gs))
    what = f"n {n} leads {leads} {cls} wd {wd} gs {gs} t {t}"
    M.check(m1, what + " exp_avg")
    V.check(v1, what + " exp_avg_sq")
    P.check(p1, what + " param")
    G.check(both, what + " grad")
    return p0, p1


ALIGNMENTS = [(0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)]
NUMELS = [1, 3, 4, 5, 1023, 1024, 1025, 2051]       # around the quad and the 1024-element chunk


@pytest.mark.parametrize("n", NUMELS)
def test_plain_tensor(n):
    """All four arrays aligned (float4 path, scalar tail) and each one alone a float off (any one
    sends the whole tensor down the scalar path), at both weight decays, three grad_scales and
    t = 1, 2, 1000."""
    for leads in ALIGNMENTS:
        for wd in (WD, 0.0):
            for gs in (1.0, 0.125, 1.0 / 3):
                for t in (1, 2, 1000):
                    run_plain(n, leads, "randn", wd, gs, t)


@pytest.mark.parametrize("n", NUMELS)
def test_plain_tensor_value_classes(n):
    for leads in (ALIGNMENTS[0], ALIGNMENTS[2]):
        run_plain(n, leads, "p_zero", t=3)
        run_plain(n, leads, "huge_grad", gs=0.125, t=3)
        run_plain(n, leads, "huge_grad", wd=0.0, t=1)
        # nothing to learn and no decay: the parameter comes back bit-unchanged
        p0, p1 = run_plain(n, leads, "zero_grad", wd=0.0, t=1)
        assert p0.tobytes() == p1.tobytes()
        run_plain(n, leads, "zero_grad", wd=WD, t=1)       # (decay alone moves it)


@pytest.mark.parametrize("n", [1, 5, 1024, 2051])
def test_non_contiguous_gradient(n):
    """optim.py hands the kernel a contiguous copy; the gradient itself is not written."""
    run_plain(n, strided_grad=True, t=2)
    run_plain(n, leads=(0, 1, 0, 0), strided_grad=True, gs=1.0 / 3)


class Tensors:
    """A parameter set: per tensor its four arrays, group and the restated state."""

    def __init__(self, shapes, groups, lrs, seed, leads=None, wd=WD):
        from bigcn_amd.optim import FusedAdam
        self.shapes, self.groups, self.lrs, self.wd = shapes, groups, lrs, wd
        self.n = len(shapes)
        leads = leads or [(0, 0, 0, 0)] * self.n
        self.leads = leads
        self.rng = np.random.default_rng(seed)
        self.p, self.m, self.v, self.P, self.M, self.V = [], [], [], [], [], []
        for k, shape in enumerate(shapes):
            p, _, m, v = model_values(int(np.prod(shape)), seed + 17 * k)
            self.p.append(p), self.m.append(m), self.v.append(v)
            self.P.append(Arr(p, leads[k][0], shape)), self.M.append(Arr(m, leads[k][2], shape))
            self.V.append(Arr(v, leads[k][3], shape))
        pg = [{"params": [self.P[k].t for k in range(self.n) if groups[k] == gi], "lr": lr}
              for gi, lr in enumerate(lrs)]
        assert [id(q) for g in pg for q in g["params"]] == [id(A.t) for A in self.P]    # groups in order
        self.opt = FusedAdam(pg, lr=LR, weight_decay=wd)
        for k in range(self.n):
            self.opt.state[self.P[k].t] = (self.M[k].t, self.V[k].t)
        self.G = None

    def step(self, absent=(), gs=1.0, update=True, **kw):
        """One optimiser step with fresh gradients (none for the tensors in `absent`); the
        restated state advances unless `update` is False (a skipped step)."""
        t = self.opt.step_count + 1
        self.g = [(1e-3 * self.rng.standard_normal(self.p[k].size)).astype(np.float32) for k in range(self.n)]
        self.G = [None if k in absent else Arr(self.g[k], self.leads[k][1], self.shapes[k]) for k in range(self.n)]
        self.opt.step(grads=[None if G is None else G.t for G in self.G], grad_scale=gs, **kw)
        assert self.opt.step_count == t
        for k in range(self.n):
            if update and k not in absent:
                c = R.AdamConst(self.lrs[self.groups[k]], t, weight_decay=self.wd, grad_scale=gs)
                self.p[k], self.m[k], self.v[k] = R.adam_elem(self.p[k], self.g[k], self.m[k], self.v[k], c)

    def check(self, what=""):
        for k in range(self.n):
            tag = f"{what} tensor {k} {self.shapes[k]}"
            self.M[k].check(self.m[k], tag + " exp_avg")
            self.V[k].check(self.v[k], tag + " exp_avg_sq")
            self.P[k].check(self.p[k], tag + " param")
            if self.G[k] is not None:
                self.G[k].check(self.g[k], tag + " grad")


def test_sixteen_tensors_with_empty_ones_and_absent_gradients():
    """BGCN_ADAM_MAX_TENSORS entries, empty tensors first, in the middle (two in a row) and last
    (the block_start scan), a learning rate per group, aligned and misaligned tensors side by
    side; then the same set with gradients missing, so that the table's entries and params()
    indices diverge and the cached table is rebuilt; then all gradients again."""
    sizes = [0, 0, 1, 2051, 4, 0, 1023, 1024, 1025, 0, 0, 5, 3, 2048, 7, 0]
    groups = [0] * 6 + [1] * 5 + [2] * 5
    leads = [(0, 0, 0, 0)] * 16
    leads[3], leads[7], leads[12], leads[13] = (0, 1, 0, 0), (1, 0, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)
    T = Tensors([(n,) for n in sizes], groups, [LR, LR / 5, 3e-3], seed=1, leads=leads)
    T.step(gs=1.0 / 3)
    T.check("16 entries")
    assert T.opt._cache[1].count == 16
    T.step(absent=(0, 2, 3, 9, 14))
    T.check("11 entries")
    assert T.opt._cache[1].count == 11
    T.step(absent=(15,), gs=0.125)
    T.check("15 entries")


# ------------------------------------------------------------------------------- weight images
IMAGE_F = [4, 60, 64, 68, 124, 128, 132, 260]
# td_w1 td_b1 td_w2 td_b2 fc_w fc_b | bu_w1 bu_b1 | bu_w2 bu_b2: bigcn_adam's three groups
ROLE_AT = {0: R.IMAGE_TD_W1, 6: R.IMAGE_BU_W1, 2: R.IMAGE_TD_W2, 8: R.IMAGE_BU_W2}


class ImageCase:
    """The ten parameters of a BiGCN with in_feats = F grouped as bigcn_adam groups them, and a
    sentinel-filled image buffer."""

    def __init__(self, F, seed=0, grad_lead=0, wd=WD):
        from bigcn_amd import _lib
        self.F = F
        shapes = [(64, F), (64,), (64, F + 64), (64,), (4, 128), (4,), (64, F), (64,), (64, F + 64), (64,)]
        leads = [(0, grad_lead if k in ROLE_AT else 0, 0, 0) for k in range(10)]
        self.T = Tensors(shapes, [0] * 6 + [1] * 2 + [2] * 2, [LR, LR / 5, LR / 5], seed + F, leads, wd)
        self.size = _lib.lib().bgcn_weight_images_size(F)
        assert self.size % 4 == 0 and self.size == R.image_layout(F)[1] + 256
        self.img = torch.full((self.size // 4,), SENT, dtype=torch.int32, device=DEV)
        self.roles = {id(self.T.P[k].t): role for k, role in ROLE_AT.items()}
        self.written = set()        # the image tensors updated so far

    def step(self, absent=(), **kw):
        self.T.step(absent=absent, images=(self.img, self.F, self.roles), **kw)
        if kw.get("update", True):
            self.written |= set(ROLE_AT) - set(absent)

    def check(self, what=""):
        self.T.check(what)
        w = [torch.from_numpy(self.T.p[k]).view(self.T.shapes[k]) if k in self.written else None
             for k in (0, 6, 2, 8)]
        data, mask = R.images(self.F, *w)
        exp = np.full(self.size // 4, SENT, np.int32).view(np.uint8)
        exp[:data.size][mask] = data[mask]
        got = self.img.cpu().numpy().view(np.uint8)
        bad = got != exp
        layout, total = R.image_layout(self.F)
        where = {name: int(bad[off:off + int(np.prod(shape)) * size].sum()) for name, (off, shape, size) in layout.items()}
        where["defined"] = int(bad[:total][mask].sum())
        where["tail"] = int(bad[total:].sum())
        assert not bad.any(), f"{what} F {self.F}: image bytes that differ {where}"


@pytest.mark.parametrize("F", IMAGE_F)
def test_image_tensors(F):
    """W1's K = F, W2's K = F + 64 in {68, 124, 128, 132, 188, 192, 196, 324}: a partial tile, one
    tile exactly, a tile and a 4-column tail, between one and two tiles, three tiles (128 columns
    per tile; also the edges of 256-column tiles).  Two steps: the second reads the state and
    overwrites the images the first wrote."""
    C = ImageCase(F)
    C.step()
    C.check("step 1")
    C.step(gs=1.0 / 3)
    C.check("step 2")


@pytest.mark.parametrize("F", [4, 132])
def test_image_tensors_with_misaligned_gradients(F):
    """adam_chunk's scalar loop inside adam_image_tile."""
    C = ImageCase(F, seed=1, grad_lead=1)
    C.step()
    C.check("step 1")
    C.step()
    C.check("step 2")


@pytest.mark.parametrize("absent", sorted(ROLE_AT))
@pytest.mark.parametrize("F", [4, 132])
def test_image_tensor_without_gradient(F, absent):
    """Its image region stays untouched and the other tensors' roles stay theirs."""
    C = ImageCase(F, seed=2 + absent)
    C.step(absent=(absent,))
    C.check("step 1")
    C.step(absent=(absent, 1))
    C.check("step 2")


# ----------------------------------------------------------------------------------- skip flag
@pytest.mark.parametrize("flag,skips", [(1.0, True), (float("nan"), True), (0.0, False), (-0.0, False)],
                         ids=["one", "nan", "zero", "negzero"])
def test_skip_flag(flag, skips):
    C = ImageCase(68, seed=7)
    sf = torch.tensor([flag], dtype=torch.float32, device=DEV)
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    C.step(skip_flag=sf, skip_count=count, update=not skips)
    assert C.T.opt.step_count == 1          # the step counter advances either way
    C.check("flagged step")                 # skipped: params, moments and the whole image buffer untouched
    assert int(count) == int(skips)
    assert sf.cpu().numpy().tobytes() == np.float32(flag).tobytes()
    # the next valid step updates with t = 2
    C.step(skip_flag=torch.zeros(1, device=DEV), skip_count=count)
    C.check("next step")
    assert int(count) == int(skips)


# ------------------------------------------------------------------------------------ refusals
def _raw_case(F=8):
    """bgcn_adam_args filled by hand: tensor 0 a TD_W1 [64][F], tensor 1 a TD_W2 [64][F + 64],
    tensor 2 a plain one.  Returns the arguments, per tensor its four arrays and their values,
    and the sentinel-filled image buffer."""
    from bigcn_amd import _lib
    from bigcn_amd.optim import AdamArgs
    arrs = []
    a = AdamArgs()
    for k, n in enumerate((64 * F, 64 * (F + 64), 300)):
        values = model_values(n, 40 + k)
        four = [Arr(x) for x in values]
        arrs.append((four, values))
        e = a.t[k]
        e.param, e.grad, e.exp_avg, e.exp_avg_sq = (A.t.data_ptr() for A in four)
        e.numel, e.lr = n, LR
    a.count = 3
    a.beta1, a.beta2, a.eps, a.weight_decay = 0.9, 0.999, 1e-8, WD
    a.bias_correction1, a.bias_correction2_sqrt, a.grad_scale = 1.0 - 0.9, (1.0 - 0.999) ** 0.5, 1.0
    img = torch.full((_lib.lib().bgcn_weight_images_size(F) // 4,), SENT, dtype=torch.int32, device=DEV)
    a.images, a.images_in_feats = img.data_ptr(), F
    a.image_role[0], a.image_role[1] = R.IMAGE_TD_W1, R.IMAGE_TD_W2
    return a, arrs, img


def _refused(a, arrs, img, message, what):
    """BGCN_EINVAL with `message`, nothing launched: every array and the image buffer untouched."""
    from bigcn_amd import _lib
    assert _lib.lib().bgcn_adam_step(ctypes.addressof(a), _lib.stream_handle()) == -1
    assert message in _lib.lib().bgcn_last_error(), _lib.lib().bgcn_last_error()
    torch.cuda.synchronize()
    for k, (four, values) in enumerate(arrs):
        for A, x in zip(four, values):
            A.check(x, f"{what} tensor {k}")
    assert bool((img == SENT).all())


def _set(**fields):
    def edit(a):
        for k, v in fields.items():
            setattr(a, k, v)
    return edit


def _tensor(k, **fields):
    def edit(a):
        for name, v in fields.items():
            setattr(a.t[k], name, v)
    return edit


def _role(k, role):
    def edit(a):
        a.image_role[k] = role
    return edit


REFUSALS = {
    "count_0": (_set(count=0), b"1..BGCN_ADAM_MAX_TENSORS"),
    "count_17": (_set(count=17), b"1..BGCN_ADAM_MAX_TENSORS"),
    "numel_negative": (_tensor(2, numel=-1), b"bad tensor"),
    "null_param": (_tensor(2, param=None), b"bad tensor"),
    "null_grad": (_tensor(2, grad=None), b"bad tensor"),
    "null_exp_avg": (_tensor(0, exp_avg=None), b"bad tensor"),
    "null_exp_avg_sq": (_tensor(1, exp_avg_sq=None), b"bad tensor"),
    "images_in_feats_0": (_set(images_in_feats=0), b"images_in_feats > 0"),
    "images_in_feats_negative": (_set(images_in_feats=-8), b"images_in_feats > 0"),
    "w1_numel": (_tensor(0, numel=64 * 8 - 4), b"an image tensor must be"),
    "w2_numel_of_w1": (_tensor(1, numel=64 * 8), b"an image tensor must be"),
    "plain_tensor_with_role": (_role(2, R.IMAGE_BU_W1), b"an image tensor must be"),
    "role_5": (_role(2, 5), b"bad image_role"),
    "role_negative": (_role(0, -1), b"bad image_role"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_c_api_refuses(case):
    edit, message = REFUSALS[case]
    a, arrs, img = _raw_case()
    edit(a)
    _refused(a, arrs, img, message, case)


def test_c_api_refuses_in_feats_not_a_multiple_of_four():
    """F = 6: the sizes agree (64 x 6, 64 x 70), the float4 rows would not."""
    a, arrs, img = _raw_case(F=6)
    _refused(a, arrs, img, b"an image tensor must be", "F 6")


def test_c_api_accepts_the_unedited_case():
    """The arguments the refusals edit are valid: the same call, unedited, updates all three
    tensors and writes their images."""
    from bigcn_amd import _lib
    a, arrs, img = _raw_case()
    _lib.check(_lib.lib().bgcn_adam_step(ctypes.addressof(a), _lib.stream_handle()))
    c = R.AdamConst(LR, 1, weight_decay=WD)
    new = []
    for k, (four, (p, g, m, v)) in enumerate(arrs):
        p1, m1, v1 = R.adam_elem(p, g, m, v, c)
        new.append(p1)
        for A, x in zip(four, (p1, g, m1, v1)):
            A.check(x, f"tensor {k}")
    data, mask = R.images(8, torch.from_numpy(new[0]).view(64, 8), None, torch.from_numpy(new[1]).view(64, 72), None)
    got = img.cpu().numpy().view(np.uint8)
    exp = np.full(img.numel(), SENT, np.int32).view(np.uint8)
    exp[:data.size][mask] = data[mask]
    assert np.array_equal(got, exp)


def test_python_refuses():
    from bigcn_amd.optim import FusedAdam
    arrs = [Arr(model_values(8, k)[0]) for k in range(17)]
    with pytest.raises(ValueError, match="at most 16 tensors"):
        FusedAdam([{"params": [A.t for A in arrs[:9]]}, {"params": [A.t for A in arrs[9:]]}])
    T = Tensors([(8,)] * 16, [0] * 16, [LR], seed=3)
    extra = Arr(model_values(8, 99)[0])
    T.opt.param_groups[0]["params"].append(extra.t)       # a 17th after construction
    with pytest.raises(ValueError, match="at most 16 tensors"):
        T.opt.step(grads=[A.t for A in T.P] + [extra.t])
    T.opt.param_groups[0]["params"].pop()
    g = [Arr(model_values(8, 50 + k)[1]) for k in range(16)]
    for flag in (torch.zeros(1, dtype=torch.float64, device=DEV), torch.zeros(2, device=DEV),
                 torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1)):
        with pytest.raises(ValueError, match="skip_flag"):
            T.opt.step(grads=[G.t for G in g], skip_flag=flag)
    T.G, T.g = g, [model_values(8, 50 + k)[1] for k in range(16)]
    T.check("after the refusals")
    extra.check(model_values(8, 99)[0], "extra")


# ------------------------------------------------------------- the in-step form at small shapes
@pytest.mark.parametrize("mode", ["sparse", "auto"])
@pytest.mark.parametrize("F", [64, 132])
def test_optimizer_inside_step_at_small_shapes(F, mode):
    """test_gpu_train.test_optimizer_inside_step_matches_separate_launch (TailAdam inside the
    step's last launch vs the step followed by bgcn_adam_step: losses, parameters, moments, image
    buffer, skip count bitwise the same) on trees of 1, 2 and 40 nodes at in_feats 64 (W2: one
    tile exactly) and 132 (a tile and a tail).  With the cases above this pins the in-step form,
    through the separate launch, to the restatement."""
    from bigcn_amd.data import synth_batch
    from test_gpu_train import check_optimizer_inside_step

    def batch(seed):
        return synth_batch(np.random.default_rng(seed), [1, 2, 40], F, 4, device=DEV)

    bad = batch(83)
    bad.y = bad.y.clone()
    bad.y[2] = 9
    check_optimizer_inside_step(mode, 4, [batch(80 + k) for k in range(3)], bad, F)
