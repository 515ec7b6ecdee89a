"""CPU conditions that make the GPU bar of tests/test_gpu_bert_train.py meaningful: the structure of
the full-sequence fp64 oracle's gradients (what bgcn_bert_train_grad writes as zeros is exactly
zero there, and nothing but a tree's first row and its masks enters any gradient), torch's own fp32
autograd against the bar, the restated keep function, and the size of the reference gradients."""
import math

import pytest
import torch

import bert_train_ref as T

ZERO_KEYS = ("attention.self.query.weight", "attention.self.query.bias", "attention.self.key.weight",
             "attention.self.key.bias")
POS = "BERT.embeddings.position_embeddings.weight"
TYPE = "BERT.embeddings.token_type_embeddings.weight"


def _non_root(c):
    m = torch.ones(c.N, dtype=torch.bool)
    m[c.rootindex] = False
    return m


@pytest.mark.parametrize("name,drop", T.PARITY)
def test_the_oracle_has_exact_zeros_where_the_native_call_writes_zeros(name, drop):
    c = T.case(name)
    g = T.oracle(name, drop).grads
    assert sorted(g) == sorted(T.grad_names(c) + ["x"])
    qk = [k for k in g if k.endswith(ZERO_KEYS)]
    assert len(qk) == 4 * c.cfg["layers"]
    for k in qk:
        assert float(g[k].abs().max()) == 0.0, k
    assert float(g[POS][1:].abs().max()) == 0.0
    assert float(g[TYPE][1].abs().max()) == 0.0
    assert T.rel_err(g[POS][0], g[TYPE][0]) < 1e-12   # the same sum over the trees, in autograd's two orders
    if bool(_non_root(c).any()):
        assert float(g["x"][_non_root(c)].abs().max()) == 0.0


@pytest.mark.parametrize("name,drop", [("t_boundaries", "p01"), ("t_many_trees", "p01"), ("t_boundaries", "p0")])
def test_only_the_first_rows_and_their_masks_enter_the_gradients(name, drop):
    c = T.case(name)
    want = T.oracle(name, drop)
    p_h, p_a = T.DROPS[drop]
    x = c.x.clone()
    x[_non_root(c)] = torch.randn(int(_non_root(c).sum()), x.size(1), generator=torch.Generator().manual_seed(9)) * 3
    for got in (T.loss_and_grads(c, torch.float64, p_h, p_a, other_seed=5),
                T.loss_and_grads(c, torch.float64, p_h, p_a, x=x)):
        assert torch.equal(got.loss, want.loss) and torch.equal(got.logp, want.logp)
        for k, v in want.grads.items():
            assert torch.equal(got.grads[k], v), k


@pytest.mark.parametrize("name,drop", T.PARITY)
def test_fp32_autograd_is_ten_times_under_the_bar(name, drop):
    c = T.case(name)
    want = T.oracle(name, drop)
    got = T.loss_and_grads(c, torch.float32, *T.DROPS[drop])
    errs = {k: T.rel_err(got.grads[k], v) for k, v in want.grads.items()}
    errs["loss"] = abs(float(got.loss) - float(want.loss))
    errs["logp"] = float((got.logp.double() - want.logp).abs().max())
    worst = max(errs, key=errs.get)
    print(name, drop, worst, f"{errs[worst]:.2e}")
    for k, e in errs.items():
        assert e <= T.BAR / 10, (k, e)


@pytest.mark.parametrize("name,drop", T.PARITY)
def test_every_nonzero_reference_gradient_is_well_above_noise(name, drop):
    g = T.oracle(name, drop).grads
    peaks = {k: float(v.abs().max()) for k, v in g.items()}
    if name == "t_classes_1":
        assert all(p == 0.0 for p in peaks.values())
        return
    assert any(p > 0 for p in peaks.values())
    for k, p in peaks.items():
        assert p == 0.0 or p > 1e-6, (k, p)
        if not k.endswith(ZERO_KEYS):
            assert p > 1e-6, (k, p)


@pytest.mark.parametrize("p", [0.1, 0.5, 0.015625])
def test_the_keep_function_keeps_its_share(p):
    n_b, n_j = 400, 300   # 1.2e5 draws
    b = torch.arange(n_b)[:, None]
    j = torch.arange(n_j)[None, :]
    k = T.keep(T.DROP_SEED, 4, b, j, p)
    n = k.numel()
    assert n >= 10 ** 5
    sd = math.sqrt(n * p * (1 - p))
    assert abs(int(k.sum()) - n * (1 - p)) <= 4 * sd
    # per tree and per column too: no row or column of the table is stuck
    assert float(k.float().mean(0).min()) > 1 - p - 0.15 and float(k.float().mean(1).min()) > 1 - p - 0.15


def test_the_keep_function_is_pure_and_differs_across_sites_and_seeds():
    b = torch.arange(64)[:, None]
    j = torch.arange(128)[None, :]
    base = T.keep(T.DROP_SEED, 2, b, j, 0.1)
    assert torch.equal(base, T.keep(T.DROP_SEED, 2, b, j, 0.1))
    for other in (T.keep(T.DROP_SEED, 3, b, j, 0.1), T.keep(T.DROP_SEED + 1, 2, b, j, 0.1),
                  T.keep(T.DROP_SEED ^ (1 << 40), 2, b, j, 0.1)):
        assert not torch.equal(base, other)
        agree = float((base == other).float().mean())
        assert abs(agree - (0.81 + 0.01)) < 0.03   # independent draws agree with probability 0.9^2 + 0.1^2
    assert bool(T.keep(T.DROP_SEED, 2, b, j, 0.0).all())
    assert T.drop_threshold(0.0) == 0 and T.drop_scale(0.0) == 1.0
    assert T.drop_threshold(0.5) == 2 ** 31 and T.drop_scale(0.5) == 2.0
    # the hash's words: a value worked out by hand from the formula in include/bgcn.h
    x = 1
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    assert int(T.mix32(torch.tensor(1))) == x
