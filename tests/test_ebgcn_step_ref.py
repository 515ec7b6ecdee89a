"""CPU check that the bars of tests/test_gpu_ebgcn_step.py's trajectory test are about the code, not about
fp32: the reference trajectory (tests/ebgcn_step_ref.py) run in fp32 stays inside max-scaled 1e-4 of its
fp64 run for the loss, every gradient and every parameter after each of the three updates, on the model
fixture with the noise of ebgcn_step_ref.NOISE_SEED - and that this noise, unlike the fixture's own, keeps every
sign decision on the gradient's way resolvable in fp32 (ebgcn_step_ref.sign_margins)."""
import functools

import pytest
import torch

import ebgcn_step_ref as R
import ebgcn_train_ref as T

TOL = 1e-4


@functools.lru_cache(maxsize=None)
def _runs(td, bu):
    z = T.load_npz(R.MODEL_FIXTURE)
    steps = 3 if td and bu else 1
    return R.trajectory(z, torch.float64, steps, td, bu), R.trajectory(z, torch.float32, steps, td, bu)


@pytest.mark.parametrize("td,bu", [(True, True), (True, False), (False, True)])
def test_fp32_arithmetic_alone_stays_inside_the_bars(td, bu):
    (want, none64), (got, none32) = _runs(td, bu)
    assert none64 == none32 and len(none64) == 21 * (int(td) + int(bu)) + 27 * (2 - int(td) - int(bu))
    worst = 0.0
    zero = {f"d {d}.conv1.bias": f"{d}.conv1.lin.weight"
            for d, on in (("TDrumorGCN", td), ("BUrumorGCN", bu)) if not on}
    for t, (a, b) in enumerate(zip(got, want)):
        assert a["correct"] == b["correct"]
        pairs = [("loss", a["loss"], b["loss"])]
        pairs += [(f"d {k}", a["grads"][k], g) for k, g in b["grads"].items() if g is not None]
        pairs += [(k, a["params"][k], p) for k, p in b["params"].items()]
        for what, x, y in pairs:
            err, scale = float((x.double() - y).abs().max()), float(y.abs().max())
            if what in zero:   # zero in exact arithmetic (see tests/test_gpu_ebgcn_step.py): its conv's weight gradient's scale
                assert scale <= 1e-12 * float(b["grads"][zero[what]].abs().max()), (what, scale)
                scale = float(b["grads"][zero[what]].abs().max())
            worst = max(worst, err / max(scale, 1e-300))
            assert err <= TOL * scale, (t, what, err, scale)
    print(f"fp32 vs fp64 over {len(want)} steps: worst max-scaled error {worst:.3e}")


def test_the_noise_seed_keeps_every_sign_decision_resolvable_in_fp32():
    z = T.load_npz(R.MODEL_FIXTURE)
    for td, bu, steps in ((True, True, 3), (True, False, 1), (False, True, 1)):
        want, _ = R.trajectory(z, torch.float64, steps, td, bu, margins=True)
        for t, s in enumerate(want):
            print(td, bu, t, {k: f"{v:.1e}" for k, v in s["margins"].items()})
            assert min(s["margins"].values()) >= R.TIE_WINDOW, (td, bu, t, s["margins"])
    # why not the fixture's own draw: its third step has a LeakyReLU argument at ~1e-9 of the largest
    own, _ = R.trajectory(z, torch.float64, 3, seed=None, margins=True)
    assert min(own[0]["margins"].values()) >= R.TIE_WINDOW and min(own[1]["margins"].values()) >= R.TIE_WINDOW
    assert own[2]["margins"]["TDrumorGCN LeakyReLU"] < 1e-8 < R.TIE_WINDOW


def test_the_untouched_parameters_are_the_ones_without_a_gradient():
    (want, none), _ = _runs(True, True)
    z = T.load_npz(R.MODEL_FIXTURE)
    sd = T.group(z, "sd")
    for k in none:   # torch.optim.Adam leaves a parameter whose grad is None alone: no weight decay either
        assert torch.equal(want[-1]["params"][k], sd[k].double()), k
    moved = [k for k in want[-1]["params"] if k not in none]
    assert len(moved) == 68 - 42
    for k in moved:
        assert not torch.equal(want[-1]["params"][k], sd[k].double()), k
