"""GPU tests of the multi-label criteria losses.DiceCELoss, DiceFocalLoss, FocalLoss and TverskyLoss (csrc/sigmoid_loss.hip:
brats_sigmoid_target_prepare, brats_sigmoid_loss_stats, brats_sigmoid_loss_grad) against the float64 restatement
tests/_sigmoid_losses_ref.py.

Bar: the rule of tests/test_softmax_loss_gpu.py.  For each case the restatement is also evaluated in float32 on the CPU; the GPU
may be at most 4 x that error away from float64, and the bar is not set below 1e-6 relative.  It is applied to the loss value
(relative) and to each head's gradient (max abs error over max abs gradient).  The measured errors are printed (pytest -s) and
carried in the assertion messages."""
import argparse
import contextlib
import io

import numpy as np
import pytest
import torch

import _sigmoid_losses_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"

# criterion -> (class, what src/definer.py:204-245 passes)
CRITERIA = {
    "dice_ce": ("DiceCELoss", dict(include_background=True, sigmoid=True, softmax=False, squared_pred=True, batch=True, reduction="mean")),
    "dice_focal": ("DiceFocalLoss", dict(include_background=True, sigmoid=True, softmax=False, squared_pred=True, batch=False, reduction="mean")),
    "focal": ("FocalLoss", dict(gamma=2.0, reduction="mean")),
    "tversky": ("TverskyLoss", dict(include_background=True, sigmoid=True, softmax=False, alpha=0.5, beta=0.5, reduction="mean")),
}
SHAPES = ((1, 1, 65),      # a single partial, scalar tail
          (16, 16, 36),    # 16-byte path, several workgroups
          (9, 37, 70),     # V % 4 != 0: scalar path, several workgroups, ragged end
          "misaligned")    # (8, 12, 20) on a view one float into its allocation: V % 4 == 0 but no plane is 16-byte aligned
# the last two binary kinds are where the smoothing terms decide a Dice / Tversky value; "soft" takes the focal kernels' branch
# for a target that is neither 0 nor 1
TARGET_KINDS = ("random", "nested", "empty_channel", "full_sample", "soft")


def make_criterion(name, **options):
    from brats21_amd import losses
    cls, kwargs = CRITERIA[name]
    return getattr(losses, cls)(**{**kwargs, **options})


def make_logits(n, k, shape, g, stress=False):
    x = torch.randn((n, k) + shape, generator=g) * 3.0
    if stress:  # +-100 at the same voxels: exp() of the raw logits overflows, the result must be finite and right
        sel = torch.rand(shape, generator=g) < 0.2
        x[:, 0][:, sel] = 100.0
        x[:, k - 1][:, sel] = -100.0  # (K = 1: the one channel is -100 there ...)
        sel2 = torch.rand(shape, generator=g) < 0.05
        x[:, k - 1][:, sel2] = -100.0
        x[:, 0][:, sel2] = 100.0 if k <= 2 else 99.0  # (... and +100 here)
    return x


def make_target(kind, n, k, shape, g):
    if kind == "soft":
        return torch.rand((n, k) + shape, generator=g)
    if kind == "nested":  # the BraTS channels: every channel contains the one before it
        r = torch.rand((n, 1) + shape, generator=g)
        return (r < torch.arange(1, k + 1).view(1, k, 1, 1, 1) / (k + 1.0)).float()
    t = (torch.rand((n, k) + shape, generator=g) < 0.4).float()
    if kind == "empty_channel":  # one channel empty over the whole batch
        t[:, k - 1] = 0.0
    elif kind == "full_sample":  # one sample all foreground
        t[n - 1] = 1.0
    return t


def on_device(x, misaligned=False):
    """the tensor on the GPU; misaligned: a contiguous view that starts one float into its allocation"""
    if not misaligned:
        return x.to(DEV)
    buf = torch.empty(x.numel() + 1, dtype=torch.float32, device=DEV)
    view = buf[1:].view(x.shape)
    view.copy_(x)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def run_gpu(criterion, heads, target, prepared=True, misaligned=False):
    from brats21_amd import losses
    xs = [on_device(h, misaligned).requires_grad_(True) for h in heads]
    t = on_device(target, misaligned)
    if len(xs) == 1:
        loss = criterion(xs[0], t)
    else:
        fn = losses.deep_supervision_prepared_loss if prepared else losses.deep_supervision_loss
        loss, main = fn(criterion, (xs[0], xs[1:]), t)
        assert main is xs[0]
    loss.backward()
    return loss.detach(), [x.grad for x in xs]


def check_case(name, what, heads, target, misaligned=False, **options):
    f64, g64 = R.deep_loss_and_grads(name, heads, target, torch.float64, **options)
    f32, g32 = R.deep_loss_and_grads(name, heads, target, torch.float32, **options)
    loss, grads = run_gpu(make_criterion(name, **options), heads, target, misaligned=misaligned)
    assert np.isfinite(f64) and bool(torch.isfinite(loss)) and loss.dtype == torch.float32
    ref_err = abs(f32 - f64) / abs(f64)
    bar = max(4.0 * ref_err, 1e-6)
    err = abs(float(loss.double()) - f64) / abs(f64)
    lines = [f"{name} {what}: value {float(loss):.8f} vs float64 {f64:.10f}: rel err {err:.2e} (bar {bar:.2e}, float32 CPU {ref_err:.2e})"]
    ok = err <= bar
    for i, (g, w64, w32) in enumerate(zip(grads, g64, g32)):
        assert g.dtype == torch.float32 and g.shape == w64.shape and bool(torch.isfinite(g).all())
        scale = float(w64.abs().max())
        ref_g = float((w32.double() - w64).abs().max()) / scale
        gbar = max(4.0 * ref_g, 1e-6)
        gerr = float((g.cpu().double() - w64).abs().max()) / scale
        lines.append(f"   head {i}: gradient max err / max {gerr:.2e} (bar {gbar:.2e}, float32 CPU {ref_g:.2e})")
        ok = ok and gerr <= gbar
    print("\n" + "\n".join(lines))
    assert ok, lines


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("k", [1, 3, 5, 16])
@pytest.mark.parametrize("name", list(CRITERIA))
def test_value_and_gradient_match_float64(name, k, n):
    g = torch.Generator().manual_seed(1000 * k + n)
    for shape in SHAPES:
        mis = shape == "misaligned"
        sp = (8, 12, 20) if mis else shape
        for kind in TARGET_KINDS:
            check_case(name, f"K={k} N={n} {shape} target {kind}", [make_logits(n, k, sp, g)], make_target(kind, n, k, sp, g), misaligned=mis)
        check_case(name, f"K={k} N={n} {shape} +-100 logits", [make_logits(n, k, sp, g, stress=True)], make_target("random", n, k, sp, g),
                   misaligned=mis)


WEIGHTS = dict(smooth_nr=1e-3, smooth_dr=1e-4)
OPTIONS = ([("dice_ce", dict(jaccard=j, batch=b, **(dict(lambda_dice=0.7, lambda_ce=1.3, **WEIGHTS) if j != b else {})))
            for j in (False, True) for b in (False, True)]
           + [("dice_focal", dict(jaccard=j, batch=b, gamma=gamma, **(dict(lambda_dice=0.7, lambda_focal=1.3, **WEIGHTS) if j != b else {})))
              for j in (False, True) for b in (False, True) for gamma in (0.0, 2.0, 3.5)]
           + [("focal", dict(gamma=gamma)) for gamma in (0.0, 2.0, 3.5)]
           + [("tversky", dict(alpha=a, beta=b, batch=batch, **(WEIGHTS if batch else {}))) for a, b in ((0.5, 0.5), (0.3, 0.7)) for batch in (False, True)])


@pytest.mark.parametrize("name,options", OPTIONS, ids=[f"{n}-" + "-".join(f"{k}={v}" for k, v in o.items()) for n, o in OPTIONS])
def test_options_on_two_heads(name, options):
    g = torch.Generator().manual_seed(77)
    n, k, shape = 3, 3, (9, 37, 70)
    heads = [make_logits(n, k, shape, g), make_logits(n, k, shape, g, stress=True)]
    for kind in ("nested", "empty_channel", "soft"):
        check_case(name, f"{options} target {kind}", heads, make_target(kind, n, k, shape, g), **options)


def _three_heads():
    g = torch.Generator().manual_seed(5)
    n, k, shape = 2, 5, (9, 37, 70)
    return [make_logits(n, k, shape, g) for _ in range(3)], make_target("nested", n, k, shape, g)


@pytest.mark.parametrize("name", list(CRITERIA))
def test_prepared_target_is_bit_equal_runs_once_and_runs_are_deterministic(name):
    from brats21_amd import losses
    heads, target = _three_heads()
    crit = make_criterion(name)
    calls = []
    prepare = crit.prepare
    crit.prepare = lambda t: calls.append(1) or prepare(t)
    la, ga = run_gpu(crit, heads, target, prepared=True)
    assert len(calls) == 1  # one pass over the target for the three heads
    lb, gb = run_gpu(crit, heads, target, prepared=False)
    assert len(calls) == 1 + 3  # the reference's form: once per head
    assert torch.equal(la, lb) and all(torch.equal(a, b) for a, b in zip(ga, gb))
    la2, ga2 = run_gpu(crit, heads, target, prepared=True)  # no float atomics anywhere: bit-reproducible
    assert torch.equal(la, la2) and all(torch.equal(a, b) for a, b in zip(ga, ga2))
    prep = prepare(target.to(DEV))
    assert isinstance(prep, losses.PreparedTarget)
    want = torch.stack([target.double().sum((2, 3, 4)), (target.double() ** 2).sum((2, 3, 4))], -1)
    torch.testing.assert_close(prep.tsums.cpu().double(), want, rtol=1e-6, atol=0)
    if name == "dice_ce":
        assert prep.classmap.dtype == torch.uint8 and torch.equal(prep.classmap.cpu().long(), R.class_map(target))
    else:
        assert prep.classmap is None  # only the CE term reads a class map
    with pytest.raises(ValueError):
        make_criterion(name)(heads[0].to(DEV), prep)  # made by another criterion


def test_class_map_of_the_eight_brats_channel_patterns():
    """ties go to the lowest channel: 000 and 111 are both class 0 (the wide and the scalar kernel)"""
    patterns = torch.tensor([[a, b, c] for a in (0, 1) for b in (0, 1) for c in (0, 1)], dtype=torch.float32)
    for reps in (16, 3):  # 128 and 24 voxels
        t = patterns.repeat(reps, 1).t().reshape(1, 3, 1, reps, 8).contiguous()
        for mis in (False, True):  # the 16-byte form; one float into the allocation: the scalar form
            prep = make_criterion("dice_ce").prepare(on_device(t, mis))
            assert torch.equal(prep.classmap.cpu().long(), R.class_map(t)), (reps, mis)
            assert prep.classmap.flatten()[:8].tolist() == [0, 2, 1, 1, 0, 0, 0, 0]


def test_other_logit_dtypes_are_upcast():
    heads, target = _three_heads()
    for name in CRITERIA:
        crit = make_criterion(name)
        xb = heads[0].to(DEV).bfloat16().requires_grad_(True)
        lb = crit(xb, target.to(DEV))
        lb.backward()
        xf = xb.detach().float().requires_grad_(True)
        lf = crit(xf, target.to(DEV).bool())  # and a target of another dtype
        lf.backward()
        assert xb.grad.dtype == torch.bfloat16 and torch.equal(lb, lf) and torch.equal(xb.grad, xf.grad.bfloat16()), name


@pytest.mark.parametrize("name", list(CRITERIA))
def test_graphed_train_step_replays_the_eager_losses(name):
    """A width-8 EquiUnet step at 1 x 4 x 16^3 with the criterion: three eager steps and three replays of the step captured into
    one hipGraph, from the same initial state and with the same (capturable) optimizer, give bit-equal losses and finite
    gradients -- the capture itself shows that no pass of the criterion synchronises with the host."""
    from brats21_amd import get_model
    from brats21_amd.engine import GraphedTrainStep, TrainStep
    from brats21_amd.optim import Ranger2020
    from oracle import synth
    ns = argparse.Namespace(model="equiunet", width=8, norm="group", act="relu", num_classes=3, dropout=0)
    size = (16, 16, 16)
    xs = [synth.random_image(1, 4, size, seed=40 + i).to(DEV) for i in range(3)]
    ts = [synth.nested_spheres(1, size).to(DEV).roll(i, dims=-1) for i in range(3)]  # a new target every step
    results = []
    for graphed in (False, True):
        torch.manual_seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            m = get_model(ns).to(DEV).train()
        opt = Ranger2020(m.parameters(), lr=1e-3, weight_decay=1e-5, use_gc=True, capturable=True)
        step = TrainStep(m, opt, criterion=make_criterion(name), amp=True)
        if graphed:
            step = GraphedTrainStep(step, warmup=2)  # the first call: two eager warm-up steps on batch 0, the capture, one replay
            got = [float(step(x, t).detach()) for x, t in zip(xs, ts)]
        else:
            got = [float(step(x, t).detach()) for x, t in zip([xs[0]] * 2 + xs, [ts[0]] * 2 + ts)][2:]
        torch.cuda.synchronize()
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
        results.append(got)
    print(f"  {name}: eager {results[0]} graphed {results[1]}")
    assert len(results[1]) == 3 and all(np.isfinite(results[1]))
    assert len(set(results[0])) == 3  # the three steps differ: a replay that baked one target in would not follow them
    assert results[0] == results[1]
