"""-m gpu: csrc/gradclip.hip through brats21_amd.optim.clip_grad_norm_ / AGC against tests/golden/agc.npz (the reference's AGC
class, torch's clip_grad_norm_) and tests/_agc_ref.py, under the GradScaler pair, in a real training step and in a captured one.

Tolerance (derived, not measured): rtol 1e-5, atol 0 against the float64 value rounded to f32, on the clipped gradients and on
the total norm.  A unit's sum of squares is taken by 256 threads: each adds at most 81 squares in sequence (the largest unit of
the real network, 20,736 elements; 8,100 here -- with 16-byte loads four interleaved chains of a quarter of that), then an 8-level
tree: relative error of the sum <= ~89 * 2^-24 = 5e-6, of the norm half that; the sum across units is f64; the remaining
multiplies and the divide add ~3 ulp (2e-7)."""
import argparse
import contextlib
import io

import numpy as np
import pytest
import torch

import _agc_ref as R
from test_gradclip_cpu import load_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL = 1e-5

# the clipping of the graphed test: values at which both passes act on this model's first steps (the real-step test below
# prints the raw norm and the unit ratios); the test compares two runs of the same arithmetic, so nothing hinges on them
CLIPPING, MAX_NORM = 1e-2, 0.05


def device_case(golden_dir, name, scale=1.0):
    params, grads, max_norm, clipping, eps, ref, f64, z = load_case(golden_dir, name)
    ps = [torch.nn.Parameter(p.to(DEV)) for p in params]
    for p, g in zip(ps, grads):
        p.grad = None if g is None else (g * scale).to(DEV)
    return ps, params, max_norm, clipping, eps, f64, z


def run_case(ps, max_norm, clipping, eps, fused=False, **amp):
    """The reference's order: global clip, then AGC around SGD(lr=0) (the parameters stay, p.grad is the clipped gradient)."""
    from brats21_amd.optim import AGC, clip_grad_norm_, clip_grad_norm_agc_
    total = None
    if fused:
        return clip_grad_norm_agc_(ps, max_norm, clipping, eps, **amp)
    if max_norm is not None:
        total = clip_grad_norm_(ps, max_norm, **amp)
    if clipping is not None:
        agc = AGC(iter(ps), torch.optim.SGD(ps, lr=0.0), clipping=clipping, eps=eps)
        if amp:  # (torch's SGD does not take the pair: the clipping pass alone, as step() runs it)
            agc.clip_(**amp)
        else:
            agc.step()
    return total


def assert_close(got, want, what):
    got, want = got.detach().cpu().numpy(), want.numpy()
    err = float(np.max(np.abs(got.astype(np.float64) - want) / np.maximum(np.abs(want.astype(np.float64)), 1e-300)))
    print(f"{what}: worst relative error {err:.2e}")
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=0, err_msg=what)


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e", "e_fused"])
def test_golden_parity(golden_dir, name):
    fused, name = name.endswith("_fused"), name[0]
    ps, params, max_norm, clipping, eps, f64, z = device_case(golden_dir, name)
    twins = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    for q, p in zip(twins, ps):
        q.grad = None if p.grad is None else p.grad.clone()
    total = run_case(ps, max_norm, clipping, eps, fused=fused)
    torch.cuda.synchronize()
    for i, (p, cpu, want) in enumerate(zip(ps, params, f64)):
        assert torch.equal(p.detach().cpu(), cpu), i  # the parameters are read only
        if want is None:
            assert p.grad is None
        else:
            assert_close(p.grad, want, f"case {name} gradient {i} {tuple(cpu.shape)}")
    if max_norm is not None:
        assert total.shape == () and total.dtype == torch.float32 and total.is_cuda
        want = float(z[f"{name}__total_norm__f64"])
        print(f"case {name}: total norm {float(total):.9g} vs float64 {want:.9g}")
        assert abs(float(total) - want) <= RTOL * want
    if clipping is None:  # torch's own function on the same device
        t_total = torch.nn.utils.clip_grad_norm_(twins, max_norm)
        assert abs(float(total) - float(t_total)) <= RTOL * float(t_total)
        for i, (p, q) in enumerate(zip(ps, twins)):
            if q.grad is not None:
                np.testing.assert_allclose(p.grad.cpu().numpy(), q.grad.cpu().numpy(), rtol=RTOL, atol=0, err_msg=str(i))


@pytest.mark.parametrize("name,fused", [("a", False), ("c", False), ("e", False), ("e", True)])
def test_gradscaler_pair(golden_dir, name, fused):
    """Gradients that still carry the loss scale 2^10: the norms are the unscaled gradients', the result is -- bit for bit -- the
    unscaled run's times 2^10.  found_inf set: nothing is written."""
    ps, _, max_norm, clipping, eps, _, _ = device_case(golden_dir, name)
    run_case(ps, max_norm, clipping, eps, fused=fused)
    scaled, _, _, _, _, _, _ = device_case(golden_dir, name, scale=1024.0)
    scale = torch.full((1,), 1024.0, device=DEV)
    total = run_case(scaled, max_norm, clipping, eps, fused=fused, grad_scale=scale, found_inf=torch.zeros(1, device=DEV))
    changed = 0
    for p, q in zip(ps, scaled):
        if p.grad is not None:
            assert torch.equal(p.grad * 1024.0, q.grad)
    if max_norm is not None:
        plain, _, _, _, _, _, _ = device_case(golden_dir, name)
        assert float(run_case(plain, max_norm, clipping, eps, fused=fused)) == float(total)
    before = [None if p.grad is None else p.grad.clone() for p in scaled]
    run_case(scaled, 1e-3 if max_norm is not None else None, clipping, eps, fused=fused, grad_scale=scale,
             found_inf=torch.ones(1, device=DEV))
    for b, q in zip(before, scaled):
        if b is not None:
            assert torch.equal(b, q.grad)
            changed += 1
    assert changed == 10


def test_found_inf_reaches_the_wrapped_capturable_ranger(golden_dir):
    """GradScaler's skipped step through the wrapper: the AGC kernels write nothing, the wrapped Ranger2020(capturable=True) moves no
    parameter and does not advance its device-side step counter."""
    from brats21_amd.optim import AGC, Ranger2020
    ps, _, _, clipping, eps, _, _ = device_case(golden_dir, "a")
    ps = [p for p in ps if p.grad is not None]
    with contextlib.redirect_stdout(io.StringIO()):
        ranger = Ranger2020(ps, lr=1e-2, capturable=True)
    agc = AGC(ps, ranger, clipping=clipping, eps=eps)
    assert agc._step_supports_amp_scaling and agc.capturable
    agc.step()
    ranger.sync_steps()
    assert ranger.state[ps[0]]["step"] == 1
    params = [p.detach().clone() for p in ps]
    grads = [p.grad.clone() for p in ps]
    agc.grad_scale, agc.found_inf = torch.ones(1, device=DEV), torch.ones(1, device=DEV)
    agc.step()
    del agc.grad_scale, agc.found_inf
    assert not hasattr(ranger, "grad_scale") and not hasattr(ranger, "found_inf")
    ranger.sync_steps()
    assert ranger.state[ps[0]]["step"] == 1
    assert all(torch.equal(a, p.detach()) for a, p in zip(params, ps))
    assert all(torch.equal(a, p.grad) for a, p in zip(grads, ps))
    agc.step()  # and a clean step moves again
    ranger.sync_steps()
    assert ranger.state[ps[0]]["step"] == 2 and not torch.equal(params[0], ps[0].detach())


@pytest.mark.parametrize("name,fused", [("a", False), ("e", False), ("e", True)])
def test_two_runs_are_bit_identical(golden_dir, name, fused):
    runs = []
    for _ in range(2):
        ps, _, max_norm, clipping, eps, _, _ = device_case(golden_dir, name)
        total = run_case(ps, max_norm, clipping, eps, fused=fused)
        runs.append(([p.grad for p in ps if p.grad is not None], total))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0], runs[1][0]))
    if runs[0][1] is not None:
        assert torch.equal(runs[0][1], runs[1][1])


def test_non_contiguous_or_half_gradients_raise():
    from brats21_amd._lib import BratsHipError
    from brats21_amd.optim import clip_grad_norm_
    p = torch.nn.Parameter(torch.ones(4, 6, device=DEV))
    p.grad = torch.ones(6, 4, device=DEV).t()
    with pytest.raises(BratsHipError, match="contiguous f32"):
        clip_grad_norm_([p], 1.0)
    p.grad = None
    q = torch.nn.Parameter(torch.ones(4, 6, device=DEV, dtype=torch.float16))
    q.grad = torch.ones(4, 6, device=DEV, dtype=torch.float16)
    with pytest.raises(BratsHipError, match="contiguous f32"):
        clip_grad_norm_([q], 1.0)


def small_model():
    from brats21_amd import get_model
    ns = argparse.Namespace(model="equiunet", width=8, norm="group", act="relu", num_classes=3, dropout=0)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        return get_model(ns).to(DEV).train()


def test_agc_and_global_clip_in_a_real_step():
    """One eager TrainStep with AGC(m.parameters(), Ranger2020) and max_grad_norm: p.grad afterwards is tests/_agc_ref.py applied to
    the raw gradients (taken by the same forward / backward, which is deterministic) and the parameters before the step.
    max_norm is half the raw norm; clipping sits in the widest gap between the unit ratios grad_norm / param_norm near their
    median, so that about half of the units trigger and none of the decisions is a rounding tie -- asserted below."""
    from brats21_amd.engine import TrainStep
    from brats21_amd.optim import AGC, Ranger2020
    from oracle import synth
    x = synth.random_image(1, 4, (16, 16, 16), seed=20).to(DEV)
    t = synth.nested_spheres(1, (16, 16, 16)).to(DEV)
    m = small_model()
    params = list(m.parameters())
    with contextlib.redirect_stdout(io.StringIO()):
        opt = AGC(m.parameters(), Ranger2020(m.parameters(), lr=1e-2, weight_decay=1e-5, use_gc=True))
    step = TrainStep(m, opt, amp=True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        step.loss(m(x), t).backward()
    raw = [p.grad.clone() for p in params]
    before = [p.detach().clone() for p in params]
    eps = 1e-3
    _, total, _, _, _ = R.clip_then_agc(before, raw, max_norm=1.0)
    max_norm = 0.5 * float(total)
    clipped, _, _ = R.global_clip(raw, max_norm)
    ratios = torch.cat([(R.unitwise_norm(g) / torch.clamp(R.unitwise_norm(p.double()), min=eps)).reshape(-1)
                        for p, g in zip(before, clipped)]).sort().values
    mid = ratios[int(0.4 * len(ratios)):int(0.6 * len(ratios)) + 1]
    k = int(torch.argmax(mid[1:] / mid[:-1]))
    clipping = float(torch.sqrt(mid[k] * mid[k + 1]))
    want, _, coef, trig, ratio = R.clip_then_agc(before, raw, max_norm, clipping, eps)
    trig, ratio = torch.cat(trig), torch.cat(ratio)
    frac = float(trig.double().mean())
    print(f"raw norm {float(total):.4g}, units {trig.numel()}, triggered {frac:.2f}, clip_coef {float(coef):.4f}, clipping {clipping:.3e}, "
          f"closest decision {float((ratio - 1).abs().min()):.2e}")
    assert 0.1 <= frac <= 0.9 and float(coef) < 1 and float((ratio - 1).abs().min()) > 1e-4
    opt.clipping, step.max_grad_norm = clipping, max_norm
    step(x, t)
    torch.cuda.synchronize()
    assert not torch.equal(before[0], params[0].detach())  # the wrapped optimizer stepped
    for i, (p, w) in enumerate(zip(params, want)):
        assert_close(p.grad, w.float().cpu(), f"gradient {i} {tuple(p.shape)}")


@pytest.mark.parametrize("amp_dtype", [torch.bfloat16, torch.float16])
def test_graphed_step_with_clipping_matches_eager(amp_dtype):
    """tests/test_optim_gpu.py::test_graphed_train_step_matches_eager with AGC around the optimizer and max_grad_norm: the two
    clipping calls are captured with the step (float16: together with GradScaler's unscale_ and the device-side skip), same
    schedule, same bounds."""
    from brats21_amd.engine import GraphedTrainStep, TrainStep
    from brats21_amd.optim import AGC, Ranger2020
    from oracle import synth
    xs = [synth.random_image(1, 4, (16, 16, 16), seed=20 + i).to(DEV) for i in range(8)]
    t = synth.nested_spheres(1, (16, 16, 16)).to(DEV)
    results = []
    for graphed in (False, True):
        m = small_model()
        with contextlib.redirect_stdout(io.StringIO()):
            ranger = Ranger2020(m.parameters(), lr=1e-2, weight_decay=1e-5, use_gc=True, capturable=graphed)
        opt = AGC(m.parameters(), ranger, clipping=CLIPPING)
        step = TrainStep(m, opt, amp=True, amp_dtype=amp_dtype, max_grad_norm=MAX_NORM)
        losses = []
        if graphed:
            step = GraphedTrainStep(step, warmup=2)
            losses.append(float(step(xs[0], t).detach()))  # 2 eager warm-ups + capture + 1 replay = steps 1..3 on xs[0]
            for x in xs[1:]:
                losses.append(float(step(x, t).detach()))
        else:
            for i, x in enumerate([xs[0], xs[0], xs[0]] + xs[1:]):
                l = float(step(x, t).detach())
                if i >= 2:
                    losses.append(l)
        torch.cuda.synchronize()
        results.append((losses, [p.detach().clone() for p in m.parameters()], opt))
    (l0, p0, o0), (l1, p1, o1) = results
    assert len(l0) == len(l1) == 8
    np.testing.assert_allclose(l0, l1, rtol=1e-5, atol=1e-6)
    worst = max(float((a - b).abs().max()) for a, b in zip(p0, p1))
    assert worst < 1e-5, worst
    assert o1.state_dict()["state"][0]["step"] == 10 == o0.state_dict()["state"][0]["step"]

