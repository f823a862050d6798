"""-m gpu: EquiUnet's refinement stage (``--model equiunet_ref``, networks/equiunet.py: RefUnet, _ref_fwd / _ref_bwd) against the
reference's own class (tests/golden/refine_*.npz, made by tests/golden/make_golden_refine.py) and against tests/_refine_ref.py
in float64.

Bars of the f32 mode: those of tests/test_general_channels_gpu.py::test_f32_matches_reference_golden -- logits and deep heads 1e-3,
loss 1e-4, gradient norms rtol 2e-3, small gradients 2e-3 of their maximum -- on both heads.  The reference's own f32 error
against float64 is recorded in the fixtures (ref_err_*).  The encoder's gradients are in the norm list: they see the whole
gradient of the unrefined logits (through the residual, from the loss on that head, and through the stage's first convolution)."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

import _general_cases as G
import _refine_ref as R
from oracle import synth, unet

pytestmark = pytest.mark.gpu
LOGIT_ATOL = 1e-3


@pytest.fixture(autouse=True)
def _release():
    yield
    torch.cuda.empty_cache()


def _golden(golden_dir, case):
    return np.load(os.path.join(golden_dir, R.fname(case)), allow_pickle=False)


def _check_grads(params, names, ref_norms, small):
    norms = np.array([float(params[n].grad.double().norm()) for n in names])
    print(f"  gradient norms: worst relative deviation {np.abs(norms / ref_norms - 1).max():.2e} "
          f"({names[int(np.abs(norms / ref_norms - 1).argmax())]})")
    worst = max(float(np.abs(params[k].grad.cpu().numpy() - ref).max() / max(np.abs(ref).max(), 1e-6)) for k, ref in small.items())
    print(f"  small gradients: worst max abs deviation / max {worst:.2e}")
    np.testing.assert_allclose(norms, ref_norms, rtol=2e-3, atol=1e-7)
    for k, ref in small.items():
        np.testing.assert_allclose(params[k].grad.cpu().numpy(), ref, atol=2e-3 * max(np.abs(ref).max(), 1e-6), rtol=2e-3, err_msg=k)


@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_f32_matches_reference_golden(golden_dir, case):
    g = _golden(golden_dir, case)
    meta = json.loads(str(g["meta"]))
    m = R.build(case).cuda().train()
    x, t = R.image().cuda(), synth.nested_spheres(1, R.SIZE).cuda()
    (refined, out), deeps = m(x)
    assert refined.shape == out.shape == (1, 3, *R.SIZE) and len(deeps) == 4 and all(d.shape == out.shape for d in deeps)
    e_ref = np.abs(refined.detach().cpu().numpy() - g["refined"]).max()
    e_out = np.abs(out.detach().cpu().numpy()[:, :, ::meta["out_z_stride"]] - g["out"]).max()
    print(f"  {R.fname(case)}: max abs err refined {e_ref:.2e} out {e_out:.2e} (the reference's own against f64: "
          f"{float(g['ref_err_refined']):.2e}, {float(g['ref_err_out']):.2e})")
    assert e_ref < LOGIT_ATOL and e_out < LOGIT_ATOL
    for i, d in enumerate(deeps):
        e = np.abs(d.detach().cpu().numpy()[:, :, ::2, ::2, ::2] - g[f"deep{i}"]).max()
        assert e < LOGIT_ATOL, f"deep head {i} max abs err {e}"
    loss = R.ds_loss(([refined, out], deeps), t)
    print(f"  loss {loss.item():.7f} golden {float(g['loss']):.7f}")
    assert abs(loss.item() - float(g["loss"])) < 1e-4
    loss.backward()
    params = dict(m.named_parameters())
    assert params["refunet.conv0.weight"].grad.shape == (R.WIDTH, 3, 3, 3, 3), "num_classes input columns"
    assert params["refunet.conv_d0.weight"].grad.shape == (3, R.WIDTH, 3, 3, 3), "num_classes rows"
    names = json.loads(str(g["grad_names"]))
    assert set(names) == set(params) and names[0].startswith("encoder1")
    _check_grads(params, names, g["grad_norms"], {k[5:]: g[k] for k in g.files if k.startswith("grad:")})


@pytest.mark.parametrize("inplanes,num_classes,image", [(4, 3, "random"), (1, 5, "closed")], ids=["c4_k3", "c1_k5"])
def test_non_cubic_batch_matches_float64(inplanes, num_classes, image):
    """2 x C x 32 x 48 x 64 at width 8 in f32 mode against tests/_refine_ref.py on the CPU in float64, at the same bars.

    Weights: the constructor's own initialisation under torch.manual_seed(0) (kaiming-normal convolutions, the two end
    convolutions included), copied into the restatement through the state dict.  Weights and input of each case are the pair with
    the smallest error of the REFERENCE ARITHMETIC itself -- torch's f32 evaluation of tests/_refine_ref.py against its f64 one,
    on the CPU, (gradient norms, small gradients) against the bars (2e-3, 2e-3):
        weights / image               (4, 3)               (1, 5)
        closed-form / random_image    9.6e-4, 1.7e-3       1.7e-3, 1.9e-3
        closed-form / closed_form     6.2e-3, 1.1e-2       8.3e-4, 1.7e-3
        seeded init / random_image    5.7e-4, 1.7e-3  <-   2.1e-4, 4.7e-4
        seeded init / closed_form     6.5e-4, 2.4e-3       1.8e-5, 1.4e-4  <-
    (on this volume the closed-form weights of the fixtures leave any f32 arithmetic little or no room under the gradient bars)."""
    size = (32, 48, 64)
    torch.manual_seed(0)
    m = R.build(inplanes=inplanes, num_classes=num_classes, load=False).cuda().train()
    x = synth.random_image(2, inplanes, size, seed=70 + inplanes) if image == "random" else synth.closed_form_image(2, inplanes, size)
    t = G.nested_targets(2, num_classes, size)
    (refined, out), deeps = m(x.cuda())
    R.ds_loss(([refined, out], deeps), t.cuda()).backward()
    sd64 = {k: (v.detach().cpu().double().requires_grad_(True) if v.is_floating_point() else v.cpu()) for k, v in m.state_dict().items()}
    assert list(sd64) == list(R.state_shapes(R.WIDTH, inplanes, num_classes))
    res = R.forward(sd64, x.double())
    loss64 = R.ds_loss(res, t.double())
    loss64.backward()
    heads64 = R.flat(res)
    for name, got, want in zip(("refined", "out", "deep0", "deep1", "deep2", "deep3"), [refined, out] + list(deeps), heads64):
        e = float((got.detach().cpu().double() - want.detach()).abs().max())
        print(f"  {name}: max abs err {e:.2e}")
        assert e < LOGIT_ATOL, name
    loss = R.ds_loss(([refined, out], deeps), t.cuda())
    print(f"  loss {loss.item():.7f} float64 {float(loss64):.7f}")
    assert abs(loss.item() - float(loss64)) < 1e-4
    params = dict(m.named_parameters())
    assert params["refunet.conv0.weight"].grad.shape[1] == num_classes and params["refunet.conv_d0.weight"].grad.shape[0] == num_classes
    names = list(params)
    ref_norms = np.array([float(sd64[n].grad.norm()) for n in names])
    _check_grads(params, names, ref_norms, {n: sd64[n].grad.float().numpy() for n in names if sd64[n].numel() <= 2048})


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_16bit_stage_adds_what_the_reference_adds(golden_dir, precision):
    """r = mean |refined - golden| / mean |out - golden| in a 16-bit mode, on the fixture's weights, is at most twice the same
    ratio of the reference under bf16 autocast (ref_bf16_ratio of the fixture).  The `out` head is the parent's code path, not code
    under test; the factor 2 allows for different rounding points."""
    case = R.CASES[0]
    g = _golden(golden_dir, case)
    zs = json.loads(str(g["meta"]))["out_z_stride"]
    m = R.build(case).cuda().eval()
    m.precision = precision
    with torch.no_grad():
        (refined, out), _ = m(R.image().cuda())
    e_ref = float((refined.cpu() - torch.from_numpy(g["refined"])).abs().mean())
    e_out = float((out.cpu()[:, :, ::zs] - torch.from_numpy(g["out"])).abs().mean())
    r = e_ref / e_out
    print(f"  {precision}: mean |refined - golden| {e_ref:.4e}, mean |out - golden| {e_out:.4e}, r = {r:.3f}; "
          f"the reference under bf16 autocast: {float(g['ref_bf16_ratio']):.3f}")
    assert r <= 2.0 * float(g["ref_bf16_ratio"])


def _train_run(graphed, steps=3, dropout=0):
    """_train_run of tests/test_general_channels_gpu.py for the network with the stage: `steps` recorded steps of TrainStep (bf16
    autocast, fused Dice, Ranger2020) on a batch of two after two unrecorded ones -> (losses, parameters)"""
    from brats21_amd.engine import GraphedTrainStep, TrainStep
    from brats21_amd.optim import Ranger2020
    dev = torch.device("cuda")
    x = synth.random_image(2, 4, R.SIZE, seed=44).to(dev)
    t = synth.nested_spheres(2, R.SIZE).to(dev)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        m = R.build(load=False, dropout=dropout)
    m.precision = "auto"
    m = m.to(dev).train()
    opt = Ranger2020(m.parameters(), lr=1e-2, weight_decay=1e-5, use_gc=True, capturable=graphed)
    step = TrainStep(m, opt, amp=True)
    losses = []
    if graphed:
        step = GraphedTrainStep(step, warmup=2)
        for _ in range(steps):  # (the first call: two eager warm-ups, the capture, one replay)
            losses.append(step(x, t).detach().clone())
    else:
        for i in range(2 + steps):
            loss = step(x, t).detach().clone()
            if i >= 2:
                losses.append(loss)
    torch.cuda.synchronize()
    return torch.stack(losses).cpu(), [p.detach().clone() for p in m.parameters()]


def test_training_steps_eager_and_graphed_are_bit_identical():
    l0, p0 = _train_run(False)
    lg, pg = _train_run(True)
    print(f"  eager {l0.tolist()} graphed {lg.tolist()}")
    assert bool(torch.isfinite(l0).all()) and l0[-1] < l0[0]
    assert torch.equal(l0, lg), (l0, lg)
    assert all(torch.equal(a, b) for a, b in zip(p0, pg)), "the replayed steps end at other weights than the eager ones"


def test_fused_six_head_dice_equals_the_criterion():
    """fused_deep_supervision_dice on ([refined, out], deeps) = deep_supervision_loss(DiceLoss()) over the six heads (value: the
    bar of the loss sequences in tests/test_general_channels_gpu.py, rtol 1e-5 / atol 1e-6; gradients of both heads alike) and
    returns the refined head as the output."""
    from brats21_amd.losses import DiceLoss, deep_supervision_loss, fused_deep_supervision_dice
    g = torch.Generator(device="cuda").manual_seed(5)
    heads = [torch.randn((2, 3, 16, 16, 16), device="cuda", generator=g, requires_grad=True) for _ in range(6)]
    t = synth.nested_spheres(2, (16, 16, 16)).cuda()
    nested = ([heads[0], heads[1]], heads[2:])
    fused = fused_deep_supervision_dice(nested, t)
    plain, first = deep_supervision_loss(DiceLoss(), nested, t)
    assert first is heads[0]
    np.testing.assert_allclose(fused.item(), plain.item(), rtol=1e-5, atol=1e-6)
    gf = torch.autograd.grad(fused, heads)
    gp = torch.autograd.grad(plain, heads)
    for a, b in zip(gf, gp):
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()) + 1e-12


def test_dropout_trains_one_step():
    losses, params = _train_run(False, steps=1, dropout=0.1)
    assert bool(torch.isfinite(losses).all()) and all(bool(torch.isfinite(p).all()) for p in params)


def test_sliding_window_returns_the_refined_head():
    """A 32 x 32 x 48 volume, 32^3 window, overlap 0.5, constant blend, f32: against the refined head of the same model run window
    by window and averaged in torch."""
    from brats21_amd.inferers import _first, sliding_window_inference
    m = R.build(deep_supervision=False).cuda().eval()
    x = synth.closed_form_image(1, 4, (32, 32, 48)).cuda()
    with torch.no_grad():
        got = sliding_window_inference(x, (32, 32, 32), 1, m, overlap=0.5, mode="constant")
        acc = torch.zeros((1, 3, 32, 32, 48), device=x.device)
        cnt = torch.zeros_like(acc)
        for x0 in (0, 16):
            res = m(x[..., x0:x0 + 32].contiguous())
            assert isinstance(res, list) and len(res) == 2 and _first(res) is res[0]
            assert float((res[0] - res[1]).abs().max()) > 1e-3, "the refined head is not the unrefined one"
            acc[..., x0:x0 + 32] += res[0]
            cnt[..., x0:x0 + 32] += 1.0
    want = acc / cnt
    assert got.shape == want.shape and bool(torch.isfinite(got).all())
    tol = 1e-6 * float(want.abs().max())
    err = float((got - want).abs().max())
    print(f"  sliding window: max |got - want| {err:.2e} / {tol:.2e}")
    assert err <= tol


def test_refused_configurations():
    m = R.build().cuda().train()
    with pytest.raises(ValueError, match="divisible by 16"):
        m(torch.zeros(1, 4, 24, 24, 24, device="cuda"))
    m.conv_fp8 = "fwd"
    with pytest.raises(NotImplementedError):
        m(torch.zeros(1, 4, 32, 32, 32, device="cuda"))


def test_get_model_trains_and_infers():
    """definer.get_model(model="equiunet_ref"): one step through TrainStep, then sliding-window inference with the same module."""
    from brats21_amd import get_model
    from brats21_amd.engine import TrainStep
    from brats21_amd.inferers import sliding_window_inference
    from brats21_amd.optim import Ranger2020
    with contextlib.redirect_stdout(io.StringIO()):
        m = get_model(G.namespace(model="equiunet_ref")).cuda().train()
    x, t = synth.random_image(1, 4, R.SIZE, seed=3).cuda(), synth.nested_spheres(1, R.SIZE).cuda()
    loss = TrainStep(m, Ranger2020(m.parameters(), lr=1e-3), amp=True)(x, t)
    assert bool(torch.isfinite(loss))
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
    m.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        y = sliding_window_inference(x, R.SIZE, 1, m, overlap=0.5)
    assert y.shape == (1, 3, *R.SIZE) and bool(torch.isfinite(y).all())
