"""-m gpu: brats21_amd.networks.Unet (``--model modified_unet``) against the reference's own class (tests/golden/unet_w8_*.npz, made
by tests/golden/make_golden_unet.py) and against tests/_unet_ref.py in float64.

Bars of the f32 mode: those of tests/test_refine_gpu.py / tests/test_att_gpu.py -- heads 1e-3 abs, loss 1e-4, gradient norms rtol 2e-3,
small gradients 2e-3 of their maximum.  The reference's own f32 error against float64 is recorded in the fixtures (ref_err_*).

A convolution bias in front of a per-channel normalisation (every unit under ``instance``; the 8-wide units under ``group``, whose 8
groups hold one channel each) has a gradient that is zero in exact arithmetic: sum_v dy = 0.  What arithmetic leaves of it is the
rounding of that channel sum, and it is bounded ABSOLUTELY, by the same 2e-3 of a maximum -- the maximum of the gradient of the
unit's norm shift, which is the channel sum of the unit's OUTPUT gradient over the same voxels (the reference's own f32 leaves
3e-8 where those maxima are 1e-4 .. 1e-2)."""
import contextlib
import io

import numpy as np
import pytest
import torch

import _unet_ref as R
from oracle import synth

pytestmark = pytest.mark.gpu
HEAD_ATOL = 1e-3
CONV_BIAS = ("conv.0.bias", "conv.3.bias", "up.1.bias")


@pytest.fixture(autouse=True)
def _release():
    yield
    torch.cuda.empty_cache()


def _norm_bias_of(name):
    """Key of the norm shift behind a convolution bias: the Sequential's next entry."""
    head, idx, _ = name.rsplit(".", 2)
    return f"{head}.{int(idx) + 1}.bias"


def _check_grads(grads, names, ref):
    """grads / ref: {key: gradient} (ref float64 or the fixture's float32 where it holds one); the bars of the module docstring."""
    dead = [n for n in names if n.endswith(CONV_BIAS) and float(np.abs(ref[n]).max()) < 1e-6 * float(np.abs(ref[_norm_bias_of(n)]).max())]
    live = [n for n in names if n not in dead]
    rel = {n: abs(float(np.linalg.norm(grads[n].astype(np.float64))) / float(np.linalg.norm(ref[n].astype(np.float64))) - 1) for n in live
           if n in ref}
    worst = max(rel, key=rel.get)
    print(f"  gradient norms: worst relative deviation {rel[worst]:.2e} ({worst})")
    small = {n: float(np.abs(grads[n] - ref[n]).max() / np.abs(ref[n]).max()) for n in live if ref[n].size <= 2048}
    worst_s = max(small, key=small.get)
    print(f"  small gradients: worst max abs deviation / max {small[worst_s]:.2e} ({worst_s})")
    left = {n: float(np.abs(grads[n]).max() / np.abs(ref[_norm_bias_of(n)]).max()) for n in dead}
    if left:
        print(f"  {len(dead)} convolution-bias gradients that are zero in exact arithmetic: worst |g| / max |norm-shift gradient| "
              f"{max(left.values()):.2e}")
    assert rel[worst] <= 2e-3, worst
    assert small[worst_s] <= 2e-3, worst_s
    assert all(v <= 2e-3 for v in left.values()), left
    return dead


def _step(m, x, t):
    """One forward / backward of the four-head Dice -> (heads, loss, {key: gradient as numpy})."""
    m.zero_grad()
    heads = m(x)
    assert isinstance(heads, tuple) and len(heads) == 4
    loss = R.ds_loss(heads, t)
    loss.backward()
    torch.cuda.synchronize()
    return [h.detach() for h in heads], float(loss.detach()), {k: p.grad.detach().cpu().numpy() for k, p in m.named_parameters()}


@pytest.mark.parametrize("precision", ["fp32", "x3"])
@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_matches_the_reference_fixture_and_float64(case, precision):
    z, meta = R.golden(case)
    names = meta["keys"]
    m = R.build(case).cuda().train()
    m.precision = precision
    assert list(m.state_dict()) == names
    x, t = R.image().cuda(), R.target().cuda()
    heads, loss, grads = _step(m, x, t)
    h64, loss64, g64 = R.fixture_run64(case)
    for i, (h, s) in enumerate(zip(heads, R.SCALES)):
        assert h.shape == (R.BATCH, 3, *R.SIZE) and h.dtype == torch.float32
        e_fix = float(np.abs(h.cpu().numpy()[:, :, ::s, ::s, ::s] - z[f"d{i + 1}"]).max())
        e_64 = float((h.cpu().double() - h64[i]).abs().max())
        print(f"  d{i + 1}: max abs err against the fixture {e_fix:.2e}, against float64 {e_64:.2e} (the reference's own: "
              f"{float(z['ref_err_heads']):.2e})")
        assert e_fix < HEAD_ATOL and e_64 < HEAD_ATOL
        if s > 1:  # nearest up-sampling: every s^3 block holds one value
            low = h[:, :, ::s, ::s, ::s]
            assert torch.equal(low.repeat_interleave(s, 2).repeat_interleave(s, 3).repeat_interleave(s, 4), h)
    print(f"  loss {loss:.7f} fixture {float(z['loss']):.7f} float64 {loss64:.7f}")
    assert abs(loss - float(z["loss"])) < 1e-4 and abs(loss - loss64) < 1e-4
    assert set(grads) == set(names)
    # against float64: every gradient; against the fixture: the norms of all, the values of those it holds
    ref64 = {n: g64[n].numpy() for n in names}
    dead = _check_grads(grads, names, ref64)
    fix_norms = dict(zip(names, z["grad_norms"]))
    norms = {n: float(np.linalg.norm(grads[n].astype(np.float64))) for n in names if n not in dead}
    worst = max(norms, key=lambda n: abs(norms[n] / fix_norms[n] - 1))
    print(f"  gradient norms against the fixture: worst relative deviation {abs(norms[worst] / fix_norms[worst] - 1):.2e} ({worst})")
    assert abs(norms[worst] / fix_norms[worst] - 1) <= 2e-3
    for k in (k for k in z.files if k.startswith("grad:") and k[5:] not in dead):
        assert float(np.abs(grads[k[5:]] - z[k]).max()) <= 2e-3 * float(np.abs(z[k]).max()), k
    conv_bias = [n for n in names if n.endswith(CONV_BIAS)]
    if case[0] == "group":
        # the convolution-bias gradients of the 16-, 32- and 64-wide units are real gradients: non-zero, and inside the bars above
        real = [n for n in conv_bias if n not in dead]
        assert len(real) == 12 and len(dead) == 5
        assert all(float(np.abs(grads[n]).max()) > 1e-3 * float(np.abs(ref64[_norm_bias_of(n)]).max()) for n in real)
    else:
        assert dead == conv_bias and len(dead) == 17


def test_bf16_is_finite_and_deviates_like_the_reference():
    """Forward and backward in bf16 are finite, and the mean |bf16 - f32| of d1 is at most FACTOR x the reference's own deviation
    under torch.autocast("cpu", bfloat16) (ref_bf16_dev of the fixture).  FACTOR = 2, the factor of tests/test_att_gpu.py for the
    same comparison: activations here are STORED in 16 bits between the norm and the next convolution, where autocast keeps the
    norms' outputs in f32 and rounds once on the way into the convolution -- other rounding points, the same number format.
    (First measurement: 4.69e-2 against the reference's 4.49e-2, ratio 1.05.)"""
    FACTOR = 2.0
    case = R.CASES[0]
    z, _ = R.golden(case)
    m = R.build(case).cuda().train()
    x, t = R.image().cuda(), R.target().cuda()
    with torch.no_grad():
        want = m(x)[0]
    m.precision = "bf16"
    heads, loss, grads = _step(m, x, t)
    assert np.isfinite(loss) and all(bool(torch.isfinite(h).all()) for h in heads)
    assert all(bool(np.isfinite(g).all()) for g in grads.values())
    dev = float((heads[0] - want).abs().mean())
    print(f"  mean |bf16 - f32| of d1 {dev:.4e}; the reference under bf16 autocast {float(z['ref_bf16_dev']):.4e}; "
          f"ratio {dev / float(z['ref_bf16_dev']):.3f}")
    assert dev <= FACTOR * float(z["ref_bf16_dev"])


@pytest.mark.parametrize("act", ["elu", "swish", "mish"])
def test_other_activations_match_float64(act):
    """The activations without a fold (no fused head, no fused pooling backward), instance norm, at the f32 bars on the heads and
    the loss; the restatement with the same closed-form weights is the reference."""
    case = ("instance", act)
    m = R.build(case).cuda().train()
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    x, t = R.image(), R.target()
    heads, loss, _ = _step(m, x.cuda(), t.cuda())
    h64, loss64, _ = R.run64(sd, x, t, case)
    errs = [float((h.cpu().double() - e).abs().max()) for h, e in zip(heads, h64)]
    print(f"  {act}: max abs err of the heads {max(errs):.2e}; loss {loss:.7f} float64 {loss64:.7f}")
    assert max(errs) < HEAD_ATOL and abs(loss - loss64) < 1e-4


def _train_run(graphed, steps=3, amp_dtype=torch.bfloat16):
    """`steps` recorded steps of TrainStep (autocast, fused Dice, Ranger2020) on a fixed batch of two after two unrecorded ones ->
    (losses, parameters); the manner of tests/test_refine_gpu.py."""
    from brats21_amd.engine import GraphedTrainStep, TrainStep
    from brats21_amd.optim import Ranger2020
    dev = torch.device("cuda")
    x = synth.random_image(2, 4, R.SIZE, seed=44).to(dev)
    t = R.target().to(dev)
    torch.manual_seed(0)
    m = R.build(load=False)
    m.precision = "auto"
    m = m.to(dev).train()
    opt = Ranger2020(m.parameters(), lr=1e-2, weight_decay=1e-5, use_gc=True, capturable=graphed)
    step = TrainStep(m, opt, amp=True, amp_dtype=amp_dtype)
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
    assert bool(torch.isfinite(l0).all()) and l0[-1] < l0[0], "three steps lower the loss on a fixed batch"
    assert torch.equal(l0, lg), (l0, lg)
    assert all(torch.equal(a, b) for a, b in zip(p0, pg)), "the replayed steps end at other weights than the eager ones"


def test_fp16_train_step_is_finite():
    losses, params = _train_run(False, steps=1, amp_dtype=torch.float16)
    assert bool(torch.isfinite(losses).all()) and all(bool(torch.isfinite(p).all()) for p in params)


def test_every_parameter_gradient_is_handed_over_exactly_once():
    """What data-parallel buckets depend on: one backward calls model._grad_sink once for each of the 76 parameter indices (17 units
    of four, four heads of two), with the gradient autograd then stores, and for no other."""
    m = R.build().cuda().train()
    seen = []
    m._grad_sink = lambda i, g: seen.append((i, g))
    _step(m, R.image().cuda(), R.target().cuda())
    params = list(m.parameters())
    assert sorted(i for i, _ in seen) == list(range(76)) == list(range(len(params)))
    assert all(g.shape == params[i].shape and torch.equal(g, params[i].grad) for i, g in seen)


def test_sliding_window_is_the_stitched_windows():
    """A 24 x 32 x 40 volume, 16 x 24 x 32 window, overlap 0.5, constant blend, f32: against d1 of the same model run window by
    window and averaged in torch.  Window starts, restated: interval = window * 0.5 = (8, 12, 16); per axis the starts 0 and one
    interval on, the last window shifted back to end at the volume's edge: (0, 8) on every axis."""
    from brats21_amd.inferers import sliding_window_inference
    m = R.build().cuda().eval()
    x = synth.random_image(1, 4, (24, 32, 40), seed=5).cuda()
    with torch.no_grad():
        got = sliding_window_inference(x, (16, 24, 32), 1, m, overlap=0.5, mode="constant")
        acc = torch.zeros((1, 3, 24, 32, 40), device=x.device)
        cnt = torch.zeros_like(acc)
        for z0 in (0, 8):
            for y0 in (0, 8):
                for x0 in (0, 8):
                    res = m(x[:, :, z0:z0 + 16, y0:y0 + 24, x0:x0 + 32].contiguous())
                    assert isinstance(res, tuple) and len(res) == 4
                    acc[:, :, z0:z0 + 16, y0:y0 + 24, x0:x0 + 32] += res[0]
                    cnt[:, :, z0:z0 + 16, y0:y0 + 24, x0:x0 + 32] += 1.0
    want = acc / cnt
    assert got.shape == want.shape and bool(torch.isfinite(got).all())
    tol = 1e-6 * float(want.abs().max())
    err = float((got - want).abs().max())
    print(f"  sliding window: max |got - want| {err:.2e} / {tol:.2e}")
    assert err <= tol
    # and one window of it is the restatement's d1 (float64), at the head bar
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    d1 = R.forward({k: v.double() for k, v in sd.items()}, x[:, :, :16, :24, :32].cpu().double())[0]
    with torch.no_grad():
        e = float((m(x[:, :, :16, :24, :32].contiguous())[0].cpu().double() - d1).abs().max())
    assert e < HEAD_ATOL


def test_return_value_without_deep_heads():
    x = R.image().cuda()
    m = R.build().cuda().eval()
    with torch.no_grad():
        full = m(x)
        m.skip_deep_heads_in_eval = True
        alone = m(x)
        single = R.build(deep_supervision=False).cuda().eval()(x)
        with torch.autocast("cuda", dtype=torch.bfloat16):  # (inference in 16 bits: the activation inside a block applied on load)
            low = m(x)
    assert isinstance(alone, torch.Tensor) and torch.equal(alone, full[0])
    assert isinstance(single, torch.Tensor) and torch.equal(single, full[0]), "the same closed-form weights, the same d1"
    assert isinstance(low, torch.Tensor) and bool(torch.isfinite(low).all())
    m.train()  # training mode: the deep heads are back, and d1 alone can carry the loss
    heads = m(x)
    assert len(heads) == 4
    R.dice_loss(heads[0], R.target().cuda()).backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for n, p in m.named_parameters() if not n.startswith("outconv"))
    with pytest.raises(ValueError, match="divisible by 8"):
        m(torch.zeros(1, 4, 16, 16, 12, device="cuda"))


def test_get_model_trains_and_evaluates():
    """definer.get_model(model="modified_unet"): one step through TrainStep, then sliding-window inference with the same module."""
    import argparse
    from brats21_amd import get_model
    from brats21_amd.engine import TrainStep
    from brats21_amd.inferers import sliding_window_inference
    from brats21_amd.optim import Ranger2020
    with contextlib.redirect_stdout(io.StringIO()):
        m = get_model(argparse.Namespace(model="modified_unet", width=8, norm="instance", act="relu", num_classes=3, dropout=0)).cuda().train()
    x, t = synth.random_image(1, 4, R.SIZE, seed=3).cuda(), R.target(1).cuda()
    loss = TrainStep(m, Ranger2020(m.parameters(), lr=1e-3), amp=True)(x, t)
    assert bool(torch.isfinite(loss))
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
    m.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        y = sliding_window_inference(x, R.SIZE, 1, m, overlap=0.5)
    assert y.shape == (1, 3, *R.SIZE) and bool(torch.isfinite(y).all())
