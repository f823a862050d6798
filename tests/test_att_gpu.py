"""-m gpu: brats21_amd.networks.AttEquiUnet and the three pooled passes of its gates (csrc/cbam.hip: brats_cbam_apply_pool,
brats_cbam_bwd_reduce_pool, brats_cbam_bwd_apply_pool).

Kernels: the fused forms are BIT-IDENTICAL to the composition they replace -- cbam_fwd + maxpool2(want_argmax) forward,
maxpool2_bwd(dx_skip=) + cbam_bwd backward -- in every output, for float32 and bfloat16 storage, on a single window, a non-cubic
shape with C % 16 != 0, a shape that crosses the 4 x 8 x 32 stencil tile and a workgroup chunk boundary, and an integer-valued input
whose windows hold equal maxima.

Network: the f32 mode against the reference's own class (tests/golden/att_w16_instance_relu.npz) and against tests/_att_ref.py in
float64, at the bars of tests/test_refine_gpu.py -- logits and deep heads 1e-3 abs, loss 1e-4, gradient norms rtol 2e-3, small
gradients 2e-3 of their maximum; the reference's own f32 error against float64 is recorded in the fixture (ref_err_*)."""
import json
import os

import numpy as np
import pytest
import torch

import _att_ref as R
from oracle import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOGIT_ATOL = 1e-3
STORAGES = (torch.float32, torch.bfloat16)
SHAPES = ((1, 16, 2, 2, 2),      # a single window
          (2, 24, 4, 6, 10),     # C not a multiple of 16, non-cubic, two samples
          (1, 16, 6, 10, 72))    # crosses the 4 x 8 x 32 tile; 4320 voxels: several workgroups (each walks 8 voxels per voxel lane)
IDS = ["x".join(map(str, s)) for s in SHAPES]


@pytest.fixture(autouse=True)
def _release():
    yield
    torch.cuda.empty_cache()


def _bits(t):
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _gate_case(shape, storage, ties=False):
    """(NDHWC input, seven parameters, skip gradient, pooled gradient) on the device.  ties: small integers and a spatial gate
    that is the same for every voxel (convolution weight 0), so equal inputs inside a window are equal stored outputs."""
    from brats21_amd import ops
    n, c, d, h, w = shape
    g = torch.Generator().manual_seed(1000 + sum(shape))
    ch = c // 16
    p = [torch.randn((ch, c), generator=g) * (2.0 / ch) ** 0.5, (torch.rand((ch,), generator=g) - 0.5) * 0.5,
         torch.randn((c, ch), generator=g) * (2.0 / c) ** 0.5, (torch.rand((c,), generator=g) - 0.5) * 0.5,
         torch.randn((1, 2, 7, 7, 7), generator=g) * (2.0 / 343) ** 0.5, torch.tensor([1.3]), torch.tensor([0.2])]
    if ties:
        x = torch.randint(-3, 4, shape, generator=g).float()
        p[4] = torch.zeros((1, 2, 7, 7, 7))
    else:
        x = (2 * torch.randn(shape, generator=g)).bfloat16().float()
    d_skip = torch.randn(shape, generator=g)
    d_pooled = torch.randn((n, c, d // 2, h // 2, w // 2), generator=g)
    to = lambda t: ops.ncdhw_to_ndhwc(t.to(DEV), storage)  # noqa: E731
    return to(x), [t.to(DEV) for t in p], to(d_skip), to(d_pooled)


def _composition_fwd(x, p):
    from brats21_amd import ops
    out, saved = ops.cbam_fwd(x, *p, save=True)
    pooled = ops.maxpool2(out, want_argmax=True)
    return out, pooled, saved


@pytest.mark.parametrize("storage", STORAGES, ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("ties", [False, True], ids=["random", "ties"])
def test_fused_forward_is_the_composition_bit_for_bit(shape, storage, ties):
    from brats21_amd import ops
    x, p, _, _ = _gate_case(shape, storage, ties)
    out, pooled, saved = ops.cbam_fwd(x, *p, save=True, pool=True)
    out_c, pooled_c, _ = _composition_fwd(x, p)
    n, c, d, h, w = shape
    assert pooled.shape == (n, d // 2, h // 2, w // 2, c) and pooled.dtype == storage and saved.pidx.dtype == torch.uint8
    assert _same_bits(out, out_c), "out"
    assert _same_bits(pooled, pooled_c), "pooled"
    assert torch.equal(saved.pidx, out_c._pool_argmax), "window-index bytes"
    if ties:
        win = out_c.float().view(n, d // 2, 2, h // 2, 2, w // 2, 2, c).permute(0, 1, 3, 5, 7, 2, 4, 6).reshape(n, d // 2, h // 2, w // 2, c, 8)
        tied = (win == win.max(-1, keepdim=True)[0]).sum(-1) > 1
        assert bool(tied.any()), "the case holds no equal maxima"
        # the first of equal maxima, in (d, h, w) window order
        first = (win == win.max(-1, keepdim=True)[0]).float().argmax(-1)
        assert torch.equal(saved.pidx.long(), first)
    # the inference form keeps nothing and writes no index plane; same tensors
    out_i, pooled_i, none = ops.cbam_fwd(x, *p, save=False, pool=True)
    assert none is None and _same_bits(out_i, out) and _same_bits(pooled_i, pooled)
    # calls without the new argument behave as before
    assert len(ops.cbam_fwd(x, *p, save=False)) == 2


@pytest.mark.parametrize("storage", STORAGES, ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("skip", [True, False], ids=["skip", "noskip"])
def test_fused_backward_is_the_composition_bit_for_bit(shape, storage, skip):
    from brats21_amd import ops
    x, p, d_skip, d_pooled = _gate_case(shape, storage)
    d_skip = d_skip if skip else None
    out, _, saved = ops.cbam_fwd(x, *p, save=True, pool=True)
    out_c, _, saved_c = _composition_fwd(x, p)
    dout = ops.maxpool2_bwd(out_c, d_pooled, dx_skip=d_skip)
    want = ops.cbam_bwd(dout, x, saved_c, *p)
    got = ops.cbam_bwd(d_skip, x, saved, *p, d_pooled=d_pooled)
    again = ops.cbam_bwd(d_skip, x, saved, *p, d_pooled=d_pooled)
    names = ("dx", "dW1", "db1", "dW2", "db2", "dWc", "dgamma", "dbeta")
    assert len(got) == len(want) == 8
    for name, a, b, c in zip(names, got, want, again):
        # (the MLP gradients may be all zero: a dead hidden unit at hidden width 1)
        assert bool(torch.isfinite(a.float()).all()) and (float(a.float().abs().max()) > 0 or name in ("dW1", "db1", "dW2")), name
        assert _same_bits(a, b), f"{name}: fused != composition"
        assert _same_bits(a, c), f"{name}: two runs differ"
    # the plain form is untouched by the new argument
    assert all(_same_bits(a, b) for a, b in zip(ops.cbam_bwd(dout, x, saved, *p), want))


def test_pooled_backward_refuses_what_it_cannot_compose():
    from brats21_amd import BratsHipError, ops
    x, p, d_skip, d_pooled = _gate_case(SHAPES[1], torch.float32)
    _, saved = ops.cbam_fwd(x, *p, save=True)
    with pytest.raises(BratsHipError, match="pool=True"):
        ops.cbam_bwd(d_skip, x, saved, *p, d_pooled=d_pooled)
    with pytest.raises(BratsHipError):
        ops.cbam_bwd(None, x, saved, *p)
    xo, po, _, _ = _gate_case((1, 16, 2, 3, 2), torch.float32)
    with pytest.raises(BratsHipError, match="even"):
        ops.cbam_fwd(xo, *po, pool=True)


# ------------------------------------------------------------------------------------------ the network, f32 mode
def _golden(golden_dir):
    return np.load(os.path.join(golden_dir, R.FNAME), allow_pickle=False)


def _check_grads(params, names, ref_norms, small):
    norms = np.array([float(params[n].grad.double().norm()) for n in names])
    rel = np.abs(norms - ref_norms) / np.maximum(ref_norms, 1e-30)  # (a gradient that is zero on both sides: 0)
    print(f"  gradient norms: worst relative deviation {rel.max():.2e} ({names[int(rel.argmax())]})")
    worst = max(float(np.abs(params[k].grad.cpu().numpy() - ref).max() / max(np.abs(ref).max(), 1e-6)) for k, ref in small.items())
    print(f"  small gradients: worst max abs deviation / max {worst:.2e}")
    np.testing.assert_allclose(norms, ref_norms, rtol=2e-3, atol=1e-7)
    for k, ref in small.items():
        np.testing.assert_allclose(params[k].grad.cpu().numpy(), ref, atol=2e-3 * max(np.abs(ref).max(), 1e-6), rtol=2e-3, err_msg=k)


def _step(m, x, t):
    """forward + five-head Dice + backward -> (heads, loss)"""
    m.zero_grad(set_to_none=True)
    res = m(x)
    loss = R.ds_loss(res, t)
    loss.backward()
    return [h.detach() for h in R.heads(res)], float(loss.detach())


def test_f32_matches_reference_golden(golden_dir):
    g = _golden(golden_dir)
    m = R.build(sd=R.weights()).cuda().train()
    x, t = R.image().cuda(), synth.nested_spheres(1, R.SIZE).cuda()
    heads, loss = _step(m, x, t)
    assert heads[0].shape == (1, 3, *R.SIZE) and len(heads) == 5 and all(h.shape == heads[0].shape for h in heads)
    e = np.abs(heads[0].cpu().numpy() - g["logits"]).max()
    print(f"  logits: max abs err {e:.2e} (the reference's own against f64: {float(g['ref_err_logits']):.2e})")
    assert e < LOGIT_ATOL
    for i, d in enumerate(heads[1:]):
        e = np.abs(d.cpu().numpy()[:, :, ::2, ::2, ::2] - g[f"deep{i}"]).max()
        assert e < LOGIT_ATOL, f"deep head {i} max abs err {e}"
    print(f"  loss {loss:.7f} golden {float(g['loss']):.7f}")
    assert abs(loss - float(g["loss"])) < 1e-4
    params = dict(m.named_parameters())
    names = json.loads(str(g["grad_names"]))
    assert names == list(params) and len(names) == 103
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0 for p in params.values())
    _check_grads(params, names, g["grad_norms"], {k[5:]: g[k] for k in g.files if k.startswith("grad:")})
    # the composition instead of the pooled gate passes: the same bits everywhere
    grads = [p.grad.clone() for p in m.parameters()]
    m.fold_gate_pool = False
    heads_c, loss_c = _step(m, x, t)
    assert loss_c == loss and all(_same_bits(a, b) for a, b in zip(heads, heads_c))
    assert all(_same_bits(a, p.grad) for a, p in zip(grads, m.parameters())), "fold_gate_pool=False gives other gradients"


def test_f32_non_cubic_batch_matches_float64():
    """2 x 4 x 16 x 24 x 32 at width 16 against tests/_att_ref.py on the CPU in float64, at the same bars; weights: the
    constructor's own initialisation under torch.manual_seed(0), copied into the restatement through the state dict.  Input seed:
    the one of 74 .. 77 with the smallest float32 error of the reference arithmetic itself (tests/_att_ref.py in float32 against
    float64 on the CPU, worst parameter-gradient |delta| / |g|: 5.0e-5 <-, 3.6e-3, 2.3e-5 -- its smallest gradients are smaller --,
    5.7e-4).  At this initialisation the one hidden unit of encoder1's gate is dead: three gradients are exactly zero on both sides."""
    size = (16, 24, 32)
    torch.manual_seed(0)
    m = R.build().cuda().train()
    x, t = R.image(2, size=size, seed=74), synth.nested_spheres(2, size)
    heads, loss = _step(m, x.cuda(), t.cuda())
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    assert list(sd) == list(R.state_shapes())
    heads64, loss64, g64 = R.run64(sd, x, t)
    for i, (got, want) in enumerate(zip(heads, heads64)):
        e = float((got.cpu().double() - want).abs().max())
        print(f"  head {i}: max abs err {e:.2e}")
        assert e < LOGIT_ATOL, i
    print(f"  loss {loss:.7f} float64 {loss64:.7f}")
    assert abs(loss - loss64) < 1e-4
    params = dict(m.named_parameters())
    names = list(params)
    assert len(names) == 103 and all(p.grad is not None for p in params.values())
    _check_grads(params, names, np.array([float(g64[n].norm()) for n in names]),
                 {n: g64[n].float().numpy() for n in names if g64[n].numel() <= 2048})


def test_bf16_is_finite_and_deviates_like_the_reference(golden_dir):
    """Forward and backward in bf16 are finite, and the mean |bf16 - f32| of the logits is at most FACTOR x the reference's own
    deviation under torch.autocast("cpu", bfloat16) (ref_bf16_dev of the fixture).  FACTOR = 2, set after the first
    measurement (6.63e-2 against the reference's 8.58e-2: ratio 0.77) and not tuned since: activations here are STORED in 16 bits
    between the norm, the gate and the next convolution, where autocast keeps the norms' outputs in f32 and rounds once on the way
    into the convolution -- other rounding points, the same number format, so the same size of deviation is expected and twice
    it is allowed (the factor of tests/test_refine_gpu.py for the same comparison)."""
    FACTOR = 2.0
    g = _golden(golden_dir)
    m = R.build(sd=R.weights()).cuda().train()
    x, t = R.image().cuda(), synth.nested_spheres(1, R.SIZE).cuda()
    with torch.no_grad():
        want = m(x)[0]
    m.precision = "bf16"
    heads, loss = _step(m, x, t)
    assert np.isfinite(loss) and all(bool(torch.isfinite(h).all()) for h in heads)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
    dev = float((heads[0] - want).abs().mean())
    print(f"  mean |bf16 - f32| of the logits {dev:.4e}; the reference under bf16 autocast {float(g['ref_bf16_dev']):.4e}; "
          f"ratio {dev / float(g['ref_bf16_dev']):.3f}")
    assert dev <= FACTOR * float(g["ref_bf16_dev"])
    m.precision = "auto"
    with torch.autocast("cuda", dtype=torch.float16), pytest.raises(NotImplementedError, match="fp16"):
        m(x)


def test_x3_mode_runs_at_the_f32_bars(golden_dir):
    """precision="x3" (fp16-pair convolutions on f32 tensors): the gates take the f32 tensors; logits at the f32 bar."""
    g = _golden(golden_dir)
    m = R.build(sd=R.weights()).cuda().train()
    m.precision = "x3"
    heads, loss = _step(m, R.image().cuda(), synth.nested_spheres(1, R.SIZE).cuda())
    assert np.abs(heads[0].cpu().numpy() - g["logits"]).max() < LOGIT_ATOL and abs(loss - float(g["loss"])) < 1e-4
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())


# ------------------------------------------------------------------------------------------ the step, inference
def _train_run(graphed, steps=2, dropout=0):
    """`steps` recorded steps of TrainStep (bf16 autocast, fused Dice, Ranger2020) on a batch of two after two unrecorded ones ->
    (losses, parameters)"""
    from brats21_amd.engine import GraphedTrainStep, TrainStep
    from brats21_amd.optim import Ranger2020
    dev = torch.device("cuda")
    x = R.image(2, seed=44).to(dev)
    t = synth.nested_spheres(2, R.SIZE).to(dev)
    torch.manual_seed(0)
    m = R.build(dropout=dropout)
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
    assert bool(torch.isfinite(l0).all())
    assert torch.equal(l0, lg), (l0, lg)
    assert all(torch.equal(a, b) for a, b in zip(p0, pg)), "the replayed steps end at other weights than the eager ones"


def test_dropout_trains_one_step():
    losses, params = _train_run(False, steps=1, dropout=0.1)
    assert bool(torch.isfinite(losses).all()) and all(bool(torch.isfinite(p).all()) for p in params)


def test_eval_forward_skips_the_deep_heads_and_keeps_nothing():
    m = R.build(sd=R.weights()).cuda().train()
    x = R.image().cuda()
    with torch.no_grad():
        want = m(x)[0]
    m.eval()
    m.skip_deep_heads_in_eval = True
    with torch.no_grad():
        out, deeps = m(x)
    assert deeps == [] and _same_bits(out, want), "instance norm: eval and training forward are the same function"
    m.precision = "bf16"
    with torch.no_grad():
        out16, _ = m(x)
    assert bool(torch.isfinite(out16).all())


def test_sliding_window_and_evaluator_on_one_window_are_the_direct_forward():
    from brats21_amd.inferers import sliding_window_inference
    m = R.build(sd=R.weights(), deep_supervision=False).cuda().eval()
    x = R.image().cuda()
    with torch.no_grad():
        want = m(x)
        got = sliding_window_inference(x, R.SIZE, 1, m, overlap=0.5, mode="constant")
    assert got.shape == want.shape == (1, 3, *R.SIZE)
    err, tol = float((got - want).abs().max()), 1e-6 * float(want.abs().max())
    print(f"  sliding window: max |got - want| {err:.2e} / {tol:.2e}")
    assert err <= tol
    # the Evaluator on the same volume (its patch step captured into a hipGraph): the probability and the thresholded map of the
    # direct forward (seeded noise: no all-zero voxel for the background removal to clear)
    from brats21_amd.evaluate import Evaluator
    ev = Evaluator(m, sliding_window_size=R.SIZE, overlap=0.5, amp=False)
    prob, passes = ev.probability_sum(x)
    assert passes == 1 and float((prob - torch.sigmoid(want)).abs().max()) <= 1e-6
    seg = ev(x)["seg"]
    differs = (seg > 0.5) != (torch.sigmoid(want) > 0.5)
    assert seg.shape == want.shape and not bool((differs & ((torch.sigmoid(want) - 0.5).abs() > 1e-6)).any())


def test_cpu_input_is_refused():
    from brats21_amd import BratsHipError
    with pytest.raises(BratsHipError):
        R.build().cuda()(torch.zeros(1, 4, 16, 16, 16))
