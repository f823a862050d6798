"""-m gpu: brats21_amd.networks.AttUnet / R2AttUnet and the pass they add.

The pass: brats_attgate_dx_unpool (ops.AttGatePending.finish on a skip tensor with a recorded arg-max plane) -- the gate's dx and the
un-pooling of the level in one launch -- bit for bit against its two parents, brats_attgate_dx followed by ops.maxpool2_bwd; and
ops.attgate_bwd(defer_dx=True) + finish() against ops.attgate_bwd().

The networks: against the reference's own classes (tests/golden/attunet_w8_*.npz, r2attunet_w8_*.npz, made by
tests/golden/make_golden_attunet.py) and against tests/_attunet_ref.py in float64, at the bars of tests/test_unet_gpu.py -- heads 1e-3
abs, loss 1e-4, gradient norms rtol 2e-3, small gradients 2e-3 of their maximum -- with its treatment of the convolution biases whose
gradient is zero in exact arithmetic, extended by the three convolution biases of every gate, which stand in front of a
training-mode BatchNorm: bounded absolutely, by 2e-3 of the maximum of the gradient of the BatchNorm shift behind them.  The gates'
buffers after the step: num_batches_tracked exactly, means and variances by tests/test_attgate_gpu.py's rule -- max abs error against
float64 over the buffer's max abs at most max(4 x the reference's recorded float32 error, 1e-6).  The reference's own f32 error
against float64 is recorded in the fixtures (ref_err_*)."""
import numpy as np
import pytest
import torch

import _attgate_ref as G
import _attunet_ref as R
from brats21_amd import _lib, ops
from brats21_amd import _attgate  # (after ops, which it is a part of)
from oracle import synth
from test_r2unet_gpu import _Recorder
from test_unet_gpu import HEAD_ATOL, _check_grads, _norm_bias_of, _step

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DT_IDS = ["f32", "bf16", "fp16"]
# [N, D, H, W, C].  N = 2: q is indexed across the batch, the pool walk is per sample.  In 16-bit storage: one full x segment of
# 128 + a tail of 2; 42 x positions per block + a tail of 2; four x positions per block
SHAPES = [(2, 4, 6, 8, 16), (1, 2, 2, 130, 16), (1, 2, 4, 44, 48), (1, 2, 2, 6, 384)]
SH_IDS = ["2x4x6x8x16", "1x2x2x130x16", "1x2x4x44x48", "1x2x2x6x384"]
KIND_CASES = [(k, c) for k in R.KINDS for c in R.CASES]
KC_IDS = [f"{k}-{i}" for k in R.KINDS for i in R.IDS]
GATE_BIAS = tuple(f"{b}.0.bias" for b in ("W_g", "W_x", "psi"))
NPARAMS = {k: v[1] for k, v in R.NKEYS.items()}


@pytest.fixture(autouse=True)
def _release():
    yield
    torch.cuda.empty_cache()


def _rand(shape, dtype, seed, scale=2.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(shape, device=DEV, generator=g) * scale).to(dtype)


def _st1(a=1.3, b=-0.2):
    """BN_1's table as the passes read it: entries 4, 5 = a, b of alpha = sigmoid(a q + b)."""
    return torch.tensor([0.1, 1.0, 1.0, 0.0, a, b, 0.0, 0.0], device=DEV)


def _operands(shape, dtype, seed=0):
    """-> (dout, t, q, st1, skip with its recorded arg-max plane, d_pooled)."""
    n, d, h, w, c = shape
    skip = _rand(shape, dtype, seed + 1)
    pooled = ops.maxpool2(skip, want_argmax=True)
    return (_rand(shape, dtype, seed + 2), _rand(shape, dtype, seed + 3), _rand((n * d * h * w,), torch.float32, seed + 4, 1.5), _st1(), skip,
            _rand(pooled.shape, dtype, seed + 5))


def _two_passes(dout, t, q, st1, skip, d_pooled):
    """What the pass replaces: brats_attgate_dx, then ops.maxpool2_bwd with dx as the skip gradient."""
    dx = ops.AttGatePending(dout, t, q, st1).finish()
    return dx, ops.maxpool2_bwd(skip, d_pooled, dx_skip=dx)


# ------------------------------------------------------------------------------------------ the pass
@pytest.mark.parametrize("shape", SHAPES, ids=SH_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_dx_unpool_is_the_two_passes_bit_for_bit(dtype, shape):
    dout, t, q, st1, skip, d_pooled = _operands(shape, dtype)
    dx, want = _two_passes(dout, t, q, st1, skip, d_pooled)
    assert int(skip._pool_argmax.max()) == 7 and int(skip._pool_argmax.min()) == 0
    got = ops.AttGatePending(dout, t, q, st1).finish(skip, d_pooled)
    assert got.dtype == dtype and got.shape == shape and torch.equal(got, want)
    # the pooled term is in it, at one voxel per window and channel; and the parents are the formula (f32 arithmetic)
    assert int((got != dx).sum()) > 0.9 * d_pooled.numel()
    alpha = torch.sigmoid(1.3 * q - 0.2).view(*shape[:4], 1)
    ref = (dout.float() * alpha + t.float()).to(dtype).float()
    # (one rounding to the storage type; f32: the kernel's fast exponential against torch's)
    rtol = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10, torch.float32: 1e-5}[dtype]
    assert float((dx.float() - ref).abs().max()) <= rtol * float(ref.abs().max())


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_dx_unpool_on_channel_slices(dtype):
    """dout, t and the output as channel slices of wider tensors (pitch 40, 32 and 56 against C = 24); the channels beside the
    output slice stay as they were."""
    shape, c = (2, 4, 6, 10, 24), 24
    dout, t, q, st1, skip, d_pooled = _operands(shape, dtype, 10)
    wide_d, wide_t, wide_o = _rand(shape[:4] + (40,), dtype, 20), _rand(shape[:4] + (32,), dtype, 21), _rand(shape[:4] + (56,), dtype, 22)
    before = wide_o.clone()
    ds, ts, out = wide_d[..., 8:8 + c], wide_t[..., 8:8 + c], wide_o[..., 16:16 + c]
    _, want = _two_passes(ds.contiguous(), ts.contiguous(), q, st1, skip, d_pooled)
    res = ops.AttGatePending(ds, ts, q, st1).finish(skip, d_pooled, out=out)
    assert res.data_ptr() == out.data_ptr() and torch.equal(out, want)
    assert torch.equal(wide_o[..., :16], before[..., :16]) and torch.equal(wide_o[..., 16 + c:], before[..., 16 + c:])


def test_a_window_of_eight_ties_goes_to_the_first_voxel():
    """A constant skip tensor: every window a tie of eight -> arg-max byte 0, the pooled gradient lands on the first voxel in d, h, w
    order and nowhere else."""
    shape = (2, 4, 6, 8, 16)
    dout, t, q, st1, _, d_pooled = _operands(shape, torch.bfloat16, 30)
    skip = torch.zeros(shape, dtype=torch.bfloat16, device=DEV)
    ops.maxpool2(skip, want_argmax=True)
    assert not bool(skip._pool_argmax.any())
    dx, want = _two_passes(dout, t, q, st1, skip, d_pooled)
    got = ops.AttGatePending(dout, t, q, st1).finish(skip, d_pooled)
    assert torch.equal(got, want)
    rest = got.clone()
    rest[:, ::2, ::2, ::2] = dx[:, ::2, ::2, ::2]
    assert torch.equal(rest, dx) and not torch.equal(got, dx)
    assert torch.equal(got[:, ::2, ::2, ::2], (d_pooled.float() + dx[:, ::2, ::2, ::2].float()).to(torch.bfloat16))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_finish_without_a_recorded_argmax_is_the_two_passes(dtype, monkeypatch):
    shape = (2, 4, 6, 8, 16)
    dout, t, q, st1, skip, d_pooled = _operands(shape, dtype, 40)
    _, want = _two_passes(dout, t, q, st1, skip, d_pooled)
    view = skip[:]  # (a view of its own: no recorded plane hangs on it -- the window is read again)
    assert getattr(view, "_pool_argmax", None) is None
    assert torch.equal(ops.AttGatePending(dout, t, q, st1).finish(view, d_pooled), want)
    out = torch.empty_like(dout)
    assert torch.equal(ops.AttGatePending(dout, t, q, st1).finish(view, d_pooled, out=out), want) and torch.equal(out, want)
    # and the size rule's other side: with the plane, below the threshold, the two passes run
    monkeypatch.setattr(_attgate, "DX_UNPOOL_MIN_BYTES", 1 << 40)
    assert torch.equal(ops.AttGatePending(dout, t, q, st1).finish(skip, d_pooled), want)


def test_bad_calls_raise_before_anything_is_launched():
    shape = (2, 4, 6, 8, 16)
    bf = torch.bfloat16
    dout, t, q, st1, skip, d_pooled = _operands(shape, bf, 50)
    odd = (2, 3, 6, 8, 16)
    odd_skip = _rand(odd, bf, 51)
    odd_skip._pool_argmax = torch.zeros((2, 1, 3, 4, 16), dtype=torch.uint8, device=DEV)
    wide = _rand(shape[:4] + (36,), bf, 52)  # pitch 36: no multiple of the 8-element channel vector

    def pend(dout=dout, t=t, q=q, st1=st1):
        return ops.AttGatePending(dout, t, q, st1)
    bad = {"odd D": lambda: pend(_rand(odd, bf, 53), _rand(odd, bf, 54), _rand((2 * 3 * 6 * 8,), torch.float32, 55)).finish(
               odd_skip, _rand((2, 1, 3, 4, 16), bf, 56)),
           "another storage type": lambda: pend(dout.double(), t.double()).finish(skip, d_pooled),
           "t of another storage type": lambda: pend(t=t.float()).finish(skip, d_pooled),
           "a CPU dout": lambda: pend(dout.cpu()).finish(skip, d_pooled),
           "a CPU d_pooled": lambda: pend().finish(skip, d_pooled.cpu()),
           "a misaligned pitch": lambda: pend(wide[..., :16]).finish(skip, d_pooled),
           "a misaligned out": lambda: pend().finish(skip, d_pooled, out=wide[..., 16:32]),
           "a short q": lambda: pend(q=q[:-1]).finish(skip, d_pooled),
           "a short st1": lambda: pend(st1=st1[:4]).finish(skip, d_pooled),
           "a short arg-max plane": lambda: pend().finish(_with_plane(skip, skip._pool_argmax[:1]), d_pooled),
           "d_pooled of the full size": lambda: pend().finish(skip, dout),
           "skip without d_pooled": lambda: pend().finish(skip),
           "out is dout": lambda: pend().finish(skip, d_pooled, out=dout)}
    wide32 = _rand(shape[:4] + (32,), bf, 58)
    bad["out overlaps t"] = lambda: pend(t=wide32[..., :16]).finish(skip, d_pooled, out=wide32[..., 8:24])
    real = _lib.lib()
    rec = _Recorder(real)
    _lib._lib = rec
    try:
        pend().finish(skip, d_pooled)
        assert rec.calls == ["brats_attgate_dx_unpool"]
        del rec.calls[:]
        pend().finish(skip[:], d_pooled)
        assert rec.calls == ["brats_attgate_dx", "brats_maxpool2_bwd"]
        del rec.calls[:]
        pend().finish()
        assert rec.calls == ["brats_attgate_dx"]
        del rec.calls[:]
        pend(t=wide32[..., :16]).finish(skip, d_pooled, out=wide32[..., 16:])  # (disjoint channel slices of one buffer)
        assert rec.calls == ["brats_attgate_dx_unpool"]
        for what, call in bad.items():
            del rec.calls[:]
            with pytest.raises(_lib.BratsHipError):
                call()
            assert rec.calls == [], what
    finally:
        _lib._lib = real
        ops.invalidate_packed_weights()


def _with_plane(skip, plane):
    v = skip[:]
    v._pool_argmax = plane
    return v


# ------------------------------------------------------------------------------------------ the deferred backward
@pytest.mark.parametrize("name", ["unlike", "narrow"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_deferred_backward_is_the_backward_bit_for_bit(dtype, name):
    sd, g, x, dout, _ = G.pick(name)
    params = [sd[k].to(DEV) for k in G.PARAMS]
    gs, xs, ds = (ops.ncdhw_to_ndhwc(v.to(DEV), dtype) for v in (g, x, dout))
    _, saved, _ = ops.attgate_fwd(gs, xs, params, "relu")
    dg, dx, grads = ops.attgate_bwd(ds, saved, params)
    dg2, pending, grads2 = ops.attgate_bwd(ds, saved, params, defer_dx=True)
    assert isinstance(pending, ops.AttGatePending) and pending.dout is ds and pending.q is saved.q and pending.st1 is saved.st1
    assert pending.t.shape == xs.shape and pending.t.dtype == dtype
    dx2 = pending.finish()
    assert pending.dout is None and pending.t is None, "spent: the two x-sized tensors are released"
    assert torch.equal(dg, dg2) and torch.equal(dx, dx2) and len(grads) == len(grads2) == 12
    assert all(torch.equal(a, b) for a, b in zip(grads, grads2))
    assert float(dx.float().abs().max()) > 0 and all(float(gr.abs().max()) > 0 for i, gr in enumerate(grads) if i not in (1, 5, 9))
    _, none, _ = ops.attgate_bwd(ds, saved, params, need_dx=False, defer_dx=True)
    assert none is None


# ------------------------------------------------------------------------------------------ the networks
def _buffers(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items() if R.is_buffer(k)}


@pytest.mark.parametrize("kind,case", KIND_CASES, ids=KC_IDS)
def test_matches_the_reference_fixture_and_float64(kind, case):
    z, meta = R.golden(kind, case)
    keys = meta["keys"]
    names = [k for k in keys if not R.is_buffer(k)]
    m = R.build(kind, case).cuda().train()
    assert list(m.state_dict()) == keys
    x, t = R.image().cuda(), R.target().cuda()
    heads, loss, grads = _step(m, x, t)
    after = _buffers(m)
    h64, loss64, g64, b64 = R.fixture_run64(kind, case)
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
    assert set(grads) == set(names) and len(names) == NPARAMS[kind]
    # against float64: every gradient; against the fixture: the norms of all, the values of those it holds.  The gates' three
    # convolution biases are zero in exact arithmetic (training-mode BatchNorm behind them): held absolutely, like the family's
    ref64 = {n: g64[n].numpy() for n in names}
    gate_dead = [n for n in names if n.startswith("Att") and n.endswith(GATE_BIAS)]
    assert len(gate_dead) == 9
    dead = _check_grads(grads, [n for n in names if n not in gate_dead], ref64)
    left = {n: float(np.abs(grads[n]).max() / np.abs(ref64[_norm_bias_of(n)]).max()) for n in gate_dead}
    print(f"  9 gate convolution-bias gradients that are zero in exact arithmetic: worst |g| / max |BatchNorm-shift gradient| "
          f"{max(left.values()):.2e}")
    assert all(float(np.abs(ref64[n]).max()) < 1e-6 * float(np.abs(ref64[_norm_bias_of(n)]).max()) for n in gate_dead)
    assert all(v <= 2e-3 for v in left.values()), left
    dead = dead + gate_dead
    fix_norms = dict(zip(names, z["grad_norms"]))
    norms = {n: float(np.linalg.norm(grads[n].astype(np.float64))) for n in names if n not in dead}
    worst = max(norms, key=lambda n: abs(norms[n] / fix_norms[n] - 1))
    print(f"  gradient norms against the fixture: worst relative deviation {abs(norms[worst] / fix_norms[worst] - 1):.2e} ({worst}; the "
          f"reference's own against float64: {float(z['ref_err_gnorm_rel']):.2e})")
    assert abs(norms[worst] / fix_norms[worst] - 1) <= 2e-3
    for k in (k for k in z.files if k.startswith("grad:") and k[5:] not in dead):
        assert float(np.abs(grads[k[5:]] - z[k]).max()) <= 2e-3 * float(np.abs(z[k]).max()), k
    assert len(dead) == 9 + (5 if case[0] == "group" else 17)
    # the gates' buffers after the one training forward
    lines, ok = [], True
    for k in (k for k in keys if R.is_buffer(k)):
        if k.endswith("num_batches_tracked"):
            assert int(after[k]) == int(z["buf:" + k]) == int(b64[k]) == 1, k
            continue
        scale = float(b64[k].abs().max())
        err, ref_err = float((after[k].cpu().double() - b64[k]).abs().max()) / scale, float(z["ref_err_buf:" + k]) / scale
        bar = max(4.0 * ref_err, 1e-6)
        lines.append(f"  {k}: max err / max {err:.2e} (bar {bar:.2e}, the reference's float32 {ref_err:.2e})")
        ok = ok and err <= bar
        assert float((after[k].cpu() - torch.from_numpy(z["buf:" + k])).abs().max()) / scale <= bar + ref_err, k
    print("\n".join(lines))
    assert ok, lines


@pytest.mark.parametrize("kind,case", KIND_CASES, ids=KC_IDS)
def test_eval_mode_heads_match_the_fixture(kind, case):
    """The inference path: eval mode, the loaded running buffers, no_grad -- against the reference's own eval-mode heads and against
    float64; the buffers stay as loaded.  (Measured, d1 against the fixture / float64: AttUnet 6.7e-5 / 6.7e-5 and 1.4e-4 / 2.1e-4;
    R2AttUnet 9.0e-4 / 7.2e-4 and 7.5e-4 / 7.3e-4, where the logits reach 32 and 56 and the reference's own float32 is at 2.8e-4 and
    3.3e-4 of float64.)"""
    z, _ = R.golden(kind, case)
    m = R.build(kind, case).cuda().eval()
    before = _buffers(m)
    with torch.no_grad():
        heads = m(R.image().cuda())
    e64 = R.fixture_run64(kind, case, training=False)[0]
    assert isinstance(heads, tuple) and len(heads) == 4
    for i, (h, s) in enumerate(zip(heads, R.SCALES)):
        e_fix = float(np.abs(h.cpu().numpy()[:, :, ::s, ::s, ::s] - z[f"eval_d{i + 1}"]).max())
        e_64 = float((h.cpu().double() - e64[i]).abs().max())
        print(f"  eval d{i + 1}: max abs err against the fixture {e_fix:.2e}, against float64 {e_64:.2e} (the reference's own: "
              f"{float(z['ref_err_eval']):.2e})")
        assert e_fix < HEAD_ATOL and e_64 < HEAD_ATOL
    assert all(torch.equal(v, before[k]) for k, v in _buffers(m).items())
    # training mode under no_grad still updates them, as torch does
    m.train()
    with torch.no_grad():
        m(R.image().cuda())
    now = _buffers(m)
    assert all(int(v) == 1 for k, v in now.items() if k.endswith("tracked"))
    assert not any(torch.equal(v, before[k]) for k, v in now.items())


@pytest.mark.parametrize("kind", R.KINDS)
def test_every_parameter_gradient_is_handed_over_exactly_once(kind):
    """What data-parallel buckets depend on: one backward calls model._grad_sink once for each of the 112 / 126 parameter indices,
    with the gradient autograd then stores, and for no other."""
    m = R.build(kind).cuda().train()
    seen = []
    m._grad_sink = lambda i, g: seen.append((i, g))
    _step(m, R.image().cuda(), R.target().cuda())
    params = list(m.parameters())
    assert sorted(i for i, _ in seen) == list(range(NPARAMS[kind])) == list(range(len(params)))
    assert all(g.shape == params[i].shape and torch.equal(g, params[i].grad) for i, g in seen)


@pytest.mark.parametrize("kind", R.KINDS)
def test_bf16_is_finite_and_deviates_like_the_reference(kind):
    """Forward and backward in bf16 are finite, and the mean |bf16 - f32| of d1 is at most FACTOR x the reference's own deviation
    under torch.autocast("cpu", bfloat16) (ref_bf16_dev of the fixture).  FACTOR = 2, the project's standing factor for this
    comparison (tests/test_unet_gpu.py, tests/test_r2unet_gpu.py)."""
    FACTOR = 2.0
    case = R.CASES[0]
    z, _ = R.golden(kind, case)
    m = R.build(kind, case).cuda().train()
    x, t = R.image().cuda(), R.target().cuda()
    with torch.no_grad():
        want = m(x)[0]
    m.precision = "bf16"
    heads, loss, grads = _step(m, x, t)
    assert np.isfinite(loss) and all(bool(torch.isfinite(h).all()) for h in heads)
    assert all(bool(np.isfinite(g).all()) for g in grads.values())
    assert all(bool(torch.isfinite(v).all()) for v in _buffers(m).values())
    dev = float((heads[0] - want).abs().mean())
    print(f"  mean |bf16 - f32| of d1 {dev:.4e}; the reference under bf16 autocast {float(z['ref_bf16_dev']):.4e}; "
          f"ratio {dev / float(z['ref_bf16_dev']):.3f}")
    assert dev <= FACTOR * float(z["ref_bf16_dev"])


def _train_run(kind, graphed, steps=3, amp_dtype=torch.bfloat16):
    """`steps` recorded steps of TrainStep (autocast, fused Dice, Ranger2020) on a fixed batch of two after two unrecorded ones ->
    (losses, parameters, gate buffers); the manner of tests/test_r2unet_gpu.py."""
    from brats21_amd.engine import GraphedTrainStep, TrainStep
    from brats21_amd.optim import Ranger2020
    dev = torch.device("cuda")
    x = synth.random_image(2, 4, R.SIZE, seed=44).to(dev)
    t = R.target().to(dev)
    torch.manual_seed(0)
    m = R.build(kind, load=False)
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
    return torch.stack(losses).cpu(), [p.detach().clone() for p in m.parameters()], _buffers(m)


@pytest.mark.parametrize("kind", R.KINDS)
def test_training_steps_eager_and_graphed_are_bit_identical(kind):
    l0, p0, b0 = _train_run(kind, False)
    lg, pg, bg = _train_run(kind, True)
    print(f"  eager {l0.tolist()} graphed {lg.tolist()}")
    assert bool(torch.isfinite(l0).all())
    assert torch.equal(l0, lg), (l0, lg)
    assert all(torch.equal(a, b) for a, b in zip(p0, pg)), "the replayed steps end at other weights than the eager ones"
    assert sorted(b0) == sorted(bg) and len(b0) == 27
    assert all(torch.equal(b0[k], bg[k]) for k in b0), "the replayed steps leave other BatchNorm buffers than the eager ones"
    assert all(int(v) == 5 for k, v in b0.items() if k.endswith("tracked")), "five training forwards each"


@pytest.mark.parametrize("kind", R.KINDS)
def test_fp16_train_step_is_finite(kind):
    losses, params, buffers = _train_run(kind, False, steps=1, amp_dtype=torch.float16)
    assert bool(torch.isfinite(losses).all()) and all(bool(torch.isfinite(p).all()) for p in params)
    assert all(bool(torch.isfinite(v).all()) for v in buffers.values())


@pytest.mark.parametrize("kind", R.KINDS)
def test_sliding_window_is_the_stitched_windows(kind):
    """A 24 x 32 x 40 volume, 16 x 24 x 32 window, overlap 0.5, constant blend, f32, eval mode (running statistics: the windows are
    independent of each other): against d1 of the same model run window by window and averaged in torch -- tests/test_r2unet_gpu.py's
    test.  Window starts: (0, 8) on every axis."""
    from brats21_amd.inferers import sliding_window_inference
    m = R.build(kind).cuda().eval()
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


@pytest.mark.parametrize("kind", R.KINDS)
def test_forward_time_refusals(kind):
    m = R.build(kind).cuda().train()
    x = R.image().cuda()
    before = _buffers(m)
    with pytest.raises(ValueError, match="divisible by 8"):
        m(torch.zeros(1, 4, 16, 16, 12, device="cuda"))
    m.precision = "x3"
    with pytest.raises(NotImplementedError, match="split-precision"):
        m(x)
    m.precision = "fp32"
    m.conv_fp8 = "fwd"
    with pytest.raises(NotImplementedError, match="e4m3"):
        m(x)
    m.conv_fp8 = None
    assert all(torch.equal(v, before[k]) for k, v in _buffers(m).items()), "a refused forward launches nothing"
    assert len(m(x)) == 4
