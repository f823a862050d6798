"""-m gpu: brats21_amd.networks.R2Unet and the pass it adds.

The pass: ops.affine_act_add(pool=True) -- the last normalise pass of an encoder block, which writes the block output and its 2x2x2
max pool (brats_affine_act_add_pool_fwd) -- bit for bit against ops.affine_act_add followed by ops.maxpool2(want_argmax=True), and
ops.rrcnn_fwd(pool=True) against ops.rrcnn_fwd() + ops.maxpool2.

The network: against the reference's own class (tests/golden/r2unet_w8_*.npz, made by tests/golden/make_golden_r2unet.py) and against
tests/_r2unet_ref.py in float64, at the bars of tests/test_unet_gpu.py -- heads 1e-3 abs, loss 1e-4, gradient norms rtol 2e-3, small
gradients 2e-3 of their maximum -- and with its treatment of the convolution biases in front of a per-channel normalisation, whose
gradient is zero in exact arithmetic (sum_v dy = 0): those are bounded absolutely, by 2e-3 of the maximum of the gradient of the
unit's norm shift.  Such biases here: 5 of the 17 under group / relu (the 8-wide units of RRCNN1, Up2 and Up_RRCNN2: 8 groups of one
channel), all 17 under instance / leakyrelu (the 14 recurrent units and the 3 UpConv units).  The reference's own f32 error against
float64 is recorded in the fixtures (ref_err_*) and in tests/_r2unet_ref.py's docstring."""
import re

import numpy as np
import pytest
import torch

import _r2unet_ref as R
from brats21_amd import _lib, ops
from oracle import synth
from test_unet_gpu import HEAD_ATOL, _check_grads, _norm_bias_of, _step

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DT_IDS = ["f32", "bf16", "fp16"]
# [N, D, H, W, C].  In 16-bit storage: 128 x positions per item + a tail of 2; 42 + a tail of 2; four x positions per block
SHAPES = [(2, 4, 6, 8, 16), (1, 2, 2, 130, 16), (1, 2, 4, 44, 48), (1, 2, 2, 6, 384)]
SH_IDS = ["2x4x6x8x16", "1x2x2x130x16", "1x2x4x44x48", "1x2x2x6x384"]
CONV_BIAS = ("conv.0.bias", "up.1.bias")


@pytest.fixture(autouse=True)
def _release():
    yield
    torch.cuda.empty_cache()


def _rand(shape, dtype, seed, scale=2.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(shape, device=DEV, generator=g) * scale).to(dtype)


def _ss(n, c, seed):
    """[N, C, 2] {scale, shift}: scales of both signs around 1, shifts around 0."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    ss = torch.randn((n, c, 2), device=DEV, generator=g)
    ss[..., 0] = ss[..., 0] * 0.5 + 1.0
    return ss.contiguous()


def _two_passes(y, ss, add, act):
    """What the pass replaces: -> (out, pooled, arg-max bytes)."""
    out = ops.affine_act_add(y, ss, add, act)
    pooled = ops.maxpool2(out, want_argmax=True)
    return out, pooled, out._pool_argmax


# ------------------------------------------------------------------------------------------ the pass
@pytest.mark.parametrize("shape", SHAPES, ids=SH_IDS)
@pytest.mark.parametrize("act", ["relu", "leakyrelu"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_add_pool_is_the_two_passes_bit_for_bit(dtype, act, shape):
    y, add, ss = _rand(shape, dtype, 1), _rand(shape, dtype, 2), _ss(shape[0], shape[-1], 3)
    want, want_p, want_i = _two_passes(y, ss, add, act)
    out, pooled = ops.affine_act_add(y, ss, add, act, pool=True, want_argmax=True)
    assert out.dtype == pooled.dtype == dtype and pooled.shape == (shape[0], shape[1] // 2, shape[2] // 2, shape[3] // 2, shape[4])
    assert torch.equal(out, want) and torch.equal(pooled, want_p)
    assert out._pool_argmax.dtype == torch.uint8 and torch.equal(out._pool_argmax, want_i)
    assert int(want_i.max()) == 7 and int(want_i.min()) == 0 and float(pooled.float().abs().max()) > 1.0
    # without the bytes: the same two tensors, nothing hung on the output
    out2, pooled2 = ops.affine_act_add(y, ss, add, act, pool=True)
    assert torch.equal(out2, want) and torch.equal(pooled2, want_p) and getattr(out2, "_pool_argmax", None) is None


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_add_pool_on_channel_slices(dtype):
    """add and the output as channel slices of wider tensors (pitch 40 and 56 against C = 24); the channels beside the output slice
    stay as they were."""
    shape, c = (2, 4, 6, 10, 24), 24
    y, ss = _rand(shape, dtype, 7), _ss(2, c, 8)
    wide_add, wide_out = _rand(shape[:4] + (40,), dtype, 9), _rand(shape[:4] + (56,), dtype, 10)
    before = wide_out.clone()
    add, out = wide_add[..., 8:8 + c], wide_out[..., 16:16 + c]
    want, want_p, want_i = _two_passes(y, ss, add.contiguous(), "leakyrelu")
    res, pooled = ops.affine_act_add(y, ss, add, "leakyrelu", out=out, pool=True, want_argmax=True)
    assert res.data_ptr() == out.data_ptr()
    assert torch.equal(out, want) and torch.equal(pooled, want_p) and torch.equal(res._pool_argmax, want_i)
    assert torch.equal(wide_out[..., :16], before[..., :16]) and torch.equal(wide_out[..., 16 + c:], before[..., 16 + c:])


def test_all_ties_go_to_the_first_voxel():
    """add = 0 and y < 0 under relu: every stored value is 0, every window a tie of eight -> the first voxel in d, h, w order (byte
    0), and the pooling backward from the bytes is the pooling backward from the window."""
    shape = (2, 4, 6, 8, 16)
    y = -_rand(shape, torch.bfloat16, 11).abs() - 1.0
    ss = torch.zeros((2, 16, 2), device=DEV)
    ss[..., 0] = 1.0
    out, pooled = ops.affine_act_add(y, ss, torch.zeros_like(y), "relu", pool=True, want_argmax=True)
    assert not bool(out.any()) and not bool(pooled.any()) and not bool(out._pool_argmax.any())
    dy = _rand(pooled.shape, torch.bfloat16, 12)
    from_bytes = ops.maxpool2_bwd(out, dy)
    from_window = ops.maxpool2_bwd(out[:], dy)  # (a view of its own: no recorded plane hangs on it)
    assert torch.equal(from_bytes, from_window)
    assert torch.equal(from_bytes[:, ::2, ::2, ::2], dy) and float(from_bytes.float().abs().sum()) == float(dy.float().abs().sum())


@pytest.mark.parametrize("act", ["elu", "swish", "mish"])
def test_the_other_activations_give_the_same_bits(act):
    shape = (2, 4, 6, 8, 24)
    for dtype in DTYPES:
        y, add, ss = _rand(shape, dtype, 13), _rand(shape, dtype, 14), _ss(2, 24, 15)
        want, want_p, want_i = _two_passes(y, ss, add, act)
        out, pooled = ops.affine_act_add(y, ss, add, act, pool=True, want_argmax=True)
        assert torch.equal(out, want) and torch.equal(pooled, want_p) and torch.equal(out._pool_argmax, want_i)


def test_add_pool_across_the_non_temporal_switch():
    """From 256 MiB on the pass streams with non-temporal accesses on 8192 blocks: the smallest bf16 tensor across the switch (one
    sample of it is below), against the two passes and against the pass on one sample."""
    shape = (2, 64, 128, 128, 64)
    y, add, ss = _rand(shape, torch.bfloat16, 16), _rand(shape, torch.bfloat16, 17), _ss(2, 64, 18)
    assert y.numel() * y.element_size() == (256 << 20) > y[0].numel() * y.element_size()
    out, pooled = ops.affine_act_add(y, ss, add, "relu", pool=True, want_argmax=True)
    one, one_p = ops.affine_act_add(y[1:], ss[1:].contiguous(), add[1:], "relu", pool=True, want_argmax=True)
    assert torch.equal(out[1:], one) and torch.equal(pooled[1:], one_p) and torch.equal(out._pool_argmax[1:], one._pool_argmax)
    del one, one_p
    want = ops.affine_act_add(y, ss, add, "relu")
    assert torch.equal(out, want)
    del out
    assert torch.equal(pooled, ops.maxpool2(want, want_argmax=True))


class _Recorder:
    """The loaded library with every entry point that takes a stream recorded instead of called (tests/test_ops_checks_gpu.py)."""

    def __init__(self, real):
        txt = re.sub(r"/\*.*?\*/", " ", open(_lib.HEADER_PATH).read(), flags=re.S)
        self._launch = {m.group(1) for m in re.finditer(r"(brats_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", txt) if "brats_stream_t" in m.group(2)}
        self._real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in self._launch:
            return fn

        def recorded(*a):
            self.calls.append(name)
            return 0
        return recorded


def test_bad_calls_raise_before_anything_is_launched():
    shape = (2, 4, 6, 8, 16)
    y, add, ss = _rand(shape, torch.bfloat16, 19), _rand(shape, torch.bfloat16, 20), _ss(2, 16, 21)
    odd = (2, 3, 6, 8, 16)
    wide = _rand(shape[:4] + (32,), torch.bfloat16, 22)
    bad = {"odd D": lambda: ops.affine_act_add(_rand(odd, torch.bfloat16, 23), ss, _rand(odd, torch.bfloat16, 24), pool=True),
           "a CPU add": lambda: ops.affine_act_add(y, ss, add.cpu(), pool=True),
           "add of another storage type": lambda: ops.affine_act_add(y, ss, add.float(), pool=True),
           "out is y": lambda: ops.affine_act_add(y, ss, add, out=y, pool=True),
           "out overlaps y": lambda: ops.affine_act_add(wide[..., :16], ss, add, out=wide[..., 8:24], pool=True),
           "out overlaps add": lambda: ops.affine_act_add(y, ss, wide[..., 8:24], out=wide[..., :16], pool=True),
           "out of another storage type": lambda: ops.affine_act_add(y, ss, add, out=torch.empty(shape, device=DEV), pool=True),
           "a short scale_shift": lambda: ops.affine_act_add(y, ss[:1], add, pool=True),
           "want_argmax without pool": lambda: ops.affine_act_add(y, ss, add, want_argmax=True),
           "rrcnn_fwd(pool=True), odd D": lambda: ops.rrcnn_fwd(_rand(odd, torch.bfloat16, 25), None, _block_params(16, 16), 8, "relu", 1,
                                                                pool=True)}
    real = _lib.lib()
    rec = _Recorder(real)
    _lib._lib = rec
    try:
        ops.affine_act_add(y, ss, add, pool=True, want_argmax=True)
        assert rec.calls == ["brats_affine_act_add_pool_fwd"]
        del rec.calls[:]
        ops.affine_act_add(y, ss, add, "mish", pool=True)
        assert rec.calls == ["brats_affine_act_add_fwd", "brats_maxpool2_fwd"]
        del rec.calls[:]
        ops.affine_act_add(y, ss, wide[..., 16:], out=wide[..., :16], pool=True)  # (disjoint channel slices of one buffer)
        assert rec.calls == ["brats_affine_act_add_pool_fwd"]
        for what, call in bad.items():
            del rec.calls[:]
            with pytest.raises(_lib.BratsHipError):
                call()
            assert rec.calls == [], what
    finally:
        _lib._lib = real
        ops.invalidate_packed_weights()


# ------------------------------------------------------------------------------------------ the block
def _block_params(cin, c):
    """The ten parameters of an RRCNNblock in state-dict order, closed-form values."""
    import _rrcnn_ref as B
    return [v.to(DEV) for v in B.weights(B.shapes_of(cin, c)).values()]


ROUTES = {"one_pass": 0, "by_size": ops.POOL_FUSED_MIN_BYTES}  # the last pass of an encoder block: always fused / the size rule


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("save", [True, False], ids=["save", "no_save"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_rrcnn_fwd_with_pool_is_rrcnn_fwd_and_maxpool2(dtype, save, route, monkeypatch):
    monkeypatch.setattr(ops, "POOL_FUSED_MIN_BYTES", ROUTES[route])
    x = _rand((2, 4, 6, 8, 16), dtype, 26, scale=1.0)
    params = _block_params(16, 24)
    want, _ = ops.rrcnn_fwd(x, None, params, 8, "relu", 2, save=save)
    want_p = ops.maxpool2(want, want_argmax=True)
    (out, pooled), saved = ops.rrcnn_fwd(x, None, params, 8, "relu", 2, save=save, pool=True)
    assert torch.equal(out, want) and torch.equal(pooled, want_p)
    assert (saved is not None) == save
    if save:
        assert torch.equal(out._pool_argmax, want._pool_argmax)
    else:
        assert getattr(out, "_pool_argmax", None) is None


# ------------------------------------------------------------------------------------------ the network
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_matches_the_reference_fixture_and_float64(case, route, monkeypatch):
    monkeypatch.setattr(ops, "POOL_FUSED_MIN_BYTES", ROUTES[route])
    z, meta = R.golden(case)
    names = meta["keys"]
    m = R.build(case).cuda().train()
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
    print(f"  convolution biases in front of a norm: {len(conv_bias)}, zero in exact arithmetic: {len(dead)}")
    if case[0] == "group":
        # the convolution-bias gradients of the 16-, 32- and 64-wide units are real gradients: non-zero, and inside the bars above
        real = [n for n in conv_bias if n not in dead]
        assert len(real) == 12 and len(dead) == 5
        assert all(float(np.abs(grads[n]).max()) > 1e-3 * float(np.abs(ref64[_norm_bias_of(n)]).max()) for n in real)
    else:
        assert dead == conv_bias and len(dead) == 17


@pytest.mark.parametrize("t", [1, 3])
def test_other_recurrence_depths_match_float64(t):
    """t = 1 and t = 3, group / relu, the fixture's input: heads, loss and every gradient against the restatement in float64.  (The
    reference's own f32 error there: gradient norms 5e-6 / 1.8e-5, small gradients 1.1e-5 / 2.5e-5.)"""
    case = R.CASES[0]
    m = R.build(case, t=t).cuda().train()
    names = [n for n, _ in m.named_parameters()]
    heads, loss, grads = _step(m, R.image().cuda(), R.target().cuda())
    h64, loss64, g64 = R.fixture_run64(case, rec=t)
    errs = [float((h.cpu().double() - e).abs().max()) for h, e in zip(heads, h64)]
    print(f"  t = {t}: max abs err of the heads {max(errs):.2e}; loss {loss:.7f} float64 {loss64:.7f}")
    assert max(errs) < HEAD_ATOL and abs(loss - loss64) < 1e-4
    dead = _check_grads(grads, names, {n: g64[n].numpy() for n in names})
    assert len(dead) == 5


@pytest.mark.parametrize("act", ["elu", "swish", "mish"])
def test_other_activations_match_float64(act):
    """The activations without a one-pass pooled form, instance norm, at the f32 bars on the heads and the loss; the restatement with
    the same closed-form weights is the reference."""
    case = ("instance", act)
    m = R.build(case).cuda().train()
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    x, t = R.image(), R.target()
    heads, loss, _ = _step(m, x.cuda(), t.cuda())
    h64, loss64, _ = R.run64(sd, x, t, case)
    errs = [float((h.cpu().double() - e).abs().max()) for h, e in zip(heads, h64)]
    print(f"  {act}: max abs err of the heads {max(errs):.2e}; loss {loss:.7f} float64 {loss64:.7f}")
    assert max(errs) < HEAD_ATOL and abs(loss - loss64) < 1e-4


def test_bf16_is_finite_and_deviates_like_the_reference():
    """Forward and backward in bf16 are finite, and the mean |bf16 - f32| of d1 is at most FACTOR x the reference's own deviation
    under torch.autocast("cpu", bfloat16) (ref_bf16_dev of the fixture).  FACTOR = 2, the project's standing factor for this
    comparison (tests/test_unet_gpu.py, tests/test_att_gpu.py): activations here are STORED in 16 bits between the norm and the next
    convolution, where autocast keeps the norms' outputs in f32 -- other rounding points, the same number format.
    (Measured: 2.99e-2 against the reference's 3.13e-2, ratio 0.956.)"""
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


def _train_run(graphed, steps=3, amp_dtype=torch.bfloat16):
    """`steps` recorded steps of TrainStep (autocast, fused Dice, Ranger2020) on a fixed batch of two after two unrecorded ones ->
    (losses, parameters); the manner of tests/test_unet_gpu.py."""
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
    """What data-parallel buckets depend on: one backward calls model._grad_sink once for each of the 90 parameter indices, with
    the gradient autograd then stores, and for no other."""
    m = R.build().cuda().train()
    seen = []
    m._grad_sink = lambda i, g: seen.append((i, g))
    _, _, grads = _step(m, R.image().cuda(), R.target().cuda())
    assert sorted(i for i, _ in seen) == list(range(90)) == list(range(len(list(m.parameters()))))
    params = list(m.parameters())
    assert all(g.shape == params[i].shape and torch.equal(g, params[i].grad) for i, g in seen)


def test_return_value_without_deep_heads():
    x = R.image().cuda()
    m = R.build().cuda().train()
    trained = m(x)[0].detach()
    m.eval()
    with torch.no_grad():
        full = m(x)
        m.skip_deep_heads_in_eval = True
        alone = m(x)
        single = R.build(deep_supervision=False).cuda().eval()(x)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            low = m(x)
    assert isinstance(full, tuple) and len(full) == 4
    assert torch.equal(full[0], trained), "no_grad / eval: d1 has the training forward's bits"
    assert isinstance(alone, torch.Tensor) and torch.equal(alone, full[0])
    assert isinstance(single, torch.Tensor) and torch.equal(single, full[0]), "the same closed-form weights, the same d1"
    assert isinstance(low, torch.Tensor) and bool(torch.isfinite(low).all())
    m.train()  # training mode: the deep heads are back, and d1 alone can carry the loss
    heads = m(x)
    assert len(heads) == 4
    R.dice_loss(heads[0], R.target().cuda()).backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for n, p in m.named_parameters() if not n.startswith("outconv"))


def test_sliding_window_is_the_stitched_windows():
    """A 24 x 32 x 40 volume, 16 x 24 x 32 window, overlap 0.5, constant blend, f32: against d1 of the same model run window by
    window and averaged in torch.  Window starts: interval = window * 0.5 = (8, 12, 16); per axis the starts 0 and one interval on,
    the last window shifted back to end at the volume's edge: (0, 8) on every axis."""
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


def test_forward_time_refusals():
    m = R.build().cuda().train()
    x = R.image().cuda()
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
    assert len(m(x)) == 4
