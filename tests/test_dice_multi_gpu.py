"""-m gpu: the all-heads Dice entries (brats_dice_stats_multi / brats_dice_finish / brats_dice_grad_multi, csrc/dice.hip), the
path of losses.fused_deep_supervision_dice built on them, and ops.upsample_bwd with an addend (brats_upsample_bwd_add,
csrc/pool_up.hip).

Everything here is a bit-for-bit statement (torch.equal) against what the step computed before these entries existed:
  * per-block partials and totals of every head against one brats_dice_stats call for that head;
  * the coefficients against the torch algebra _FusedDiceFn.forward ran on the [heads][classes] sums, copied below
    (_torch_algebra), on the same sums;
  * the gradients against one brats_dice_grad call per head with (coef * g).contiguous();
  * the adjoint with addend against ops.upsample_bwd(dy) + add.
The one exception is the loss value: the mean of the H * K per-class values is added in torch's order as far as that order is
known, and is asserted to within one f32 ulp of torch's mean (the test prints whether it is equal).

Shapes: 210 voxels (5 x 6 x 7: no multiple of 4, the scalar loop only), 7680 voxels (two blocks on the 16-byte path), 128^3
(the block count is exactly the cap of 512) and 208 x 208 x 200 (above the cap: some blocks take a second trip); H = 1, 5, 6
heads, K = 1, 3 classes.  One case has one head's storage start 4 bytes off a 16-byte boundary: the all-heads kernels then send
EVERY head through the scalar loop (the target vector is loaded once for all heads, so there is one path per launch), and
the per-head reference is given each head at such an address too, so that it takes the scalar loop as well.

The end-to-end bounds are those of tests/test_loss_end_gpu.py for the same quantities: loss within max(4 x the error of the
same loss evaluated by torch in f32 against f64, 1e-6 relative); gradients rtol 1e-4, atol 1e-9 against f64 autograd.
"""
import argparse
import contextlib
import io

import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")
BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32


@pytest.fixture(autouse=True)
def _release():
    yield
    torch.cuda.empty_cache()


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _gen(seed):
    return torch.Generator(device=_dev()).manual_seed(seed)


def _ptrs(tensors):
    import ctypes
    return (ctypes.c_void_p * len(tensors))(*[x.data_ptr() for x in tensors])


def _gx(vox, cap):
    return min(max((vox // 4 + 255) // 256 // 4, 1), cap)


def _offset_copy(x, floats):
    """x at an address `floats` f32 past a 16-byte boundary"""
    buf = torch.full((x.numel() + 4,), NAN, device=x.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[floats:floats + x.numel()].view(x.shape)
    v.copy_(x)
    return v


def _inputs(seed, nh, n, k, shape, offset_head=None):
    g = _gen(seed)
    heads = [torch.randn((n, k, *shape), generator=g, device=_dev()).mul_(3.0).clamp_(-12.0, 12.0) for _ in range(nh)]
    if offset_head is not None:
        heads[offset_head] = _offset_copy(heads[offset_head], 1)
    t = (torch.rand((n, k, *shape), generator=g, device=_dev()) > 0.6).float()
    return heads, t


def _stats_multi(heads, t):
    """-> (ws [H][floats per head], blocks per sample); the workspace starts as NaN"""
    from brats21_amd import _lib, ops
    lib = _lib.lib()
    n, k = t.shape[:2]
    vox = t[0, 0].numel()
    ws = torch.full((lib.brats_dice_multi_ws_floats(len(heads), n, k),), NAN, device=t.device)
    assert ws.numel() == len(heads) * lib.brats_dice_ws_floats(n, k)
    _lib.check(lib.brats_dice_stats_multi(_ptrs(heads), len(heads), t.data_ptr(), ws.data_ptr(), n, k, vox, ops._stream()), "dice_stats_multi")
    return ws.view(len(heads), -1)


def _finish(ws, nh, n, k, vox, jaccard, eps=1e-5):
    """-> sums [H][K][3], coef [H][K][2], loss; all start as NaN"""
    from brats21_amd import _lib, ops
    sums = torch.full((nh, k, 3), NAN, device=ws.device)
    coef = torch.full((nh, k, 2), NAN, device=ws.device)
    loss = torch.full((), NAN, device=ws.device)
    _lib.check(_lib.lib().brats_dice_finish(ws.data_ptr(), nh, n, k, vox, eps, int(jaccard), sums.data_ptr(), coef.data_ptr(),
                                            loss.data_ptr(), ops._stream()), "dice_finish")
    return sums, coef, loss


def _stats_one(x, t):
    from brats21_amd import _lib, ops
    lib = _lib.lib()
    n, k = x.shape[:2]
    sums = torch.full((k, 3), NAN, device=x.device)
    ws = torch.full((lib.brats_dice_ws_floats(n, k),), NAN, device=x.device)
    _lib.check(lib.brats_dice_stats(x.data_ptr(), t.data_ptr(), sums.data_ptr(), ws.data_ptr(), n, k, x[0, 0].numel(), ops._stream()), "dice_stats")
    return sums, ws


def _grad_one(x, t, coef):
    from brats21_amd import _lib, ops
    n, k = x.shape[:2]
    dx = torch.full_like(x, NAN)
    _lib.check(_lib.lib().brats_dice_grad(x.data_ptr(), t.data_ptr(), coef.data_ptr(), dx.data_ptr(), n, k, x[0, 0].numel(), ops._stream()), "dice_grad")
    return dx


def _grad_multi(heads, t, coef, g, outs=None):
    from brats21_amd import _lib, ops
    n, k = t.shape[:2]
    outs = [torch.full_like(h, NAN) for h in heads] if outs is None else outs
    _lib.check(_lib.lib().brats_dice_grad_multi(_ptrs(heads), len(heads), t.data_ptr(), coef.data_ptr(), g.data_ptr(), _ptrs(outs), n, k,
                                                t[0, 0].numel(), ops._stream()), "dice_grad_multi")
    return outs


def _torch_algebra(sums, jaccard, eps=1e-5):
    """The [heads][classes] algebra of _FusedDiceFn.forward as it ran in torch before brats_dice_finish -> (coef, loss)."""
    inter, p2, t2 = sums[..., 0], sums[..., 1], sums[..., 2]
    hk = float(sums.shape[0] * sums.shape[1])
    if jaccard:
        den = 2.0 * (t2 + p2 - inter)
        f = 1.0 - (2.0 * inter + eps) / (den + eps)
        dden = (2.0 * inter + eps) / (den + eps) ** 2
        coef = torch.stack([(-2.0 / (den + eps) - 2.0 * dden) / hk, 2.0 * dden / hk], -1)
    else:
        den = t2 + p2
        f = 1.0 - (2.0 * inter + eps) / (den + eps)
        coef = torch.stack([-2.0 / (den + eps) / hk, (2.0 * inter + eps) / (den + eps) ** 2 / hk], -1)
    return coef.contiguous(), f.mean()


def _assert_one_ulp(name, got, ref):
    lo, hi = torch.nextafter(ref, torch.full_like(ref, -float("inf"))), torch.nextafter(ref, torch.full_like(ref, float("inf")))
    print(f"  {name}: loss {float(got):.9g} vs torch's mean {float(ref):.9g}: {'equal' if torch.equal(got, ref) else 'one ulp apart' if bool((got >= lo) & (got <= hi)) else 'FURTHER APART'}")
    assert bool((got >= lo) & (got <= hi)), (name, float(got), float(ref))


SMALL = {"scalar_210": (5, 6, 7), "two_blocks_7680": (8, 24, 40)}
CASES = {f"{s}-H{h}-K{k}": (h, 2, k, SMALL[s], None) for s in SMALL for h in (1, 5, 6) for k in (1, 3)}
CASES["cap_exact_128cube"] = (5, 1, 1, (128, 128, 128), None)
CASES["cap_exceeded"] = (2, 1, 1, (208, 208, 200), None)
CASES["one_head_off_alignment"] = (5, 2, 3, (8, 24, 40), 3)


@pytest.mark.parametrize("case", list(CASES))
def test_multi_entries_match_per_head_entries(case):
    """Statistics (every per-block partial, every total), coefficients (plain and Jaccard), loss and gradients (g = 1 and
    g = 65536) of the three all-heads entries against the per-head entries and the torch algebra between them."""
    nh, n, k, shape, off = CASES[case]
    vox = shape[0] * shape[1] * shape[2]
    gx = _gx(vox, 512)
    if case.startswith("scalar"):
        assert vox % 4 and gx == 1
    if case.startswith("two_blocks"):
        assert vox % 4 == 0 and gx == 2
    if case == "cap_exact_128cube":
        assert (vox // 4 + 255) // 256 // 4 == 512
    if case == "cap_exceeded":
        assert (vox // 4 + 255) // 256 // 4 > 2048
    heads, t = _inputs(400 + len(case), nh, n, k, shape, off)
    # with one head off alignment every head goes through the scalar loop: the reference gets each head at such an address
    ref_heads = heads if off is None else [_offset_copy(h, 1) for h in heads]
    if off is not None:
        assert heads[off].data_ptr() % 16 == 4 and all(h.data_ptr() % 16 == 0 for i, h in enumerate(heads) if i != off)
    ws = _stats_multi(heads, t)
    used = n * gx * k * 3
    ref_sums = []
    for h in range(nh):
        s1, w1 = _stats_one(ref_heads[h], t)
        assert bool(torch.isfinite(w1[:used]).all()) and torch.equal(ws[h, :used], w1[:used]), f"{case}: partials of head {h} differ"
        assert bool(torch.isnan(ws[h, used:]).all()), f"{case}: head {h} wrote past its {n * gx} partial vectors"
        ref_sums.append(s1)
    ref_sums = torch.stack(ref_sums)
    for jaccard in (False, True):
        sums, coef, loss = _finish(ws, nh, n, k, vox, jaccard)
        assert torch.equal(sums, ref_sums), f"{case}: totals differ"
        ref_coef, ref_loss = _torch_algebra(ref_sums, jaccard)
        assert torch.equal(coef, ref_coef), (case, jaccard, coef, ref_coef)
        _assert_one_ulp(f"{case} jaccard={jaccard}", loss, ref_loss)
        if jaccard and vox > 10 ** 6:
            continue  # (the gradient kernels do not know about jaccard: one pass over the large shapes is enough)
        for gval in (1.0, 65536.0):
            g = torch.tensor(gval, device=_dev())
            outs = _grad_multi(heads, t, coef, g)
            scaled = (ref_coef * g).contiguous()
            for h in range(nh):
                want = _grad_one(ref_heads[h], t, scaled[h])
                assert bool(torch.isfinite(want).all()) and torch.equal(outs[h], want), f"{case}: gradient of head {h} differs (g = {gval})"


@pytest.mark.parametrize("jaccard", [False, True])
def test_finisher_with_empty_classes(jaccard):
    """Sums of exactly 0 (an empty class whose prediction underflowed as well): only eps keeps the quotients finite; and
    classes with an empty target only.  The partial vectors are written by hand: 300 of them, so that every slice of the ordered
    sum runs its eight-in-flight loop once and the first 44 slices the remainder loop as well."""
    from brats21_amd import _lib
    nh, n, k, vox = 5, 1, 3, 300 * 4096
    gx = _gx(vox, 512)
    assert gx == 300
    per = _lib.lib().brats_dice_ws_floats(n, k)
    ws = torch.full((nh, per), NAN, device=_dev())
    part = torch.rand((nh, gx, k, 3), generator=_gen(7), device=_dev()) * 100.0
    part[0, :, 0, :] = 0.0          # head 0, class 0: all three sums 0
    part[1, :, 1, 0] = 0.0          # no overlap
    part[1, :, 1, 2] = 0.0          # ... because the target is empty
    part[2, :, 2, 1] = 0.0          # prediction underflowed
    ws[:, :gx * k * 3] = part.reshape(nh, -1)
    sums, coef, loss = _finish(ws.reshape(-1), nh, n, k, vox, jaccard)
    # the ordered sum in torch: 32 slices (block b to slice b % 32, blocks in order), then the slices in order
    acc = torch.zeros((32, nh, k, 3), device=_dev())
    for b in range(gx):
        acc[b % 32] += part[:, b]
    tot = acc[0].clone()
    for s in range(1, 32):
        tot += acc[s]
    assert torch.equal(sums, tot)
    assert float(sums[0, 0].abs().max()) == 0.0
    ref_coef, ref_loss = _torch_algebra(sums, jaccard)
    assert bool(torch.isfinite(coef).all()) and bool(torch.isfinite(loss))
    assert torch.equal(coef, ref_coef), (coef, ref_coef)
    _assert_one_ulp(f"empty classes jaccard={jaccard}", loss, ref_loss)


def test_multi_gradient_at_extreme_logits():
    """+-30, +-inf and 0 logits on the ragged plane (210 voxels), g = 1 and 65536: equal to the per-head kernel, and finite."""
    nh, n, k, shape = 5, 2, 3, (5, 6, 7)
    heads, t = _inputs(77, nh, n, k, shape)
    vals = torch.tensor([30.0, -30.0, float("inf"), -float("inf"), 0.0], device=_dev())
    for i, h in enumerate(heads):
        flat = h.view(-1)
        flat[i::7] = vals[(torch.arange(flat[i::7].numel(), device=_dev()) + i) % 5]
    ws = _stats_multi(heads, t)
    used = n * k * 3
    for h in range(nh):
        s1, w1 = _stats_one(heads[h], t)
        assert bool(torch.isfinite(w1[:used]).all()) and torch.equal(ws[h, :used], w1[:used])
    sums, coef, _ = _finish(ws, nh, n, k, 210, False)
    assert torch.equal(coef, _torch_algebra(sums, False)[0])
    for gval in (1.0, 65536.0):
        g = torch.tensor(gval, device=_dev())
        outs = _grad_multi(heads, t, coef, g)
        scaled = (coef * g).contiguous()
        for h in range(nh):
            want = _grad_one(heads[h], t, scaled[h])
            assert bool(torch.isfinite(outs[h]).all()) and torch.equal(outs[h], want), (h, gval)


def _dice_torch(x, t, jaccard, eps=1e-5):
    p = torch.sigmoid(x)
    ax = (0, 2, 3, 4)
    inter = (t * p).sum(ax)
    den = (t * t).sum(ax) + (p * p).sum(ax)
    if jaccard:
        den = 2.0 * (den - inter)
    return (1.0 - (2.0 * inter + eps) / (den + eps)).mean()


def _forbid(monkeypatch, names):
    from brats21_amd import _lib
    for name in names:
        def fail(*a, _n=name, **kw):
            raise AssertionError(f"{_n} was called on the wrong path")
        monkeypatch.setattr(_lib.lib(), name, fail)


@pytest.mark.parametrize("jaccard", [False, True])
@pytest.mark.parametrize("route", ["multi", "fallback"])
@pytest.mark.parametrize("shape", [(5, 7, 9), (11, 13, 53)])
def test_fused_deep_supervision_dice(shape, route, jaccard, monkeypatch):
    """fused_deep_supervision_dice over five heads against DiceLoss per head in f64 (autograd), through the three all-heads
    entries (every head contiguous f32 of the target's shape) and, with one head handed in as a strided view (every second
    element of a wider buffer), through the per-head path; each route must not touch the other's entries."""
    from brats21_amd import losses
    n, k = 2, 3
    heads, target = _inputs(510, 5, n, k, shape)
    if route == "fallback":
        wide = torch.full((n, k, shape[0], shape[1], shape[2] * 2), NAN, device=_dev())
        wide[..., ::2] = heads[2]
        heads[2] = wide[..., ::2]
        assert not heads[2].is_contiguous()
        _forbid(monkeypatch, ["brats_dice_stats_multi", "brats_dice_finish", "brats_dice_grad_multi"])
    else:
        _forbid(monkeypatch, ["brats_dice_stats", "brats_dice_grad"])
    xs = [h.detach().requires_grad_(True) for h in heads]
    loss = losses.fused_deep_supervision_dice((xs[0], xs[1:]), target, jaccard=jaccard)
    grads = torch.autograd.grad(loss, xs)
    x64 = [h.detach().double().requires_grad_(True) for h in heads]
    ref = torch.stack([_dice_torch(h, target.double(), jaccard) for h in x64]).mean()
    g64 = torch.autograd.grad(ref, x64)
    f32 = torch.stack([_dice_torch(h.detach(), target, jaccard) for h in heads]).mean()
    f64 = float(ref)
    ref_err = abs(float(f32.double()) - f64) / abs(f64)
    bar = max(4.0 * ref_err, 1e-6)
    err = abs(float(loss.double()) - f64) / abs(f64)
    print(f"  loss {shape} {route} jaccard={jaccard}: {float(loss):.8f} vs float64 {f64:.10f}: relative error {err:.2e} / bar {bar:.2e}")
    assert err <= bar, (err, bar)
    for g, w in zip(grads, g64):
        torch.testing.assert_close(g, w.float(), rtol=1e-4, atol=1e-9)


def test_graphed_step_replays_to_the_eager_loss():
    """The training step of a width-8 model at 32^3 with the fused Dice: captured into a graph (the head pointers are kernel
    arguments, nothing is uploaded per step) it gives the losses of the same steps run eagerly.  Both use the capturable
    optimizer, so both run the same kernels on the same values: the losses are equal."""
    from brats21_amd import get_model
    from brats21_amd.engine import GraphedTrainStep, TrainStep
    from brats21_amd.optim import Ranger2020
    from oracle import synth
    ns = argparse.Namespace(model="equiunet", width=8, norm="group", act="relu", num_classes=3, dropout=0)
    xs = [synth.random_image(1, 4, (32, 32, 32), seed=40 + i).to(_dev()) for i in range(3)]
    t = synth.nested_spheres(1, (32, 32, 32)).to(_dev())
    results = []
    for graphed in (False, True):
        torch.manual_seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            m = get_model(ns).to(_dev()).train()
        opt = Ranger2020(m.parameters(), lr=1e-2, weight_decay=1e-5, use_gc=True, capturable=True)
        step = TrainStep(m, opt, amp=True, amp_dtype=BF)
        assert step.fused
        if graphed:
            step = GraphedTrainStep(step, warmup=2)
            losses = [float(step(xs[0], t).detach())]  # two eager warm-ups + capture + one replay: steps 1..3 on xs[0]
        else:
            losses = [float(step(xs[0], t).detach()) for _ in range(3)][2:]
        losses += [float(step(x, t).detach()) for x in xs[1:]]
        torch.cuda.synchronize()
        results.append(losses)
    print(f"  eager {results[0]} graphed {results[1]}")
    assert results[0] == results[1]


@pytest.mark.parametrize("dtype", [BF, HF, F32], ids=["bf16", "fp16", "f32"])
@pytest.mark.parametrize("coarse", [(3, 4, 5), (8, 8, 16)])
@pytest.mark.parametrize("c", [8, 48])
def test_upsample_bwd_with_addend(c, coarse, dtype):
    """ops.upsample_bwd(dy, add=a) against ops.upsample_bwd(dy) + a, bit for bit; the addend and the output are channel slices
    of NaN-filled buffers, whose other channels must stay NaN.  (8 x 8 x 16 with 48 channels in 16 bits is the one-launch
    tile form, everything else the three passes.)"""
    from brats21_amd import ops
    n, (d, h, w), off = 2, coarse, 8
    g = _gen(900 + c + d)
    dy = torch.randn((n, 2 * d, 2 * h, 2 * w, c), generator=g, device=_dev()).to(dtype)
    abuf = torch.full((n, d, h, w, c + 2 * off), NAN, device=_dev(), dtype=dtype)
    obuf = torch.full((n, d, h, w, c + 3 * off), NAN, device=_dev(), dtype=dtype)
    add = abuf[..., off:off + c]
    add.copy_(torch.randn((n, d, h, w, c), generator=g, device=_dev()).mul_(4.0).to(dtype))
    want = ops.upsample_bwd(dy, 2) + add
    out = obuf[..., 2 * off:2 * off + c]
    got = ops.upsample_bwd(dy, 2, add=add, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert bool(torch.isfinite(want.float()).all()) and torch.equal(got, want)
    assert bool(torch.isnan(obuf[..., :2 * off]).all()) and bool(torch.isnan(obuf[..., 2 * off + c:]).all()), "written outside the slice"
    assert torch.equal(ops.upsample_bwd(dy, 2, add=add), want)  # a dense output tensor
