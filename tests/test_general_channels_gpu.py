"""-m gpu: brats_head_fwd / brats_head_bwd with 5 to 16 classes (csrc/head.hip: the class tiles of the plain kernels, all sixteen
accumulator rows of the MFMA form, the class-tiled backward) and the two networks with input-channel and class counts other
than BraTS' (4, 3).

Head values follow the derived rules of tests/test_loss_end_gpu.py, imported from there: _check_logits (the sum rule over C + 1
terms), _check_bwd (the element rule for dx, the sum rule for dw / db), inputs from _head_inputs, results and workspace NaN
before every call.  Shapes are the smallest that reach each path; every case that is there for a launch geometry asserts it.

Up-sampled heads (scale 2, 4, 8).  Forward: plane k of the K-class call against the one-class call on row k of the weights --
the K <= 4 path, which the wide forms leave as it was.  Both up-sample low-resolution logits that each obey the sum rule, with
interpolation weights that are non-negative and sum to 1 (the low-resolution errors pass through undiminished at most), so the
bound is 2 x (the largest sum-rule bound of the plane's low-resolution logits) + 2^-21 max|logit| for the lerp roundings.
Backward: against float64, the low-resolution gradient taken by autograd through F.interpolate(trilinear, align_corners=True)
in double; dout is positive, so that adjoint is also the adjoint of |dout| that _check_bwd's bounds want.  The rules of
_check_bwd carry no term for the f32 rounding of the adjoint pass itself (a sum of up to (2 s - 1)^3 non-negative terms per
low-resolution voxel); it disappears below the storage rounding of a 16-bit dx, so the scaled backward runs in bf16 and fp16.
The scaled f32 backward with K > 4 is covered by the deep heads of the f32 networks below.

Networks: the f32 mode against the fixtures of tests/golden/make_golden_general.py at the bars of
tests/test_equiunet_gpu.py::test_equiunet_f32_matches_reference_golden; the reference itself is within 5e-5 (logits) and 2e-5
relative (gradients) of float64 on these cases (recorded in the fixtures as ref_err_*).
"""
import contextlib
import io
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _general_cases as G
from oracle import synth, unet
from test_loss_end_gpu import (BF, F32, HF, NAN, ODD, _check_bwd, _check_logits, _dev, _head_bwd, _head_fwd, _head_inputs)

pytestmark = pytest.mark.gpu
LOGIT_ATOL = 1e-3


@pytest.fixture(autouse=True)
def _release():
    yield
    torch.cuda.empty_cache()


def _name(dt):
    return str(dt)[6:]


# =====================================================================================================================
# A. Heads at scale 1
# =====================================================================================================================
SMALL = (6, 7, 9)   # 378 voxels: no multiple of 16
HEAD_CASES = (
    [(f"k{k}", dt, 16, 1, k, SMALL, 0.2, k != 6) for k in (5, 6, 7, 16) for dt in (BF, HF, F32)]       # K = 6 without a bias
    + [("odd_trips", dt, 48, 2, 16, ODD, 0.2, True) for dt in (BF, HF, F32)]                           # the MFMA form (16-bit)
    + [("wide13", dt, 96, 2, 13, (8, 10, 12), 0.2, True) for dt in (BF, HF)]                           # C > 64: the plain 16-bit kernel
    + [("lds", dt, 384, 1, 16, (4, 4, 4), 0.2, True) for dt in (BF, HF)]                               # ... with its largest LDS carve
    + [("small_weights", dt, 48, 2, 16, ODD, 2.0 ** -9, True) for dt in (HF, BF)]                      # the three-term split, new rows
)


def _class_tile(k):
    return 4 if k <= 4 else (8 if k <= 8 else 16)


def _bwd_geometry(dtype, c, k, vox):
    """csrc/head.hip brats_head_bwd: channels per thread (8 bytes of a 16-bit tensor at the class tiles 8 and 16), voxels per
    block trip, blocks per sample"""
    vw = 4 if (dtype == F32 or _class_tile(k) > 4) else 8
    vl = 256 // (c // vw)
    return vw, vl, min(max(-(-vox // (vl * 16)), 1), 1024)


@pytest.mark.parametrize("name,dtype,c,n,k,shape,wstd,bias", HEAD_CASES, ids=[f"{c[0]}-{_name(c[1])}" for c in HEAD_CASES])
def test_head_values(name, dtype, c, n, k, shape, wstd, bias):
    """brats_head_fwd / brats_head_bwd against f64.  k5 .. k16: the class tiles 8 and 16 and their K guards; odd_trips: the MFMA
    forward's 21 waves on gx = 5 blocks (one wave takes a second trip, the last chunk is ragged) now storing sixteen rows, the
    16-class backward's one-voxel loop over 4 blocks of 21 voxel lanes (four idle threads); wide13 / lds: the plain 16-bit
    kernel at C = 96 and at K x C = 16 x 384 (40 KB of LDS); small_weights: weights of N(0, 1) * 2^-9."""
    vox = shape[0] * shape[1] * shape[2]
    if name == "odd_trips":
        vw, vl, gx = _bwd_geometry(dtype, c, k, vox)
        assert (vw, vl, gx) == (4, 21, 4) and 256 - vl * (c // vw) == 4
        trips = [len(range(blk * vl + lane, vox, gx * vl)) for blk in range(gx) for lane in range(vl)]
        assert min(trips) >= 2 and len(set(trips)) == 2, "every thread loops, and not all equally often"
        assert -(-vox // 64) == 21 and max(-(-vox // 64) // 4, 1) == 5 and vox % 16
    if name == "lds":
        assert (_class_tile(k) * c + 256 * _class_tile(k)) * 4 == 40960
        vw, vl, gx = _bwd_geometry(dtype, c, k, vox)
        assert (vw, vl, gx) == (4, 2, 2) and (k * c + vl * 4 * c + vl * 4) * 4 < 65536
    x, w, b, dout = _head_inputs(500 + c + k, dtype, c, n, k, shape, wstd, bias)
    tag = f"{name} {_name(dtype)}"
    _check_logits(f"logits {tag}", _head_fwd(x, w, b), x, w, b)
    dx = torch.full_like(x, NAN)
    dw, db = _head_bwd(x, w, dout, dx)
    _check_bwd(tag, dtype, x, w, dout, dx, dw, db)


@pytest.mark.parametrize("dtype,c", [(BF, 48), (HF, 48), (F32, 48), (BF, 96)], ids=["bfloat16", "float16", "float32", "bfloat16-c96"])
def test_head_exact_count(dtype, c):
    """x = 1, dout = 1, K = 16: every partial is an integer below 2^24, so db == dw == N * V exactly; a dropped or doubled
    voxel, class row or partial slot cannot hide."""
    n, k, shape = 2, 16, ODD
    vox = shape[0] * shape[1] * shape[2]
    x, w, b, dout = _head_inputs(520, dtype, c, n, k, shape)
    x, dout = torch.ones_like(x), torch.ones_like(dout)
    dw, db = _head_bwd(x, w, dout, None)
    print(f"  exact count {_name(dtype)}: db in [{float(db.min())}, {float(db.max())}] dw in [{float(dw.min())}, {float(dw.max())}] want {n * vox}")
    assert bool((db == n * vox).all()) and bool((dw == n * vox).all())
    # the logits of x = 1 are the same at every voxel
    logits = _head_fwd(x, w, b)
    assert bool((logits == logits[:1, :, :1, :1, :1]).all())


@pytest.mark.parametrize("dtype", [BF, HF, F32], ids=_name)
def test_head_leaves_the_sixth_plane_alone(dtype):
    """K = 5 in buffers allocated for six classes, everything NaN before the call: the logits' plane 5, dw's row 5 and db[5]
    are still NaN afterwards, everything below is finite (and right)."""
    from brats21_amd import _lib, ops
    lib = _lib.lib()
    c, n, k, shape = 16, 1, 5, SMALL
    x, w, b, dout = _head_inputs(530, dtype, c, n, k, shape)
    ptr, _, p = ops._desc(x)
    out = torch.full((n, k + 1, *shape), NAN, device=x.device)
    _lib.check(lib.brats_head_fwd(ptr, p, w.data_ptr(), b.data_ptr(), None, out.data_ptr(), ops._code(dtype), n, c, k, *shape, 1,
                                  ops._stream()), "head_fwd")
    assert bool(torch.isnan(out[:, k]).all()), "the forward wrote a sixth plane"
    _check_logits(f"logits poisoned {_name(dtype)}", out[:, :k].contiguous(), x, w, b)
    ws = torch.full((lib.brats_head_bwd_ws_bytes(n, c, k, *shape, 1) // 4,), NAN, device=x.device)
    dw = torch.full((k + 1, c), NAN, device=x.device)
    db = torch.full((k + 1,), NAN, device=x.device)
    dx = torch.full_like(x, NAN)
    _lib.check(lib.brats_head_bwd(ptr, p, w.data_ptr(), dout.data_ptr(), ws.data_ptr(), dx.data_ptr(), c, dw.data_ptr(), db.data_ptr(),
                                  ops._code(dtype), n, c, k, *shape, 1, ops._stream()), "head_bwd")
    assert bool(torch.isnan(dw[k]).all()) and bool(torch.isnan(db[k])), "the backward wrote a sixth class"
    _check_bwd(f"poisoned {_name(dtype)}", dtype, x, w, dout, dx, dw[:k], db[:k])


# =====================================================================================================================
# B. Up-sampled heads
# =====================================================================================================================
LOW = (3, 5, 6)


@pytest.mark.parametrize("dtype", [BF, F32], ids=_name)
@pytest.mark.parametrize("k", [5, 16])
@pytest.mark.parametrize("scale", [2, 4, 8])
def test_scaled_head_forward_matches_the_one_class_path(scale, k, dtype):
    from brats21_amd import ops
    c, n = 16, 2
    x, w, b, _ = _head_inputs(540 + k, dtype, c, n, k, LOW)
    out = ops.head(x, w.view(k, c, 1, 1, 1), b, scale)
    assert out.shape == (n, k, *(s * scale for s in LOW)) and bool(torch.isfinite(out).all())
    m = (x.double().reshape(n, -1, c).abs() @ w.double().abs().t()) + b.double().abs()       # [n, voxels, k]
    low_bound = m.amax((0, 1)) * (2.0 ** -24 * math.sqrt(c + 1))
    worst = 0.0
    for i in range(k):
        one = ops.head(x, w[i:i + 1].view(1, c, 1, 1, 1), b[i:i + 1], scale)[:, 0]
        bound = 2.0 * float(low_bound[i]) + 2.0 ** -21 * float(one.abs().max())
        worst = max(worst, float((out[:, i] - one).abs().max()) / bound)
    print(f"  scaled forward x{scale} K={k} {_name(dtype)}: worst |K-class - one-class| / bound = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("dtype", [BF, HF], ids=_name)
@pytest.mark.parametrize("k", [5, 16])
@pytest.mark.parametrize("scale", [2, 4, 8])
def test_scaled_head_backward(scale, k, dtype):
    from brats21_amd import ops
    c, n = 16, 2
    x, w, _, _ = _head_inputs(560 + k, dtype, c, n, k, LOW)
    full = tuple(s * scale for s in LOW)
    dout = torch.randn((n, k, *full), generator=torch.Generator(device=_dev()).manual_seed(570 + scale), device=_dev()).abs_().add_(0.5)
    low = torch.zeros((n, k, *LOW), dtype=torch.float64, device=_dev(), requires_grad=True)
    up = F.interpolate(low, size=full, mode="trilinear", align_corners=True)
    g_low, = torch.autograd.grad(up, low, dout.double())   # the adjoint of dout (positive: also that of |dout|)
    dx, dw, db = ops.head_bwd(x, w.view(k, c, 1, 1, 1), dout, scale)
    _check_bwd(f"x{scale} K={k} {_name(dtype)}", dtype, x, w, g_low, dx, dw.view(k, c), db)


# =====================================================================================================================
# C. Networks
# =====================================================================================================================
def _golden(golden_dir, case):
    return np.load(os.path.join(golden_dir, G.fname(case)), allow_pickle=False)


@pytest.mark.parametrize("case", G.CASES, ids=G.IDS)
def test_f32_matches_reference_golden(golden_dir, case):
    g = _golden(golden_dir, case)
    k = case[3]
    m = G.build(case).cuda().train()
    x, t = G.image(case).cuda(), G.nested_targets(1, k).cuda()
    out, deeps = m(x)
    nd = 4 if case[0] == "equiunet" else 2
    assert out.shape == (1, k, *G.SIZE) and len(deeps) == nd and all(d.shape == out.shape for d in deeps)
    err = np.abs(out.detach().cpu().numpy() - g["logits"]).max()
    print(f"  {G.fname(case)}: logit max abs err {err:.2e} (the reference's own against f64: {float(g['ref_err_logits']):.2e})")
    assert err < LOGIT_ATOL, f"logit max abs err {err}"
    for i, d in enumerate(deeps):
        e = np.abs(d.detach().cpu().numpy()[:, :, ::2, ::2, ::2] - g[f"deep{i}"]).max()
        assert e < LOGIT_ATOL, f"deep head {i} max abs err {e}"
    loss = unet.deep_supervision_loss((out, deeps), t)
    print(f"  loss {loss.item():.7f} golden {float(g['loss']):.7f}")
    assert abs(loss.item() - float(g["loss"])) < 1e-4
    loss.backward()
    names = json.loads(str(g["grad_names"]))
    params = dict(m.named_parameters())
    first = names[0]
    assert params[first].grad.shape[1] == case[2], "the first layer's weight gradient has the real input channels"
    norms = np.array([float(params[n].grad.double().norm()) for n in names])
    print(f"  gradient norms: worst relative deviation {np.abs(norms / g['grad_norms'] - 1).max():.2e}")
    np.testing.assert_allclose(norms, g["grad_norms"], rtol=2e-3, atol=1e-7)
    for key in g.files:
        if key.startswith("grad:"):
            ref = g[key]
            np.testing.assert_allclose(params[key[5:]].grad.cpu().numpy(), ref, atol=2e-3 * max(np.abs(ref).max(), 1e-6), rtol=2e-3)


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_16bit_deviation_is_that_of_the_brats_shape(golden_dir, precision):
    """The (1, 5) EquiUnet in a 16-bit mode deviates from its f32 golden by at most twice what the (4, 3) network of the same
    width and size does from its own (mean absolute logit deviation; the maximum is printed beside it).  The (4, 3) network is
    the parent's behaviour, not code under test; twice allows for the different logit distribution of five classes."""
    devs = {}
    for case in (G.CASES[0], G.BRATS_CASE):
        g = _golden(golden_dir, case)
        m = G.build(case).cuda().eval()
        m.precision = precision
        with torch.no_grad():
            out, _ = m(G.image(case).cuda())
        err = (out.cpu() - torch.from_numpy(g["logits"])).abs()
        devs[case] = (float(err.mean()), float(err.max()))
        print(f"  {precision} (inplanes, classes) = {case[2:]}: mean |logit deviation| {devs[case][0]:.4e}, max {devs[case][1]:.4e}")
    assert devs[G.CASES[0]][0] <= 2.0 * devs[G.BRATS_CASE][0], devs


def _train_run(case, graphed, steps=3):
    """`steps` recorded steps of TrainStep (bf16 autocast, fused Dice, Ranger2020) on a batch of two after two unrecorded ones
    (the warm-up steps of the graphed form) -> (losses, parameters)"""
    from brats21_amd.engine import GraphedTrainStep, TrainStep
    from brats21_amd.optim import Ranger2020
    dev = _dev()
    x = synth.random_image(2, case[2], G.SIZE, seed=40 + case[2]).to(dev)
    t = G.nested_targets(2, case[3]).to(dev)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        m = G.build(case, load=False)
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


@pytest.mark.parametrize("case,parent", [(G.CASES[0], G.BRATS_CASE), (G.CASES[4], ("assp", 16, 4, 3))], ids=[G.IDS[0], G.IDS[4]])
def test_training_steps_are_reproducible_and_capture(case, parent):
    """Three TrainStep steps with Ranger2020, run twice from the same state, give bit-identical losses and weights; captured
    into a hipGraph and replayed, the loss sequence stands in the same relation to the eager one -- bit-equal or not -- as that
    of the (4, 3) network of the same kind does, and is close to it either way."""
    l0, p0 = _train_run(case, False)
    l1, p1 = _train_run(case, False)
    assert bool(torch.isfinite(l0).all()) and torch.equal(l0, l1), (l0, l1)
    assert all(torch.equal(a, b) for a, b in zip(p0, p1)), "two eager runs from the same state end at different weights"
    lg, pg = _train_run(case, True)
    np.testing.assert_allclose(lg.numpy(), l0.numpy(), rtol=1e-5, atol=1e-6)  # (the bar of tests/test_optim_gpu.py)
    le_p, _ = _train_run(parent, False)
    lg_p, _ = _train_run(parent, True)
    print(f"  {case[0]} {case[2:]}: eager {l0.tolist()} graphed {lg.tolist()} bit-equal {torch.equal(l0, lg)}; "
          f"(4, 3): eager {le_p.tolist()} graphed {lg_p.tolist()} bit-equal {torch.equal(le_p, lg_p)}")
    assert torch.equal(l0, lg) == torch.equal(le_p, lg_p)


def test_sliding_window_with_two_channels_and_five_classes():
    """A two-channel 24 x 16 x 16 volume, roi 16^3, overlap 0.5, constant blend, a (2, 5) EquiUnet in f32, against the same model
    run window by window and averaged in torch."""
    from brats21_amd.inferers import sliding_window_inference
    case = ("equiunet", 8, 2, 5)
    m = G.build(case, deep_supervision=False).cuda().eval()
    x = synth.closed_form_image(1, 2, (24, 16, 16)).cuda()
    with torch.no_grad():
        got = sliding_window_inference(x, (16, 16, 16), 1, m, overlap=0.5, mode="constant")
        acc = torch.zeros((1, 5, 24, 16, 16), device=x.device)
        cnt = torch.zeros_like(acc)
        for z0 in (0, 8):
            acc[:, :, z0:z0 + 16] += m(x[:, :, z0:z0 + 16].contiguous())
            cnt[:, :, z0:z0 + 16] += 1.0
    want = acc / cnt
    assert got.shape == want.shape and bool(torch.isfinite(got).all())
    tol = 1e-6 * float(want.abs().max())
    err = float((got - want).abs().max())
    print(f"  sliding window (2, 5): max |got - want| {err:.2e} / {tol:.2e}")
    assert err <= tol
