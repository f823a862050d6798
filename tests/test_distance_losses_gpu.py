"""GPU tests of the distance transform (csrc/edt.hip) and the hd / dice_hd / boundary / dice_boundary criteria
(csrc/dist_loss.hip, brats21_amd/losses.py) against tests/golden/losses*.npz -- the reference's own classes over real scipy --
and against the scipy-free brute-force restatement tests/_losses_ref.py (run on the GPU here, pinned to the goldens by
tests/test_distance_losses_cpu.py).

Bars.  Fields: bit-equal f32.  Gradients: rtol 1e-4, atol 1e-9, the bar of the fused Dice (tests/test_ops_gpu.py).  Loss
value against the float64 evaluation: 4 x the reference's own f32-CPU error on the same case (stored with the golden), not
below 1e-6 relative -- the margin is for the different summation order and __expf.

The measured errors are printed by the parity test (pytest -s) and carried in its assertion messages.
"""
import argparse
import contextlib
import io

import numpy as np
import pytest
import torch

import _losses_ref as R
from test_distance_losses_cpu import CRITERIA, check_factory, field_case, golden_grads, load_goldens, loss_cases, loss_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def goldens(golden_dir):
    return load_goldens(golden_dir)


def bits(t):
    return t.detach().float().cpu().numpy().view(np.uint32)


def assert_bit_equal(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.argwhere(g != w)
    assert bad.size == 0, (f"{what}: {len(bad)} of {g.size} values differ, first at {bad[0].tolist()}: "
                           f"{float(got.detach().cpu().numpy()[tuple(bad[0])])} vs {float(want.detach().cpu().numpy()[tuple(bad[0])])}")


def test_field_is_bit_equal_to_the_goldens(goldens):
    from brats21_amd import ops, transforms
    for name in goldens["field_cases"]:
        m = field_case(goldens, name).to(DEV)
        want = {k: torch.from_numpy(goldens[f"field_{name}__{k}"].astype(np.float32)) for k in ("hd_dist", "hd_dist_int", "dist_map")}
        for kind, mask in (("f32", m.float()), ("u8", m.to(torch.uint8)), ("bool", m), ("f32 values", m.float() * -2.5)):
            assert_bit_equal(ops.distance_transform_edt(mask), want["hd_dist"], f"{name} {kind} mode 0")
            assert_bit_equal(ops.distance_transform_edt(mask, mode=2), want["hd_dist_int"], f"{name} {kind} mode 2")
            assert_bit_equal(ops.distance_transform_edt(mask, mode=1), want["dist_map"], f"{name} {kind} mode 1")
        assert_bit_equal(transforms.one_hot_to_dist(m.float()), want["dist_map"], f"{name} one_hot_to_dist [K, D, H, W]")
        assert_bit_equal(transforms.one_hot_to_dist(m.float()[None])[0], want["dist_map"], f"{name} one_hot_to_dist [N, K, D, H, W]")


def seeded_volumes():
    """Shapes where the kernels can go wrong: W over one and over two waves with a ragged last chunk, line counts (H*W, D*W)
    that are no multiple of the block, single rows / columns, and a batch that mixes empty, full and ordinary planes."""
    g = torch.Generator().manual_seed(20211017)
    out = {}
    for shape in ((9, 37, 70), (40, 6, 130), (1, 1, 65), (17, 1, 1)):
        dense = torch.rand((1,) + shape, generator=g) < 0.97      # little background: long distances, carries across chunks
        half = torch.rand((1,) + shape, generator=g) < 0.5
        box = torch.zeros((1,) + shape, dtype=torch.bool)
        box[(0,) + tuple(slice(s // 5, s - s // 6) for s in shape)] = True
        out[shape] = torch.cat([dense, half, box])
    mixed = torch.rand((5, 6, 7, 66), generator=g) < 0.9
    mixed[0] = False
    mixed[2] = True
    mixed[3] = False
    mixed[3, 2, 3, 64] = True
    out["mixed batch"] = mixed
    return out


def test_field_is_bit_equal_to_the_brute_force_restatement():
    from brats21_amd import ops
    for name, masks in seeded_volumes().items():
        m = masks.to(DEV)
        seg = m.float()
        assert_bit_equal(ops.distance_transform_edt(seg), R.hd_dist(seg), f"{name} mode 0")
        assert_bit_equal(ops.distance_transform_edt(m.to(torch.uint8), mode=2), R.hd_dist(seg, integer=True), f"{name} mode 2")
        assert_bit_equal(ops.distance_transform_edt(seg, mode=1), R.one_hot_to_dist(seg), f"{name} mode 1")
    full = torch.ones((2, 3, 4, 5), device=DEV)  # no background: scipy's virtual background voxel at (-1, 0, 0)
    z, y, x = torch.meshgrid(torch.arange(3), torch.arange(4), torch.arange(5), indexing="ij")
    want = ((z + 1.0) ** 2 + y ** 2 + x ** 2).double().sqrt().float()
    assert_bit_equal(ops.distance_transform_edt(full)[1], want, "all-one volume")


def test_predicted_one_hot_ties_like_torch(goldens):
    from brats21_amd import losses
    for key in ("loss__tie", "loss__head0"):
        x = torch.from_numpy(goldens[key]).to(DEV)
        got = losses.sigmoid_one_hot(x)
        assert got.dtype == torch.uint8
        assert torch.equal(got.float().cpu(), R.probs_one_hot(x.cpu())), key
    x = torch.full((1, 3, 2, 2, 2), -200.0, device=DEV)  # every probability is 0: still the lowest channel
    assert torch.equal(losses.sigmoid_one_hot(x)[0, :, 0, 0, 0].cpu(), torch.tensor([1, 0, 0], dtype=torch.uint8))


_reference = {}


def reference(goldens, crit, case):
    """float64 value and gradients of the restatement, once per case (brute-force fields on the GPU)."""
    if (crit, case) not in _reference:
        target, dist, cases = loss_inputs(goldens)
        f64, g64 = R.loss_and_grads(crit, [h.to(DEV) for h in cases[case]], target.to(DEV), dist.to(DEV))
        _reference[(crit, case)] = (float(f64), [g.cpu() for g in g64])
    return _reference[(crit, case)]


def run_criterion(crit, heads, target, dist, prepared=True):
    from brats21_amd import definer, losses
    with contextlib.redirect_stdout(io.StringIO()):
        criterion = definer.make_criterion(argparse.Namespace(criterion=crit, num_classes=3))
    label = [target, dist] if "boundary" in crit else target
    xs = [h.to(DEV).requires_grad_(True) for h in heads]
    if len(xs) == 1:
        loss = criterion(xs[0], label)
    else:
        fn = losses.deep_supervision_prepared_loss if prepared else losses.deep_supervision_loss
        loss, main = fn(criterion, (xs[0], xs[1:]), label)
        assert main is xs[0]
    loss.backward()
    return loss.detach(), [x.grad for x in xs]


@pytest.mark.parametrize("crit", CRITERIA)
def test_loss_and_gradient_match_the_goldens_and_float64(goldens, crit):
    target, dist, cases = loss_inputs(goldens)
    target, dist = target.to(DEV), dist.to(DEV)
    report = []
    for case in loss_cases(crit):
        heads = cases[case]
        loss, grads = run_criterion(crit, heads, target, dist)
        f64, g64 = reference(goldens, crit, case)
        assert abs(f64 - float(goldens[f"{crit}__{case}__f64"])) <= 1e-12 * abs(f64)
        ref_err = abs(float(goldens[f"{crit}__{case}__loss"]) - f64) / abs(f64)
        bar = max(4.0 * ref_err, 1e-6)
        err = abs(float(loss.double()) - f64) / abs(f64)
        gerr = max(float((g.cpu().double() - w).abs().max() / w.abs().max()) for g, w in zip(grads, g64))
        report.append(f"{crit} {case}: value {float(loss):.8f} vs float64 {f64:.10f}: rel err {err:.2e} (bar {bar:.2e}, reference's own "
                      f"f32 error {ref_err:.2e}); gradient max err / max {gerr:.2e}")
        print("\n" + report[-1])
        assert err <= bar, report
        for g, w64, wgold in zip(grads, g64, golden_grads(goldens, crit, case, len(heads))):
            assert g.dtype == torch.float32
            torch.testing.assert_close(g.cpu(), w64.float(), rtol=1e-4, atol=1e-9, msg=lambda m: f"{report[-1]}\nagainst float64: {m}")
            torch.testing.assert_close(g.cpu(), wgold, rtol=1e-4, atol=1e-9, msg=lambda m: f"{report[-1]}\nagainst the golden: {m}")


def test_other_dtypes_idc_subset_and_alpha(goldens):
    """Logits of any float dtype are upcast; idc selects channels after the arg-max over all of them; alpha != 2 takes powf."""
    from brats21_amd import losses
    target, dist, cases = loss_inputs(goldens)
    target, dist, x = target.to(DEV), dist.to(DEV), cases["single"][0].to(DEV)
    with contextlib.redirect_stdout(io.StringIO()):
        hd = losses.HausdorffLoss(idc=[0, 1, 2], sigmoid=True, alpha=2)
    xb = x.bfloat16().requires_grad_(True)
    lb = hd(xb, target)
    lb.backward()
    xf = xb.detach().float().requires_grad_(True)
    lf = hd(xf, target)
    lf.backward()
    assert xb.grad.dtype == torch.bfloat16 and torch.equal(lb, lf) and torch.equal(xb.grad, xf.grad.bfloat16())
    # idc = [2, 0], alpha = 1.5 against the restatement in float64
    sub = losses.HausdorffLoss(idc=[2, 0], sigmoid=True, alpha=1.5)
    xs = x.clone().requires_grad_(True)
    ls = sub(xs, target)
    ls.backward()
    x64 = x.double().requires_grad_(True)
    oh = R.probs_one_hot(x)
    tdm = R.batched(R.hd_dist, target)[:, [2, 0]].double()
    pdm = R.batched(lambda s: R.hd_dist(s, integer=True), oh)[:, [2, 0]].double()
    want = ((torch.sigmoid(x64)[:, [2, 0]] - target[:, [2, 0]].double()) ** 2 * (tdm ** 1.5 + pdm ** 1.5)).mean()
    want.backward()
    assert abs(float(ls) - float(want)) <= 1e-6 * abs(float(want)), (float(ls), float(want))
    torch.testing.assert_close(xs.grad, x64.grad.float(), rtol=1e-4, atol=1e-9)
    assert float(xs.grad[:, 1].abs().max()) == 0.0
    bs = losses.SurfaceLoss(idc=[1], sigmoid=True)
    xs = x.clone().requires_grad_(True)
    lbs = bs(xs, [target, dist])
    lbs.backward()
    want = R.boundary_loss(x64[:, [1]], dist[:, [1]])
    assert abs(float(lbs) - float(want)) <= 1e-6 * abs(float(want))


@pytest.mark.parametrize("crit", CRITERIA)
def test_shared_prepared_target_equals_per_head_calls_exactly(goldens, crit):
    target, dist, cases = loss_inputs(goldens)
    target, dist = target.to(DEV), dist.to(DEV)
    la, ga = run_criterion(crit, cases["deep3"], target, dist, prepared=True)
    lb, gb = run_criterion(crit, cases["deep3"], target, dist, prepared=False)
    assert torch.equal(la, lb)
    assert all(torch.equal(a, b) for a, b in zip(ga, gb))
    la2, ga2 = run_criterion(crit, cases["deep3"], target, dist, prepared=True)  # deterministic: no atomics anywhere
    assert torch.equal(la, la2) and all(torch.equal(a, b) for a, b in zip(ga, ga2))


def test_make_criterion(monkeypatch):
    check_factory(monkeypatch)


@pytest.mark.parametrize("crit", ["hd", "dice_boundary"])
def test_graphed_train_step_replays_the_eager_losses(crit):
    """A width-8 EquiUnet step with a distance-map criterion captured into one hipGraph: three replays reproduce the losses of
    three eager steps -- nothing in the criterion reads the host, or the capture would fail or bake one step's field in."""
    from brats21_amd import definer, get_model, transforms
    from brats21_amd.engine import GraphedTrainStep, TrainStep
    from brats21_amd.optim import Ranger2020
    from oracle import synth
    ns = argparse.Namespace(model="equiunet", width=8, norm="group", act="relu", num_classes=3, dropout=0)
    size = (32, 32, 32)
    xs = [synth.random_image(1, 4, size, seed=40 + i).to(DEV) for i in range(3)]
    ts = [synth.nested_spheres(1, size).to(DEV).roll(i, dims=-1) for i in range(3)]  # a new target (and field) every step
    if "boundary" in crit:
        ts = [[t, transforms.one_hot_to_dist(t)] for t in ts]
    results = []
    for graphed in (False, True):
        torch.manual_seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            m = get_model(ns).to(DEV).train()
            criterion = definer.make_criterion(argparse.Namespace(criterion=crit, num_classes=3))
        opt = Ranger2020(m.parameters(), lr=1e-3, weight_decay=1e-5, use_gc=True, capturable=graphed)
        step = TrainStep(m, opt, criterion=criterion, amp=True)
        if graphed:
            step = GraphedTrainStep(step, warmup=2)  # the first call: two eager warm-up steps on batch 0, the capture, one replay
            losses = [float(step(x, t).detach()) for x, t in zip(xs, ts)]
        else:
            losses = [float(step(x, t).detach()) for x, t in zip([xs[0]] * 2 + xs, [ts[0]] * 2 + ts)][2:]
        torch.cuda.synchronize()
        results.append(losses)
    assert len(results[1]) == 3 and all(np.isfinite(results[1]))
    assert len(set(results[0])) == 3  # the three steps differ: a replay that baked one target in would not follow them
    np.testing.assert_allclose(results[0], results[1], rtol=1e-5, atol=1e-6)


def test_train_augment_crops_the_distance_map_like_the_label():
    from brats21_amd.transforms import TrainAugment
    shape, roi = (2, 3, 20, 24, 20), (16, 16, 16)
    seg = torch.arange(int(np.prod(shape)), dtype=torch.float32, device=DEV).reshape(shape)  # every voxel its own value
    img = torch.randn((2, 4) + shape[2:], device=DEV)
    aug = TrainAugment(roi, seed=3)
    for k_rot, flip in ((0, False), (1, True), (2, False), (3, True)):
        p = {"start": (3, 5, 2), "k_rot": k_rot, "flip": flip, "offset": 0.05, "gamma": None, "noise_std": None, "smooth": None}
        x, y, dm = aug(img, seg, params=p, distance_map=seg)
        assert torch.equal(dm, y) and dm.shape == (2, 3) + roi
        two = aug(img, seg, params=p)
        assert len(two) == 2 and torch.equal(two[0], x) and torch.equal(two[1], y)
    x, y, dm = aug(img, seg, distance_map=seg)  # drawn parameters
    assert torch.equal(dm, y)
