"""-m gpu: STAPLE fusion on the GPU (brats21_amd.ops.staple / StaplePacker, csrc/staple.hip; evaluate.perform_staple_on_brats_multi_channel,
Evaluator(perform_staple=True)) against the numpy float64 restatement of ITK's STAPLEImageFilter, tests/_staple_ref.py.

Bars.  The kernels and the oracle evaluate the same f64 expressions; only the order of the sums over voxels differs.
  iterations : equal (ITK's GetElapsedIterations(); a difference of one at the 1e-7 stopping step is a failure to look into).
  prior      : exactly equal -- an exact integer sum and one division on both sides.
  p, q       : within 1e-12 -- sums of at most 1.1e5 terms in [0, 1] in another order; a term's rounding is 1.1e-16.
  mask       : equal at EVERY voxel; each case first asserts on the oracle alone that no weight lies within 1e-6 of the threshold,
               so no voxel needs an exemption.
The degenerate channels (nobody marks it / everybody fills it) stop in the iteration of index 1, so ``iterations`` reads 1 there
-- the loop body has run twice; tests/test_staple_cpu.py pins the same on the oracle."""
import argparse
import functools

import numpy as np
import pytest
import torch

import _staple_ref as R
from oracle import synth, unet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL, LARGE = (13, 18, 21), (40, 48, 56)  # 4914 voxels: 20 tiles, the last one ragged; 107520: 420 workgroups, 105 sum rows per lane group
TOL = 1e-12


@functools.lru_cache(maxsize=None)
def raters_of(shape, raters, channels=3):
    """[R, C, *shape] uint8, another seed per channel."""
    return np.stack([R.make_raters(shape, raters, 100 + raters + 1000 * c) for c in range(channels)], axis=1)


@functools.lru_cache(maxsize=None)
def oracle_of(shape, raters, max_iterations=10000):
    d = raters_of(shape, raters)
    return [R.staple(d[:, c], max_iterations) for c in range(d.shape[1])]


def as_maps(d, dtype=torch.float32):
    """[R, C, D, H, W] array -> R cuda maps [1, C, D, H, W]."""
    return [torch.from_numpy(np.ascontiguousarray(m))[None].to(DEV).to(dtype) for m in d]


def check(seg, info, want, threshold, n=0):
    """want: the oracle's (W, p, q, iterations, g) per channel."""
    for c, (w, p, q, it, g) in enumerate(want):
        finite = w[np.isfinite(w)]
        assert finite.size == 0 or np.abs(finite - threshold).min() > 1e-6, "the case has a weight on the threshold"
        gp, gq = info["p"][n, c].cpu().numpy(), info["q"][n, c].cpu().numpy()
        print(f"channel {c}: iterations {int(info['iterations'][n, c])} / {it}, max |dp| {np.nanmax(np.abs(gp - p)) if finite.size else 0:.2e}, "
              f"max |dq| {np.nanmax(np.abs(gq - q)) if finite.size else 0:.2e}")
        assert int(info["iterations"][n, c]) == it
        assert float(info["prior"][n, c]) == g
        np.testing.assert_allclose(gp, p, rtol=0, atol=TOL, equal_nan=True)
        np.testing.assert_allclose(gq, q, rtol=0, atol=TOL, equal_nan=True)
        np.testing.assert_array_equal(seg[n, c].cpu().numpy(), R.fused_mask(w, threshold).astype(np.float32))


@pytest.mark.parametrize("raters", [1, 2, 5, 32, 33, 64, 65, 70])
def test_parity_with_the_oracle_over_the_word_and_lane_boundaries(raters):
    from brats21_amd import ops
    d = raters_of(SMALL, raters)
    seg, info = ops.staple(as_maps(d), return_probability=True)
    assert seg.dtype == torch.float32 and tuple(seg.shape) == (1, 3) + SMALL
    assert info["p"].dtype == torch.float64 and tuple(info["p"].shape) == (1, 3, raters) and info["p"].is_cuda
    want = oracle_of(SMALL, raters)
    check(seg, info, want, 0.5)
    # the weights themselves, the same expression of p, q at every voxel: dW = W (1 - W) sum_j d(log factor_j), at most
    # 0.25 * 2 R * 1e-12 / (smallest factor, about the 1 % flip rate) = 3.5e-9 at R = 70
    for c in range(3):
        np.testing.assert_allclose(info["probability"][0, c].cpu().numpy(), want[c][0], rtol=0, atol=1e-8)
    if raters == 1:
        np.testing.assert_array_equal(seg.cpu().numpy()[0], d[0].astype(np.float32))


@pytest.mark.parametrize("raters", [5, 40])
def test_more_than_one_workgroup_and_sum_row_and_three_thresholds(raters):
    from brats21_amd import ops
    d = raters_of(LARGE, raters)
    pk = ops.StaplePacker((1, 3) + LARGE, raters, DEV)
    for m in as_maps(d, torch.uint8):
        pk.add(m)
    for threshold in (0.1, 0.5, 0.9):
        seg, info = ops.staple(pk, threshold=threshold)
        check(seg, info, oracle_of(LARGE, raters), threshold)


def test_degenerate_channels_and_a_batch_of_two():
    from brats21_amd import ops
    a, b = raters_of(SMALL, 5).copy(), raters_of(SMALL, 33)[:5].copy()
    for d in (a, b):
        d[:, 1] = 0  # nobody marks channel 1
        d[:, 2] = 1  # everybody fills channel 2
    one = [ops.staple(as_maps(d)) for d in (a, b)]
    for (seg, info), d in zip(one, (a, b)):
        w, p, q, it, g = R.staple(d[:, 0])
        check(seg, info, [(w, p, q, it, g)], 0.5)
        assert info["iterations"][0].tolist() == [it, 1, 1]
        assert info["prior"][0].tolist() == [g, 0.0, 1.0]
        assert not seg[0, 1:].any() and seg[0, 0].any()
        assert bool(torch.isnan(info["p"][0, 1:]).all()) and bool(torch.isnan(info["q"][0, 1:]).all())
    # channel 0 does not see its neighbours: the same bits as the call without degenerate channels
    clean = ops.staple(as_maps(raters_of(SMALL, 5)))
    assert torch.equal(clean[0][0, 0], one[0][0][0, 0]) and torch.equal(clean[1]["p"][0, 0], one[0][1]["p"][0, 0])
    # N = 2 with other raters per sample = two N = 1 calls
    both = [torch.cat([x, y]) for x, y in zip(as_maps(a), as_maps(b))]
    seg2, info2 = ops.staple(both)
    for n in (0, 1):
        assert torch.equal(seg2[n], one[n][0][0])
        assert torch.equal(info2["iterations"][n], one[n][1]["iterations"][0])
        for k in ("p", "q", "prior"):
            assert torch.equal(info2[k][n].nan_to_num(-1.0), one[n][1][k][0].nan_to_num(-1.0)), (n, k)


@pytest.mark.parametrize("cap", [1, 3])
def test_max_iterations_stops_there(cap):
    from brats21_amd import ops
    seg, info = ops.staple(as_maps(raters_of(SMALL, 5)), max_iterations=cap)
    assert info["iterations"].tolist() == [[cap] * 3]
    check(seg, info, oracle_of(SMALL, 5, cap), 0.5)


def test_chunk_length_does_not_change_a_bit():
    from brats21_amd import ops
    maps = as_maps(raters_of(SMALL, 33))
    base_seg, base = ops.staple(maps, return_probability=True)
    assert base["chunk"] == ops.STAPLE_CHUNK and base["host_reads"] >= 1
    for chunk in (1, 7):
        seg, info = ops.staple(maps, return_probability=True, chunk=chunk)
        assert info["chunk"] == chunk and torch.equal(seg, base_seg)
        for k in ("p", "q", "prior", "iterations", "probability"):
            assert torch.equal(info[k], base[k]), (chunk, k)
    its = int(base["iterations"].max())
    assert ops.staple(maps, chunk=1)[1]["host_reads"] == its + 1  # iterations 0 .. its ran, one read after each


def test_streaming_forms_agree_and_two_runs_give_the_same_bits():
    from brats21_amd import ops
    d = raters_of(SMALL, 70)
    packers = []
    for dtype in (torch.float32, torch.uint8, torch.bool):
        pk = ops.StaplePacker((1, 3) + SMALL, 70)
        for m in as_maps(d, dtype):
            pk.add(m)
        packers.append(pk)
    wide = ops.StaplePacker((1, 3) + SMALL, 200, DEV)  # made for more raters than it gets: three words used of seven
    for m in as_maps(d):
        wide.add(m)
    want_bits = np.zeros((3, 3, int(np.prod(SMALL))), dtype=np.uint32)
    for j in range(70):
        want_bits[:, j // 32] |= d[j].reshape(3, -1).astype(np.uint32) << np.uint32(j % 32)
    for pk in packers:
        np.testing.assert_array_equal(pk.bits.cpu().numpy().view(np.uint32), want_bits)
        np.testing.assert_array_equal(pk.counts.cpu().numpy().T, d.reshape(70, 3, -1).sum(-1))
    np.testing.assert_array_equal(wide.bits[:, :3].cpu().numpy().view(np.uint32), want_bits)
    runs = [ops.staple(pk) for pk in packers] + [ops.staple(wide), ops.staple(as_maps(d)), ops.staple(packers[0])]
    for seg, info in runs[1:]:
        assert torch.equal(seg, runs[0][0])
        for k in ("p", "q", "prior", "iterations"):
            assert torch.equal(info[k], runs[0][1][k]), k
    check(*runs[0], oracle_of(SMALL, 70), 0.5)
    with pytest.raises(ValueError, match="70 raters"):
        packers[0].add(as_maps(d[:1])[0])


def test_cpu_inputs_of_the_reference_function_come_back_on_the_cpu():
    from brats21_amd.evaluate import perform_staple_on_brats_multi_channel as fuse
    d = raters_of(SMALL, 5)
    cpu = [torch.from_numpy(np.ascontiguousarray(m))[None] for m in d]
    out = fuse(cpu, threshold_value=0.5)
    assert out.device.type == "cpu" and out.dtype == torch.float32
    gpu = fuse([m.to(DEV) for m in cpu])
    assert gpu.is_cuda and torch.equal(gpu.cpu(), out)
    arr = fuse([m.numpy() for m in cpu], return_as_tensor=False)
    assert isinstance(arr, np.ndarray) and np.array_equal(arr, out.numpy())
    for c, (w, *_) in enumerate(oracle_of(SMALL, 5)):
        np.testing.assert_array_equal(out[0, c].numpy(), R.fused_mask(w).astype(np.float32))


# ---- Evaluator --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _models():
    from brats21_amd import get_model
    models = []
    for seed in (0, 1):
        sd = synth.fill_state_dict(unet.equiunet_state_shapes(8))
        if seed:  # the second member of the ensemble: the same weights, jittered
            gen = torch.Generator().manual_seed(seed)
            sd = {k: v + 0.05 * v.abs().mean() * torch.randn(v.shape, generator=gen) if v.is_floating_point() and "weight" in k else v
                  for k, v in sd.items()}
        m = get_model(argparse.Namespace(model="equiunet", width=8, norm="group", act="relu", num_classes=3, dropout=0))
        m.load_state_dict(sd)
        m = m.to(DEV).eval()
        m.skip_deep_heads_in_eval = True
        models.append(m)
    return models


def _image():
    size = (32, 40, 24)  # k_divisible = 16 pads it to 32 x 48 x 32
    x = synth.closed_form_image(1, 4, size, "staplecase")
    return (x * (synth.closed_form("staplemask", (1, 1) + size) > -0.3)).to(DEV)


@pytest.mark.parametrize("cleaning", [None, 20])
def test_evaluator_fuses_every_model_and_tta_pass_as_a_rater(cleaning):
    from brats21_amd import tta
    from brats21_amd.inferers import _first
    from brats21_amd.evaluate import (Evaluator, _post_chain, perform_staple_on_brats_multi_channel, remove_background_voxels,
                                      shape_to_divisible, shape_to_original, to_brats_labels)
    models, x = _models(), _image()
    ev = Evaluator(models, tta_transforms=tta.get_tta_transforms(), k_divisible=16, amp=False, perform_staple=True,
                   staple_threshold=0.4, cleaning_areas_threshold=cleaning)
    assert ev.raters == 32
    res = ev(x, want_labels=True)
    with torch.no_grad():
        xp, p_b, p_a = shape_to_divisible(x, k=16)
        assert tuple(xp.shape[2:]) == (32, 48, 32)
        raters = []
        for m in models:
            for t in tta.get_tta_transforms():
                logits = _first(m(t.augment_image(xp))).float()
                prob = torch.zeros(t.deaug_perm.out_shape(logits.shape), dtype=torch.float32, device=DEV)
                t.accumulate_probability(logits, prob)
                raters.append(_post_chain(prob, 1, 0.5, cleaning_threshold=cleaning, clean=cleaning is not None))
        assert len({int(r.sum()) for r in raters}) > 8  # the raters do differ
        fused = perform_staple_on_brats_multi_channel(raters, threshold_value=0.4)
        seg = remove_background_voxels(xp, fused)
        assert seg.any() and not torch.equal(seg, fused)
        assert torch.equal(res["seg"], shape_to_original(seg, p_b, p_a))
        assert torch.equal(res["labels"], shape_to_original(to_brats_labels(seg).float(), p_b, p_a).to(torch.uint8))
    assert tuple(res["staple"]["p"].shape) == (1, 3, 32) and int(res["staple"]["iterations"].min()) >= 1


def test_evaluator_without_staple_is_unchanged():
    from brats21_amd import tta
    from brats21_amd.evaluate import Evaluator
    models, x = _models(), _image()
    tgt = synth.nested_spheres(1, (32, 40, 24)).to(DEV)
    kw = dict(tta_transforms=tta.get_tta_transforms(), k_divisible=16, amp=False, cleaning_areas_threshold=20)
    a = Evaluator(models, **kw)(x, tgt, want_labels=True)
    b = Evaluator(models, perform_staple=False, staple_threshold=0.3, **kw)(x, tgt, want_labels=True)
    assert set(a) == set(b) == {"seg", "labels", "dice"}
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
