"""-m gpu: the label post-processing of get_post_transforms (--cleaning_areas / --replace_value) on the GPU
(brats21_amd/evaluate.py, csrc/postproc.hip) against the reference's golden vectors (tests/golden/postproc.npz), the CPU
restatement tests/_postproc_ref.py, and full-size volumes whose answer is known by construction."""
import argparse
import os

import numpy as np
import pytest
import torch

import _postproc_ref as ref
from oracle import evaluate as oev
from oracle import synth, unet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _labels_match(got, want, ties, what=""):
    """Equal, or (where the reference's pick is a tie) a value from the tie set."""
    got, want = np.asarray(got).astype(np.uint8), np.asarray(want).astype(np.uint8)
    ok = (got == want) | ((ties != 0) & (((ties >> np.minimum(got, 7)) & 1) == 1) & (got < 8))
    assert ok.all(), f"{what}: {int((~ok).sum())} voxels differ outside the tie sets"


def test_cleaning_matches_reference_golden_for_every_threshold(golden_dir):
    from brats21_amd.evaluate import KeepLargestConnectedComponent
    g = np.load(os.path.join(golden_dir, "postproc.npz"))
    for name in ("clean_a", "clean_tie"):
        vol = torch.from_numpy(g[name])
        for t in (None, 0, 1, 10, 20):
            want = g[f"{name}_t{'none' if t is None else t}"]
            out = KeepLargestConnectedComponent(t)(vol.float()[None, None].to(DEV))
            assert out.dtype == torch.float32 and out.device.type == "cuda" and tuple(out.shape) == (1, 1) + vol.shape
            np.testing.assert_array_equal(out[0, 0].cpu().numpy(), want, err_msg=f"{name} threshold {t}")
            out3 = KeepLargestConnectedComponent(t)(vol.to(DEV))                 # uint8 [D, H, W]
            np.testing.assert_array_equal(out3.cpu().numpy(), want)
    # no foreground: unchanged for every threshold (the reference raises for None)
    z = torch.zeros(1, 1, 5, 6, 7, device=DEV)
    for t in (None, 0, 20):
        assert not KeepLargestConnectedComponent(t)(z).any()


def test_replacement_matches_reference_golden(golden_dir):
    from brats21_amd.evaluate import ReplaceWithClosestValue
    g = np.load(os.path.join(golden_dir, "postproc.npz"))
    for axis in (0, 1, 2):
        for kind in ("one", "two", "zero", "none", "allr"):
            tag = f"rare_{kind}_ax{axis}"
            vol = torch.from_numpy(g[tag])
            out = ReplaceWithClosestValue([3], thresh=int(g[tag + "_t"]), axis=axis)(vol.float()[None, None].to(DEV))
            got = out[0, 0].cpu().numpy()
            if kind in ("zero", "none"):
                np.testing.assert_array_equal(got.astype(np.uint8), g[tag], err_msg=tag)   # unchanged, byte for byte
            _labels_match(got, g[tag + "_out"], g[tag + "_ties"], tag)
            # the documented tie rule: the equidistant pixel first in the slice's row-major order
            mine, _ = ref.replace(g[tag], int(g[tag + "_t"]), axis)
            np.testing.assert_array_equal(got.astype(np.uint8), mine, err_msg=tag)
    # a constructed tie in the axial slice w = 1: the rare pixel (2, 2) has four neighbours at distance 1
    v = np.zeros((5, 5, 3), np.uint8)
    v[:, :, :] = 2
    v[0:2, :, :] = 1
    v[2, 0:2, :] = 1
    v[2, 2, 1] = 4                                 # rare (count 1) in slice w = 1
    out = ReplaceWithClosestValue([3], thresh=1, axis=2)(torch.from_numpy(v).to(DEV)).cpu().numpy()
    # candidates at distance 1: (1, 2) = 1, (2, 1) = 1, (2, 3) = 2, (3, 2) = 2 -> row-major first is (1, 2)
    assert out[2, 2, 1] == 1
    v[1, 2, 1] = 2
    v[2, 1, 1] = 2
    v[2, 3, 1] = 1
    out = ReplaceWithClosestValue([3], thresh=1, axis=2)(torch.from_numpy(v).to(DEV)).cpu().numpy()
    assert out[2, 2, 1] == 2                       # now (1, 2) = 2 comes first


def test_post_transforms_chain_matches_golden_cuda_and_cpu(golden_dir):
    from brats21_amd import evaluate as ev
    g = np.load(os.path.join(golden_dir, "postproc.npz"))
    prob = torch.from_numpy(g["chain_prob"].astype(np.float32))
    img = torch.from_numpy(g["chain_img"]).to(DEV)
    for c in (0, 1):
        for r in (0, 1):
            tag = f"chain_c{c}r{r}"
            args = argparse.Namespace(cleaning_areas=bool(c), cleaning_areas_threshold=20, replace_value=bool(r),
                                      replace_value_threshold=300, logit_threshold=0.5)
            post = ev.get_post_transforms(args)
            for dev in (DEV, "cpu"):
                out = post(prob.to(dev))
                assert out.device.type == torch.device(dev).type and out.dtype == torch.float32
                seg = ev.remove_background_voxels(img, out.to(DEV)).cpu().numpy()
                ties = g[tag + "_ties"]
                want = g[tag]
                if not ties.any():
                    np.testing.assert_array_equal(seg, want, err_msg=f"{tag} {dev}")
                else:
                    _labels_match(ref.to_labels(seg[0]), ref.to_labels(want[0]), ties, tag)
    # no flags: the threshold alone (src/definer.py:695-697)
    out = ev.get_post_transforms(argparse.Namespace())(prob.to(DEV))
    np.testing.assert_array_equal(out.cpu().numpy(), (prob >= 0.5).float().numpy())


# ---- full size ----------------------------------------------------------------------------------------------------------
class _Builder:
    """Components placed by construction, with the promise checked on the fly: no part touches (26-neighbourhood) a voxel
    of another component."""

    def __init__(self, shape):
        self.vol = np.zeros(shape, np.uint8)
        self.cid = np.zeros(shape, np.int32)
        self.sizes = [0]

    def add(self, n, parts, value=1):
        k = len(self.sizes)
        size = 0
        for z, y, x in parts:
            box = (n, slice(max(z.start - 1, 0), z.stop + 1), slice(max(y.start - 1, 0), y.stop + 1),
                   slice(max(x.start - 1, 0), x.stop + 1))
            other = self.cid[box]
            assert not ((other != 0) & (other != k)).any(), "constructed components touch"
            sel = (n, z, y, x)
            fresh = self.cid[sel] == 0
            size += int(fresh.sum())
            self.cid[sel] = k
            self.vol[sel] = value
        self.sizes.append(size)
        return size

    def expected(self, t):
        keep = np.asarray(self.sizes) > t
        keep[0] = False
        return np.where(keep[self.cid], self.vol, 0).astype(np.uint8)


def _full_size_cleaning_case():
    N, D, H, W = 2, 160, 240, 240
    b = _Builder((N, D, H, W))
    s = slice
    for n in range(N):
        for i, (a, c, d) in enumerate([(1, 1, 1), (1, 1, 5), (1, 1, 19), (1, 4, 5), (1, 3, 7), (3, 3, 3), (2, 2, 7),
                                       (4, 4, 4), (3, 3, 4), (1, 1, 21)]):
            z0, x0 = 4 + 6 * (i % 4), 4 + 30 * (i // 4)
            b.add(n, [(s(z0, z0 + a), s(6, 6 + c), s(x0, x0 + d))], value=(1, 2, 4)[i % 3])
        b.add(n, [(s(30, 32), s(20, 22), s(20, 22)), (s(30, 32), s(22, 24), s(22, 24))], 4)   # edge-touching pair: 16
        b.add(n, [(s(30, 32), s(30, 32), s(30, 32)), (s(32, 34), s(32, 34), s(32, 34))], 2)   # corner-touching pair: 16
    for y in (40, 44):                                                                     # x = W-1 / x = 0 of rows y, y+1
        b.add(0, [(s(36, 37), s(y, y + 1), s(W - 12, W))], 1)
        b.add(0, [(s(36, 37), s(y + 1, y + 2), s(0, 12))], 2)
    b.add(0, [(s(38, 39), s(H - 1, H), s(60, 72))], 1)                                      # y = H-1 / y = 0 of planes z, z+1
    b.add(0, [(s(39, 40), s(0, 1), s(60, 72))], 2)
    b.add(0, [(s(D - 1, D), s(100, 101), s(100, 112))], 4)                                  # last plane of sample 0 /
    b.add(1, [(s(0, 1), s(100, 101), s(100, 112))], 4)                                      # first plane of sample 1
    # serpentine in sample 0: 20 planes of 1-voxel rows (x 5..234) joined alternately at the row ends, planes joined at one
    # corner -- 557 k voxels in one long thin component
    parts = []
    for p in range(20):
        z = 60 + 2 * p
        for r in range(120):
            parts.append((s(z, z + 1), s(2 * r, 2 * r + 1), s(5, 235)))
            if r < 119:
                xe = 234 if r % 2 == 0 else 5
                parts.append((s(z, z + 1), s(2 * r + 1, 2 * r + 2), s(xe, xe + 1)))
        if p < 19:
            parts.append((s(z + 1, z + 2), s(0, 1), s(5, 6)))
    serp = b.add(0, parts, 2)
    assert serp >= 500_000
    return b


def test_cleaning_full_size_known_by_construction():
    from brats21_amd.evaluate import KeepLargestConnectedComponent
    b = _full_size_cleaning_case()
    x = torch.from_numpy(b.vol)[:, None].to(DEV)                    # [2, 1, 160, 240, 240] uint8
    for t in (0, 20, 27):                                           # 27 = the 3x3x3 blob: strict '>' drops it
        want = b.expected(t)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = KeepLargestConnectedComponent(t)(x)
        end.record()
        torch.cuda.synchronize()
        got = out[:, 0].to(torch.uint8).cpu().numpy()
        np.testing.assert_array_equal(got, want, err_msg=f"threshold {t}")
        again = KeepLargestConnectedComponent(t)(x)[:, 0].to(torch.uint8).cpu().numpy()
        assert np.array_equal(got, again), "not reproducible"
        assert start.elapsed_time(end) < 1000.0, f"{start.elapsed_time(end):.1f} ms: find() walks long chains"
    # the 12-voxel pieces split by a row, plane or sample boundary are dropped at 20: had they merged, they would be kept
    assert b.sizes.count(12) == 8 and not b.expected(20)[0, 36:40].any()
    largest = KeepLargestConnectedComponent(None)(x)[:, 0].to(torch.uint8).cpu().numpy()
    sizes = np.asarray(b.sizes)
    for n in range(2):
        ids = np.unique(b.cid[n])
        k = ids[ids > 0][np.argmax(sizes[ids[ids > 0]])]
        np.testing.assert_array_equal(largest[n], np.where(b.cid[n] == k, b.vol[n], 0), err_msg=f"largest, sample {n}")
    assert sizes[b.cid[0][60, 0, 5]] >= 500_000


def test_replacement_full_size_vs_brute_force():
    from brats21_amd.evaluate import ReplaceWithClosestValue
    rng = np.random.RandomState(5)
    D, H, W = 160, 240, 240
    z, y, x = np.ogrid[:D, :H, :W]
    r2 = (z - 80) ** 2 + (y - 120) ** 2 + (x - 120) ** 2
    vol = np.where(r2 < 60 ** 2, 2, 0).astype(np.uint8)
    vol[r2 < 30 ** 2] = 1
    ws = rng.choice(np.arange(60, 180), size=20, replace=False)
    for w in ws:                                                  # 20 slices, 15 voxels of 4 each: 300
        pts = rng.randint(0, 120, size=(15, 2))
        d, h = 20 + pts[:, 0], 60 + pts[:, 1]
        vol[d, h, w] = 4
    assert (vol == 4).sum() <= 300
    t = int((vol == 4).sum())
    out = ReplaceWithClosestValue([3], thresh=t, axis=2)(torch.from_numpy(vol)[None, None].to(DEV))[0, 0]
    got = out.to(torch.uint8).cpu().numpy()
    rare = vol == 4
    np.testing.assert_array_equal(got[~rare], vol[~rare])
    for w in np.unique(np.nonzero(rare)[2]):
        s = vol[:, :, w]
        src = np.argwhere(s != 4)                                   # row-major: argmin takes the documented first minimum
        for d, h in np.argwhere(s == 4):
            d2 = (src[:, 0] - d) ** 2 + (src[:, 1] - h) ** 2
            k = int(np.argmin(d2))
            assert got[d, h, w] == s[src[k, 0], src[k, 1]], (d, h, w)


def test_seeded_small_volumes_vs_cpu_restatement():
    from brats21_amd.evaluate import KeepLargestConnectedComponent, ReplaceWithClosestValue
    rng = np.random.RandomState(11)
    shapes = [(1, 7, 9), (5, 1, 13), (3, 4, 1), (17, 3, 2), (1, 1, 33), (2, 33, 1), (9, 9, 9), (1, 31, 17), (13, 2, 29),
              (6, 7, 8), (33, 1, 3), (4, 32, 5), (1, 2, 1), (15, 15, 1), (3, 3, 3), (8, 1, 1), (21, 5, 6), (2, 2, 40),
              (11, 12, 13), (7, 40, 3)]
    for i, shape in enumerate(shapes):
        dens = rng.uniform(0.05, 0.7)
        vol = np.where(rng.rand(*shape) < dens, rng.choice(np.array([1, 2, 4], np.uint8), size=shape), 0).astype(np.uint8)
        t = [None, 0, 1, 3, 6][i % 5]
        got = KeepLargestConnectedComponent(t)(torch.from_numpy(vol).to(DEV)).cpu().numpy()
        np.testing.assert_array_equal(got, ref.clean(vol, t), err_msg=f"clean {shape} {t}")
        for axis in (0, 1, 2):
            rt = int(rng.randint(0, max(2, vol.size // 4)))
            got = ReplaceWithClosestValue([3], thresh=rt, axis=axis)(torch.from_numpy(vol).float().to(DEV)).cpu().numpy()
            want, ties = ref.replace(vol, rt, axis)
            np.testing.assert_array_equal(got.astype(np.uint8), want, err_msg=f"replace {shape} {rt} {axis}")
            _labels_match(got, want, ties)


def test_evaluator_with_both_flags_vs_cpu_restatement():
    """Evaluator(cleaning_areas_threshold=20, replace_value_threshold=300) on the EquiUnet w8 case of test_post_gpu.py:
    equals the CPU restatement run on the same probability sum, then background removal and the crop."""
    from brats21_amd import get_model, tta
    from brats21_amd.evaluate import Evaluator, shape_to_divisible
    sd = synth.fill_state_dict(unet.equiunet_state_shapes(8))
    m = get_model(argparse.Namespace(model="equiunet", width=8, norm="group", act="relu", num_classes=3, dropout=0))
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    m.skip_deep_heads_in_eval = True
    x = synth.closed_form_image(1, 4, (21, 18, 22), "evalcase")
    x = x * (synth.closed_form("evalmask", (1, 1, 21, 18, 22)) > -0.3)
    tgt = synth.nested_spheres(1, (21, 18, 22))
    comp = tta.Compose([tta.OnAxes(axes=["zxy", "xyz"]), tta.HorizontalFlip(), tta.Rotate90(angles=[0, 90, 180, 270])])
    ev = Evaluator(m, tta_transforms=comp, sliding_window_size=(16, 16, 16), overlap=0.5, amp=False,
                   cleaning_areas_threshold=20, replace_value_threshold=300)
    res = ev(x.to(DEV), tgt.to(DEV), want_labels=True)
    with torch.no_grad():
        xp, p_b, p_a = shape_to_divisible(x.to(DEV), k=8)
        acc, passes = ev.probability_sum(xp)
    mean = acc.cpu() * torch.tensor(1.0 / passes, dtype=torch.float32)   # the kernel's f32 mean
    seg, _ = ref.chain(mean, 0.5, 20, True, 300, True)
    seg = torch.from_numpy(ref.remove_background(xp.cpu(), seg))
    dice_ref = oev.hard_dice_metric(seg, oev.shape_to_divisible(tgt, k=8)[0])
    seg_c = oev.shape_to_original(seg, p_b, p_a)
    lab_c = oev.shape_to_original(torch.from_numpy(ref.to_labels(seg[0].numpy()))[None, None].float(), p_b, p_a)
    assert tuple(res["seg"].shape) == (1, 3, 21, 18, 22) and tuple(res["labels"].shape) == (1, 1, 21, 18, 22)
    # _postproc_ref breaks ties by the same documented rule (first in row-major order), so everything is exact
    np.testing.assert_array_equal(res["labels"].cpu().numpy(), lab_c.numpy().astype(np.uint8))
    assert torch.equal(res["seg"].cpu(), seg_c)
    torch.testing.assert_close(res["dice"].cpu(), dice_ref.float(), atol=1e-7, rtol=0)
    assert 0.0 < float(seg.mean()) < 1.0
