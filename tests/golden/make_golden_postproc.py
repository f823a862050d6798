"""Generates tests/golden/postproc.npz from the REFERENCE's own label post-processing (utils/transforms.py:
KeepLargestConnectedComponent, ReplaceWithClosestValue, ConvertToBratsClassesBasedOnMultiChannel, ChangeLabel3To4,
remove_background_voxels) imported under oracle/refshim.py, the way make_golden.py::post_fixtures does.

Run here only (the GPU box has no reference checkout):  python tests/golden/make_golden_postproc.py
skimage is not installed: the stub's skimage.morphology.label is bound to scipy.ndimage.label with the full 3^n
structuring element, which finds the same components with the same raster numbering -- asserted against a plain
breadth-first search on every fixture.  scipy's griddata (the replacement's nearest search) is the real one.
MONAI's AsDiscrete(threshold_values) and ConvertToMultiChannelBasedOnBratsClasses are restated below (two lines each).
The archive holds arrays only.
"""
import os
import sys
import warnings
from collections import deque
from itertools import product

import numpy as np
import torch
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import refshim  # noqa: E402

refshim.install()
np.int = int  # the reference still uses the alias numpy >= 1.24 dropped


def _label(mask, **kw):
    return ndimage.label(mask, structure=np.ones((3,) * mask.ndim))[0]


sys.modules["skimage.morphology"].label = _label
from utils.transforms import (KeepLargestConnectedComponent, ReplaceWithClosestValue,  # noqa: E402
                              ConvertToBratsClassesBasedOnMultiChannel, ChangeLabel3To4, remove_background_voxels)

OUT = os.path.dirname(os.path.abspath(__file__))
CLEAN_T = (None, 0, 1, 10, 20)


def as_discrete(x, thresh):  # MONAI AsDiscrete(threshold_values=True, logit_thresh)
    return (x >= thresh).float()


def to_multichannel(lab):  # MONAI ConvertToMultiChannelBasedOnBratsClasses on [D, H, W] -> (TC, WT, ET)
    return np.stack([(lab == 1) | (lab == 4), (lab == 1) | (lab == 2) | (lab == 4), lab == 4]).astype(np.float32)


def bfs_numbering(mask):
    """Plain BFS, 26-neighbourhood, components numbered in C order of their first voxel."""
    lab = np.zeros(mask.shape, np.int32)
    k = 0
    for p in zip(*np.nonzero(mask)):
        if lab[p]:
            continue
        k += 1
        lab[p] = k
        q = deque([p])
        while q:
            c = q.popleft()
            for d in product((-1, 0, 1), repeat=3):
                u = tuple(a + b for a, b in zip(c, d))
                if all(0 <= u[i] < mask.shape[i] for i in range(3)) and mask[u] and not lab[u]:
                    lab[u] = k
                    q.append(u)
    return lab


def check_label_binding(vol):
    m = np.asarray(vol) != 0
    assert np.array_equal(_label(m), bfs_numbering(m)), "scipy labelling differs from the BFS numbering"


def tie_bits(vol, thresh, axis):
    """Per voxel: bit v set when value v lies at the minimum distance of a replaced pixel (0 elsewhere); brute force."""
    vals, counts = np.unique(vol, return_counts=True)
    rare = vals[counts <= thresh]
    bits = np.zeros(vol.shape, np.uint8)
    if not rare.any():
        return bits
    for k in range(vol.shape[axis]):
        sl = tuple(k if a == axis else slice(None) for a in range(3))
        s, b = vol[sl], bits[sl]
        m = np.isin(s, rare)
        src, dst = np.argwhere(~m), np.argwhere(m)
        if len(dst) == 0:
            continue
        if len(src) == 0:
            b[m] = 1
            continue
        d2 = ((dst[:, None] - src[None]) ** 2).sum(-1)
        near = d2 == d2.min(1, keepdims=True)
        sv = s[src[:, 0], src[:, 1]]
        for i, (y, x) in enumerate(dst):
            for v in np.unique(sv[near[i]]):
                b[y, x] |= np.uint8(1 << int(v))
    return bits


def ref_clean(vol, t):
    check_label_binding(vol)
    out = KeepLargestConnectedComponent(threshold=t)(torch.from_numpy(vol.astype(np.float32))[None, None])
    return np.asarray(out)[0, 0].astype(np.uint8)


def ref_replace(vol, t, axis):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # an all-rare slice: griddata's NaN -> uint8 0
        out = ReplaceWithClosestValue(labels=[3], thresh=t, axis=axis)(torch.from_numpy(vol.astype(np.float32))[None, None])
    out = np.asarray(out)[0, 0].astype(np.uint8)
    bits = tie_bits(vol, t, axis)
    moved = bits != 0
    assert np.all((bits[moved] >> out[moved]) & 1), "reference pick outside the tie set"
    assert np.array_equal(out[~moved], vol[~moved])
    return out, bits


def clean_volume():
    """Structured part (z < 12): lines of exactly T and T+1 voxels, edge- and corner-touching pairs, components on the
    faces; speckle part (z >= 14)."""
    rng = np.random.RandomState(20)
    D, H, W = 24, 20, 28
    v = np.zeros((D, H, W), np.uint8)
    y = 1
    for t in (1, 10, 20):                       # lines of t and t + 1 voxels along x, rows 2 apart
        for n, val in ((t, 1), (t + 1, 2)):
            v[3, y, 3:3 + n] = val
            y += 2
    v[6:8, 2:4, 2:4] = 4                        # edge contact: (6..7, 3, 3) ~ (6..7, 4, 4)
    v[6:8, 4:6, 4:6] = 1
    v[6:8, 9:11, 9:11] = 2                      # corner contact only: (7, 10, 10) ~ (8, 11, 11)
    v[8:10, 11:13, 11:13] = 4
    v[0, 15, 20:23] = 1                         # faces: z = 0, y = 0, y = H-1, x = 0, x = W-1 (z = D-1: speckle)
    v[5, 0, 16:19] = 2
    v[9, H - 1, 14:18] = 4
    v[10, 14:16, 0] = 1
    v[10, 6:9, W - 1] = 2
    sp = rng.rand(10, H, W) < 0.06
    v[14:] = np.where(sp, rng.choice(np.array([1, 2, 4], np.uint8), size=sp.shape), 0)
    return v


def clean_tie_volume():
    v = np.zeros((9, 10, 11), np.uint8)
    v[5:7, 2:4, 2:4] = 2                        # 8 voxels, later in C order
    v[1:3, 6:8, 6:8] = 1                        # 8 voxels, first in C order: kept by threshold None
    v[7, 8, 1:4] = 4
    return v


def rare_volume(kind, rng, axis):
    """(D, H, W) volumes for ReplaceWithClosestValue; the special slice lies across `axis`."""
    shape = (10, 12, 14)
    coarse = rng.choice(np.array([0, 1, 2], np.uint8), size=tuple(s // 2 for s in shape))
    base = coarse.repeat(2, 0).repeat(2, 1).repeat(2, 2)       # 2x2x2 patches: ties at patch borders
    if kind == "one":
        base[4:6, 5:7, 6:9] = 4                                 # 12 voxels of 4
        return base, 20
    if kind == "two":
        base[2:4, 2:4, 2:5] = 4                                 # 12 of 4
        base[base == 1] = 2
        base[7:9, 8:10, 9:11] = 1                               # 8 of 1
        return base, 20
    if kind == "zero":                                         # only 0 is rare: unchanged
        base[base == 0] = 2
        base[3, 4:7, 5] = 0
        return base, 20
    if kind == "none":                                         # nothing rare: unchanged
        return base, 5
    if kind == "allr":                                          # one slice entirely rare (4), plus a few 4 elsewhere
        sl = tuple(3 if a == axis else slice(None) for a in range(3))
        base[sl] = 4
        base[7, 9, 11] = 4
        base[8, 2, 2] = 4
        t = int((base == 4).sum())
        assert all(int((base == v).sum()) > t for v in (0, 1, 2))
        return base, t
    raise KeyError(kind)


def chain_fixture(res):
    """The four flag combinations of get_post_transforms + remove_background_voxels (learning/engine.py:244-259) on a
    probability map kept at least 0.05 away from the threshold; two 12-voxel blobs are joined only through zero-image
    voxels, so cleaning before background removal keeps them and the reverse order would not."""
    rng = np.random.RandomState(21)
    D, H, W = 18, 20, 22
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    r2 = (z - 8) ** 2 + (y - 9) ** 2 + (x - 10) ** 2
    wt, tc, et = r2 <= 49, r2 <= 25, ((z - 9) ** 2 + (y - 8) ** 2 + (x - 11) ** 2) <= 4
    tc = tc | ((rng.rand(D, H, W) < 0.01) & (z >= 4))         # TC outside WT: nesting broken on purpose
    wt[1:3, 1:3, 18:21] = True                                 # 12 voxels (dropped at 20)
    wt[1:3, 4:7, 18:20] = True                                 # 12 voxels, joined to the next blob through the bridge
    wt[1:3, 8:11, 18:20] = True
    wt[2, 7, 18] = True                                        # the bridge: a zero-image voxel
    wt[14:17, 15:18, 1:4] = True                               # 27 voxels (kept)
    img = np.ones((1, 4, D, H, W), np.float32) * np.arange(1, 5, dtype=np.float32)[None, :, None, None, None]
    img[:, :, :, :, 0] = 0                                     # zero-image border
    img[:, :, 2, 7, 18] = 0
    want = np.stack([tc, wt, et])[None]
    u = rng.rand(*want.shape)
    prob = np.where(want, 0.55 + 0.45 * u, 0.45 - 0.45 * u).astype(np.float16).astype(np.float32)
    assert np.abs(prob - 0.5).min() >= 0.05
    res["chain_prob"], res["chain_img"] = prob.astype(np.float16), img
    get_device = torch.Tensor.get_device
    torch.Tensor.get_device = lambda self: self.device
    try:
        for clean_on, replace_on in product((False, True), repeat=2):
            tag = f"chain_c{int(clean_on)}r{int(replace_on)}"
            s = as_discrete(torch.from_numpy(prob), 0.5)
            ties = np.zeros((D, H, W), np.uint8)
            if clean_on or replace_on:
                lab = ChangeLabel3To4()(ConvertToBratsClassesBasedOnMultiChannel()(s))
                if clean_on:
                    check_label_binding(lab[0, 0].numpy())
                    lab = KeepLargestConnectedComponent(threshold=20)(lab)
                if replace_on:
                    before = np.asarray(lab)[0, 0].astype(np.uint8)
                    lab = ReplaceWithClosestValue(labels=[3], thresh=300)(torch.as_tensor(np.asarray(lab)))
                    ties = tie_bits(before, 300, 2)
                s = torch.from_numpy(to_multichannel(np.asarray(lab)[0, 0]))[None]
            out = remove_background_voxels(torch.from_numpy(img), s).numpy()
            res[tag], res[tag + "_ties"] = out, ties
        joined = res["chain_c1r0"][0, 1, 1:3, 4:11, 18:20]
        assert joined.sum() == 24, "the bridged blobs must survive cleaning (chain before background removal)"
    finally:
        torch.Tensor.get_device = get_device


def main():
    res = {}
    for name, vol in (("clean_a", clean_volume()), ("clean_tie", clean_tie_volume())):
        res[name] = vol
        for t in CLEAN_T:
            res[f"{name}_t{'none' if t is None else t}"] = ref_clean(vol, t)
    kept = res["clean_tie_tnone"]
    assert kept[1:3, 6:8, 6:8].all() and not kept[5:7].any()
    rng = np.random.RandomState(22)
    for axis in (0, 1, 2):
        for kind in ("one", "two", "zero", "none", "allr"):
            vol, t = rare_volume(kind, rng, axis)
            out, bits = ref_replace(vol, t, axis)
            tag = f"rare_{kind}_ax{axis}"
            res[tag], res[tag + "_t"], res[tag + "_out"], res[tag + "_ties"] = vol, np.array(t), out, bits
            if kind in ("zero", "none"):
                assert np.array_equal(out, vol)
            if kind == "allr":
                sl = tuple(3 if a == axis else slice(None) for a in range(3))
                assert not out[sl].any()
    chain_fixture(res)
    path = os.path.join(OUT, "postproc.npz")
    np.savez_compressed(path, **res)
    print(path, os.path.getsize(path), "bytes,", len(res), "arrays")


if __name__ == "__main__":
    main()
