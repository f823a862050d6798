"""CPU restatement (numpy / torch only) of the reference's label post-processing, for small volumes: the checker of
brats21_amd.evaluate's KeepLargestConnectedComponent / ReplaceWithClosestValue / get_post_transforms chain.

clean(): utils/transforms.py:579-600 with a breadth-first 26-connected labelling.  replace(): utils/transforms.py:603-647
with a brute-force nearest search; it also returns, per voxel, the bit mask of every value found at the minimum distance,
so a caller can accept any of the values the reference's KD-tree might have picked.  Nothing here imports scipy or reads
the reference checkout: GPU tests import this module.
"""
from collections import deque

import numpy as np
import torch

OFFSETS = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) != (0, 0, 0)]


def components(mask):
    """26-connected components of a 3-D bool array -> (int32 labels numbered 1.. in C order of first voxel, sizes)."""
    mask = np.asarray(mask, dtype=bool)
    d, h, w = mask.shape
    pad = np.zeros((d + 2, h + 2, w + 2), dtype=bool)
    pad[1:-1, 1:-1, 1:-1] = mask
    strides = ((h + 2) * (w + 2), w + 2, 1)
    offs = [dz * strides[0] + dy * strides[1] + dx for dz, dy, dx in OFFSETS]
    flat = pad.ravel()
    lab = np.zeros(flat.shape, dtype=np.int32)
    sizes = [0]
    for start in np.flatnonzero(flat):
        if lab[start]:
            continue
        k = len(sizes)
        lab[start] = k
        q, n = deque([start]), 0
        while q:
            v = q.popleft()
            n += 1
            for o in offs:
                u = v + o
                if flat[u] and not lab[u]:
                    lab[u] = k
                    q.append(u)
        sizes.append(n)
    return lab.reshape(pad.shape)[1:-1, 1:-1, 1:-1].copy(), np.asarray(sizes, dtype=np.int64)


def clean(vol, threshold):
    """get_largest_component on one 3-D label volume: keep components with more than `threshold` voxels, or only the
    largest (first on ties) when threshold is None; a volume without foreground stays unchanged."""
    vol = np.array(vol, copy=True)
    lab, sizes = components(vol != 0)
    if len(sizes) == 1:
        return vol
    if threshold is None:
        keep = np.zeros(len(sizes), dtype=bool)
        keep[int(np.argmax(sizes[1:])) + 1] = True
    else:
        keep = sizes > threshold
        keep[0] = False
    vol[~keep[lab]] = 0
    return vol


def _slices(shape, axis):
    for k in range(shape[axis]):
        idx = [slice(None)] * 3
        idx[axis] = k
        yield tuple(idx)


def replace(vol, thresh, axis=2):
    """replace_w_closest_value_3d as ReplaceWithClosestValue drives it, on one 3-D label volume.
    -> (result uint8, tie bit mask uint8: bit v set when value v lies at the minimum distance; 0 where unchanged)."""
    vol = np.asarray(vol).astype(np.uint8)
    out = vol.copy()
    ties = np.zeros(vol.shape, dtype=np.uint8)
    vals, counts = np.unique(vol, return_counts=True)
    rare = vals[counts <= thresh]
    if not rare.any():
        return out, ties
    for sl in _slices(vol.shape, axis):
        s = vol[sl]
        m = np.isin(s, rare)
        if not m.any():
            continue
        o, t = out[sl], ties[sl]
        src = np.argwhere(~m)            # row-major order: the documented tie rule takes the first minimum
        dst = np.argwhere(m)
        if len(src) == 0:
            o[m] = 0
            t[m] = 1
            continue
        d2 = ((dst[:, None, :] - src[None, :, :]) ** 2).sum(-1)
        best = d2.min(1)
        pick = d2.argmin(1)
        sv = s[src[:, 0], src[:, 1]]
        o[dst[:, 0], dst[:, 1]] = sv[pick]
        bits = np.zeros(len(dst), dtype=np.uint8)
        for v in np.unique(sv):
            hit = ((d2 == best[:, None]) & (sv[None, :] == v)).any(1)
            bits |= np.where(hit, np.uint8(1 << int(v)), np.uint8(0)) if v < 8 else 0
        t[dst[:, 0], dst[:, 1]] = bits
    return out, ties


def to_labels(seg):
    """AsDiscrete'd [3, D, H, W] (TC, WT, ET) -> BraTS labels (utils/transforms.py:169-206: ET 4, TC&!ET 1, WT&!TC 2)."""
    seg = np.asarray(seg) != 0
    tc, wt, et = seg[0], seg[1], seg[2]
    lab = np.zeros(tc.shape, dtype=np.uint8)
    lab[et] = 4
    lab[tc & ~et] = 1
    lab[wt & ~tc] = 2
    return lab


def to_channels(lab):
    """ConvertToMultiChannelBasedOnBratsClasses: TC = {1, 4}, WT = {1, 2, 4}, ET = {4} -> f32 [3, D, H, W]."""
    tc = (lab == 1) | (lab == 4)
    return np.stack([tc, tc | (lab == 2), lab == 4]).astype(np.float32)


def chain(mean, thresh=0.5, cleaning_threshold=None, clean_on=False, replace_threshold=None, replace_on=False):
    """get_post_transforms on a mean probability [N, 3, D, H, W] -> (f32 0/1 [N, 3, D, H, W], tie masks [N, D, H, W]).
    Without either step it is the threshold alone."""
    mean = mean.numpy() if torch.is_tensor(mean) else np.asarray(mean)
    s = (mean >= thresh).astype(np.float32)
    ties = np.zeros((mean.shape[0],) + mean.shape[2:], dtype=np.uint8)
    if not (clean_on or replace_on):
        return s, ties
    out = np.empty_like(s)
    for n in range(mean.shape[0]):
        lab = to_labels(s[n])
        if clean_on:
            lab = clean(lab, cleaning_threshold)
        if replace_on:
            lab, ties[n] = replace(lab, replace_threshold, axis=2)
        out[n] = to_channels(lab)
    return out, ties


def remove_background(img, seg):
    """utils/transforms.py:536-550: zero the predictions wherever every image channel is 0."""
    img = img.numpy() if torch.is_tensor(img) else np.asarray(img)
    return seg * (img != 0).any(1, keepdims=True).astype(np.float32)
