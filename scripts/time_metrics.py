"""Device-event timing of the reference's validation metrics on the GPU: brats_metrics (Dice, Hausdorff distance 95,
sensitivity, specificity) on one BraTS-sized prediction / target pair [1, 3, 160, 240, 240].  Median of `--calls` warm
calls, in two cases built from seeded synthetic volumes:
  (a) compact: a tumour of nested balls, the prediction offset by a few voxels with slightly different radii;
  (b) speckle: (a) plus sparse false-positive speckle across the whole prediction volume, so the union's box is the
      whole volume (an uncleaned validation output).

    python scripts/time_metrics.py [--calls 30] [--json out.json] [--host]

--host also times the numpy / scipy restatement of MONAI's Hausdorff distance (tests/golden/make_golden_metrics.py's
get_mask_edges + distance_transform_edt + np.percentile) on the same masks, channel by channel, single-threaded."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from brats21_amd.metrics import brats_metrics  # noqa: E402

SHAPE = (160, 240, 240)


def balls(center, radii, shape=SHAPE):
    z, y, x = torch.meshgrid(*[torch.arange(s, dtype=torch.float32) for s in shape], indexing="ij")
    r2 = (z - center[0]) ** 2 + (y - center[1]) ** 2 + (x - center[2]) ** 2
    # channels TC / WT / ET: core inside the whole tumour, a small enhancing part inside the core
    return torch.stack([r2 <= radii[0] ** 2, r2 <= radii[1] ** 2, r2 <= radii[2] ** 2])[None].float()


def case(kind, seed=0, shape=SHAPE):
    """-> (pred, target) float32 0/1 [1, 3, D, H, W] on the CPU; kind "a" (compact) or "b" (speckle)."""
    target = balls((80.0, 110.0, 130.0), (14.0, 30.0, 6.0), shape)
    pred = balls((83.0, 107.0, 132.0), (13.0, 31.0, 5.0), shape)
    if kind == "b":
        g = torch.Generator().manual_seed(seed)
        speckle = (torch.rand((1, 3) + tuple(shape), generator=g) < 2e-4).float()
        speckle[..., 0, 0, 0] = 1
        speckle[..., -1, -1, -1] = 1
        pred = torch.maximum(pred, speckle)
    return pred, target


def time_calls(fn, calls, warm=3):
    for _ in range(warm):
        fn()
    times = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def host_hd95(pred, target):
    """seconds for the numpy / scipy restatement of MONAI's compute_hausdorff_distance(percentile=95), all channels"""
    from scipy.ndimage import binary_erosion, distance_transform_edt

    def edges(p, t):
        u = p | t
        idx = np.argwhere(u)
        lo, hi = idx.min(0), idx.max(0) + 1
        sl = tuple(slice(a, b) for a, b in zip(lo, hi))
        p, t = np.squeeze(p[sl]), np.squeeze(t[sl])
        return binary_erosion(p) ^ p, binary_erosion(t) ^ t

    def surf(a, b):
        return distance_transform_edt(~b)[a]

    p, t = pred.numpy() == 1, target.numpy() == 1
    t0 = time.perf_counter()
    for k in range(p.shape[1]):
        ep, et = edges(p[0, k], t[0, k])
        max(np.percentile(surf(ep, et), 95), np.percentile(surf(et, ep), 95))
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--json", default=None)
    ap.add_argument("--host", action="store_true")
    a = ap.parse_args()
    res = {"shape": [1, 3] + list(SHAPE), "calls": a.calls}
    for kind in ("a", "b"):
        pred, target = case(kind)
        r = {}
        if torch.cuda.is_available():
            dev = torch.device("cuda", 0)
            p, t = pred.to(dev), target.to(dev)
            med, lo, hi = time_calls(lambda: brats_metrics(p, t), a.calls)
            r["gpu_ms"] = {"median": round(med, 4), "min": round(lo, 4), "max": round(hi, 4)}
            r["values"] = {k: [round(float(v), 4) for v in x[0]] for k, x in brats_metrics(p, t).items()}
        if a.host:
            r["host_s_hd95_3ch"] = round(host_hd95(pred, target), 3)
            r["host_cores"] = os.cpu_count()
        res["case_" + kind] = r
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
