"""Device-event timing of the reference's post-processing chain (get_post_transforms with --cleaning_areas 20
--replace_value 300, the README's inference flags) on one BraTS-sized prediction: mean probability [1, 3, 160, 240, 240]
-> threshold -> labels -> clean -> replace -> channels, against the threshold alone.  Median of `--calls` warm calls.

    python scripts/time_postproc.py [--calls 30] [--json out.json]

The prediction is synthetic: a tumour (nested balls: edema, core, a small enhancing part) plus scattered false-positive
speckle that cleaning removes; its enhancing region is below the replacement threshold, so both steps do real work."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from brats21_amd.evaluate import get_post_transforms  # noqa: E402


def prediction(dev, d=160, h=240, w=240, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    z, y, x = torch.meshgrid(torch.arange(d), torch.arange(h), torch.arange(w), indexing="ij")
    r2 = (z - 80.0) ** 2 + (y - 110.0) ** 2 + (x - 130.0) ** 2
    wt, tc = r2 <= 30 ** 2, r2 <= 14 ** 2
    et = ((z - 84.0) ** 2 + (y - 104.0) ** 2 + (x - 126.0) ** 2) <= 3 ** 2           # ~120 voxels: rare at 300
    speckle = torch.rand((d, h, w), generator=g) < 2e-4
    want = torch.stack([tc | speckle, wt | speckle, et])[None]
    u = torch.rand(want.shape, generator=g)
    return torch.where(want, 0.5 + 0.5 * u, 0.5 * u).to(dev)


def time_calls(fn, x, calls, warm=3):
    for _ in range(warm):
        fn(x)
    times = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(x)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_postproc.py measures on the GPU only")
    dev = torch.device("cuda", 0)
    x = prediction(dev)
    both = get_post_transforms(argparse.Namespace(cleaning_areas=True, cleaning_areas_threshold=20, replace_value=True,
                                                  replace_value_threshold=300))
    plain = get_post_transforms(argparse.Namespace())
    clean = get_post_transforms(argparse.Namespace(cleaning_areas=True, cleaning_areas_threshold=20))
    replace = get_post_transforms(argparse.Namespace(replace_value=True, replace_value_threshold=300))
    res = {"shape": list(x.shape), "calls": a.calls}
    for name, fn in (("threshold_only", plain), ("clean_20", clean), ("replace_300", replace), ("both", both)):
        med, lo, hi = time_calls(fn, x, a.calls)
        res[name + "_ms"] = {"median": round(med, 4), "min": round(lo, 4), "max": round(hi, 4)}
    out = both(x)
    res["voxels_kept"] = int(out[0, 1].sum().item())
    res["voxels_predicted"] = int((x[0, 1] >= 0.5).sum().item())
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
