"""Device-event timing of the refinement stage (``--model equiunet_ref``): median of `--calls` warm calls of
  * the narrow-output convolution (csrc/conv_narrow.hip, ops.conv3d_narrow) at the stage's last layer, 2 x 48 x 128^3 -> 3 classes
    with bias and residual, beside the composition of older kernels it replaces, in the same run: ops.conv3d at cout = 8 (the
    class rows zero-padded) writing a padded 16-bit NDHWC tensor, then the strip + layout pass to f32 NCDHW, then the residual
    add; the same for the input-gradient use (weights packed PACK_DGRAD);
  * the training step (bf16, fused Dice, Ranger2020, eager and as one hipGraph) of equiunet_ref beside equiunet at width 48 on
    2 x 4 x 128^3 -- the stage's share of the step.

    python scripts/time_refine.py [--calls 20] [--patch 128] [--width 48] [--json out.json] [--no-step]"""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from brats21_amd import get_model, ops  # noqa: E402
from brats21_amd._lib import PACK_DGRAD, PACK_FWD  # noqa: E402


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
    return {"median": round(float(np.median(times)), 4), "min": round(float(np.min(times)), 4), "max": round(float(np.max(times)), 4)}


def kernel_times(dev, patch, width, k, dtype, calls, res):
    n, size = 2, (patch,) * 3
    x = torch.randn((n,) + size + (width,), device=dev).to(dtype)
    w = torch.randn((k, width, 3, 3, 3), device=dev) * 0.05
    bias = torch.randn(k, device=dev)
    add = torch.randn((n, k) + size, device=dev)
    kpad = 8 if k <= 8 else 16
    wpad = torch.zeros((kpad, width, 3, 3, 3), device=dev)
    wpad[:k] = w
    bpad = torch.zeros(kpad, device=dev)
    bpad[:k] = bias
    with torch.no_grad():
        for mode, wt, wtp, b, bp in ((PACK_FWD, w, wpad, bias, bpad),
                                     (PACK_DGRAD, w.transpose(0, 1).contiguous(), wpad.transpose(0, 1).contiguous(), None, None)):
            tag = "fwd" if mode == PACK_FWD else "dgrad"
            wn = ops.pack_weights_narrow(wt, mode)
            wp = ops.pack_weights(wtp, dtype, mode)

            def narrow():
                return ops.conv3d_narrow(x, wn, k, bias=b, add=add)

            def conv8():
                return ops.conv3d(x, wp, kpad, 3, 1, bias=bp)[0]

            def composed():
                return ops.ndhwc_to_ncdhw(conv8()[..., :k]) + add

            dev_abs = float((narrow() - composed()).abs().max())
            res[f"narrow_{tag}_ms"] = time_calls(narrow, calls)
            res[f"composed_{tag}_ms"] = time_calls(composed, calls)
            res[f"composed_{tag}_conv_only_ms"] = time_calls(conv8, calls)
            res[f"narrow_vs_composed_{tag}_max_abs"] = dev_abs  # (the composition rounds the convolution to 16 bits)
    voxels = n * patch ** 3
    res["narrow_bytes"] = voxels * (width * x.element_size() + 8 * k)  # x read once, add read, out written
    for tag in ("fwd", "dgrad"):
        res[f"narrow_{tag}_TBps"] = round(res["narrow_bytes"] / res[f"narrow_{tag}_ms"]["median"] / 1e9, 3)


def step_times(dev, patch, width, calls, res):
    from brats21_amd.engine import GraphedTrainStep, TrainStep
    from brats21_amd.optim import Ranger2020
    size = (patch,) * 3
    x = torch.randn((2, 4) + size, device=dev)
    z, y, xx = torch.meshgrid(*[torch.linspace(-1, 1, s, device=dev) for s in size], indexing="ij")
    r2 = z * z + y * y + xx * xx
    t = torch.stack([(r2 <= r * r).float() for r in (0.6, 0.4, 0.25)])[None].repeat(2, 1, 1, 1, 1).contiguous()
    for graph in (False, True):
        for name in ("equiunet", "equiunet_ref"):
            torch.manual_seed(0)
            with contextlib.redirect_stdout(io.StringIO()):
                m = get_model(argparse.Namespace(model=name, width=width, norm="group", act="relu", num_classes=3, dropout=0)).to(dev).train()
                opt = Ranger2020(m.parameters(), lr=1e-4, alpha=0.5, k=6, N_sma_threshhold=5, betas=(.95, 0.999), eps=1e-5, weight_decay=1e-5,
                                 capturable=graph)
            step = TrainStep(m, opt, amp=True)
            if graph:
                step = GraphedTrainStep(step, warmup=2)
            res[f"step_{name}{width}_{'graph' if graph else 'eager'}_ms"] = time_calls(lambda: step(x, t), calls)
            del m, opt, step
            torch.cuda.empty_cache()
    for kind in ("eager", "graph"):
        a, b = res[f"step_equiunet_ref{width}_{kind}_ms"]["median"], res[f"step_equiunet{width}_{kind}_ms"]["median"]
        res[f"stage_share_{kind}"] = round((a - b) / a, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--patch", type=int, default=128)
    ap.add_argument("--width", type=int, default=48)
    ap.add_argument("--classes", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"shape": [2, a.width] + [a.patch] * 3, "classes": a.classes, "calls": a.calls, "device": torch.cuda.get_device_name(0)}
    kernel_times(dev, a.patch, a.width, a.classes, torch.bfloat16, a.calls, res)
    torch.cuda.empty_cache()
    if not a.no_step:
        step_times(dev, a.patch, a.width, a.calls, res)
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
