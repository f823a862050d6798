"""Device-event timing of the nearest-neighbour up-sampling kernels (csrc/nearest.hip) and of Unet (brats21_amd.networks.Unet,
``--model modified_unet``), in the manner of scripts/time_att.py: median of `--calls` warm calls of
  * ops.upsample_nearest / ops.upsample_nearest_bwd at the three decoder shapes of width 48 on 2 x 4 x 128^3, bf16 -- coarse
    2 x 384 x 16^3, 2 x 192 x 32^3, 2 x 96 x 64^3 -- beside the trilinear ops.upsample / ops.upsample_bwd at the same shapes in the same
    run.  The trilinear kernels move the same bytes with more arithmetic: they are the yardstick, timed in TWO rounds around the
    nearest kernels so that their own repeat-to-repeat spread is on record.  Per kernel: time, algorithmic bytes (coarse tensor +
    fine tensor, each once), TB/s, and the fraction of ops.probe_box's read + write stream bandwidth in the same process;
  * ops.planes_nearest / planes_nearest_bwd on the deep-head logits (2 x 3 planes, x2 / x4 / x8 up to 128^3);
  * the conv-bias gradient both ways at the 128^3 shape: ops.channel_dot against conv3d_wgrad(want_dbias=True) minus the same call
    without the bias;
  * the training step (bf16, fused Dice, Ranger2020, eager and as one hipGraph) of Unet beside EquiUnet at the same width and norm.

    python scripts/time_unet.py [--calls 20] [--patch 128] [--width 48] [--json profiles/unet_time.json] [--no-step]"""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from brats21_amd import ops  # noqa: E402
from brats21_amd.networks import EquiUnet, Unet  # noqa: E402


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


def level_times(dev, c, size, calls, stream_tbps, res):
    """One decoder level: coarse [2, D, H, W, C] bf16 <-> fine [2, 2D, 2H, 2W, C]."""
    n, (d, h, w) = 2, size
    tag = f"c{c}_{d}"
    x = torch.randn((n, d, h, w, c), device=dev).bfloat16()
    dy = torch.randn((n, 2 * d, 2 * h, 2 * w, c), device=dev).bfloat16()
    add = torch.randn((n, d, h, w, c), device=dev).bfloat16()
    out, dx = torch.empty_like(dy), torch.empty_like(x)
    nbytes = (x.numel() + dy.numel()) * 2
    runs = {
        "trilinear_fwd": lambda: ops.upsample(x, 2, out=out),
        "nearest_fwd": lambda: ops.upsample_nearest(x, 2, out=out),
        "trilinear_bwd": lambda: ops.upsample_bwd(dy, 2, out=dx),
        "nearest_bwd": lambda: ops.upsample_nearest_bwd(dy, 2, out=dx),
        "trilinear_bwd_add": lambda: ops.upsample_bwd(dy, 2, add=add, out=dx),
        "nearest_bwd_add": lambda: ops.upsample_nearest_bwd(dy, 2, add=add, out=dx),
    }
    with torch.no_grad():
        for rnd in (1, 2):  # the yardstick before and after: its own spread
            for name, fn in runs.items():
                if rnd == 1 or name.startswith("trilinear"):
                    res[f"{tag}_{name}_ms" + ("" if rnd == 1 else "_again")] = time_calls(fn, calls)
    res[f"{tag}_bytes"] = nbytes
    for name in runs:
        ms = res[f"{tag}_{name}_ms"]["median"]
        tb = (nbytes + (add.numel() * 2 if name.endswith("add") else 0)) / ms / 1e9
        res[f"{tag}_{name}_TBps"] = round(tb, 3)
        res[f"{tag}_{name}_frac_of_stream"] = round(tb / stream_tbps, 3)
    for kind in ("fwd", "bwd", "bwd_add"):
        a, b = res[f"{tag}_trilinear_{kind}_ms"]["median"], res[f"{tag}_trilinear_{kind}_ms_again"]["median"]
        res[f"{tag}_{kind}_yardstick_spread"] = round(abs(a - b) / min(a, b), 4)
        res[f"{tag}_{kind}_nearest_over_trilinear"] = round(res[f"{tag}_nearest_{kind}_ms"]["median"] / min(a, b), 4)


def planes_times(dev, patch, calls, res):
    for s in (2, 4, 8):
        low = torch.randn((2, 3) + (patch // s,) * 3, device=dev)
        dout = torch.randn((2, 3) + (patch,) * 3, device=dev)
        nbytes = (low.numel() + dout.numel()) * 4
        for name, fn in (("fwd", lambda: ops.planes_nearest(low, s)), ("bwd", lambda: ops.planes_nearest_bwd(dout, s))):
            res[f"planes_x{s}_{name}_ms"] = time_calls(fn, calls)
            res[f"planes_x{s}_{name}_TBps"] = round(nbytes / res[f"planes_x{s}_{name}_ms"]["median"] / 1e9, 3)


def dbias_times(dev, c, patch, calls, res):
    """The gradient of a convolution bias at the 128^3 level: sum over voxels of dy [2, 128^3, c]."""
    x = torch.randn((2,) + (patch,) * 3 + (c,), device=dev).bfloat16()
    dy = torch.randn_like(x)
    with torch.no_grad():
        res["dbias_channel_dot_ms"] = time_calls(lambda: ops.channel_dot(dy).sum(0), calls)
        res["wgrad_ms"] = time_calls(lambda: ops.conv3d_wgrad(x, dy, 3, 1), calls)
        res["wgrad_with_dbias_ms"] = time_calls(lambda: ops.conv3d_wgrad(x, dy, 3, 1, want_dbias=True), calls)
    res["dbias_in_wgrad_ms"] = round(res["wgrad_with_dbias_ms"]["median"] - res["wgrad_ms"]["median"], 4)


def step_times(dev, patch, width, calls, res):
    from brats21_amd.engine import GraphedTrainStep, TrainStep
    from brats21_amd.optim import Ranger2020
    size = (patch,) * 3
    x = torch.randn((2, 4) + size, device=dev)
    z, y, xx = torch.meshgrid(*[torch.linspace(-1, 1, s, device=dev) for s in size], indexing="ij")
    r2 = z * z + y * y + xx * xx
    t = torch.stack([(r2 <= r * r).float() for r in (0.6, 0.4, 0.25)])[None].repeat(2, 1, 1, 1, 1).contiguous()
    feats = [width * 2 ** i for i in range(4)]
    for graph in (False, True):
        for name in ("equiunet", "unet"):
            torch.manual_seed(0)
            with contextlib.redirect_stdout(io.StringIO()):
                if name == "equiunet":
                    m = EquiUnet(4, 3, feats, norm_layer="group", act="relu", deep_supervision=True)
                else:
                    m = Unet(4, 3, feats, norm_layer="group", act="relu", deep_supervision=True)
                m = m.to(dev).train()
                opt = Ranger2020(m.parameters(), lr=1e-4, alpha=0.5, k=6, N_sma_threshhold=5, betas=(.95, 0.999), eps=1e-5, weight_decay=1e-5,
                                 capturable=graph)
            step = TrainStep(m, opt, amp=True)
            if graph:
                step = GraphedTrainStep(step, warmup=2)
            res[f"step_{name}{width}_{'graph' if graph else 'eager'}_ms"] = time_calls(lambda: step(x, t), calls)
            del m, opt, step
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--patch", type=int, default=128)
    ap.add_argument("--width", type=int, default=48)
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_unet.py measures on the GPU; there is none here")
    dev = torch.device("cuda", 0)
    res = {"shape": [2, 4] + [a.patch] * 3, "width": a.width, "calls": a.calls, "device": torch.cuda.get_device_name(0)}
    res["probe_box_before"] = ops.probe_box(dev)
    for lvl in (3, 2, 1):  # Up4, Up3, Up2: the coarse tensors
        level_times(dev, a.width << lvl, (a.patch >> lvl,) * 3, a.calls, res["probe_box_before"]["stream_TBps"], res)
        torch.cuda.empty_cache()
    planes_times(dev, a.patch, a.calls, res)
    dbias_times(dev, a.width, a.patch, a.calls, res)
    torch.cuda.empty_cache()
    if not a.no_step:
        step_times(dev, a.patch, a.width, a.calls, res)
    res["probe_box_after"] = ops.probe_box(dev)
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
