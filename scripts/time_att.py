"""Device-event timing of AttEquiUnet (brats21_amd.networks.AttEquiUnet), in the manner of scripts/time_refine.py: median of
`--calls` warm calls of
  * the pooled gate passes (csrc/cbam.hip) at the three pooled levels of width 48 on 2 x 4 x 128^3, bf16 -- 2 x 48 x 128^3,
    2 x 96 x 64^3, 2 x 192 x 32^3 -- beside the composition they replace, in the same run: brats_cbam_apply_pool against
    brats_cbam_apply + brats_maxpool2_fwd (with the index plane), brats_cbam_bwd_reduce_pool / _bwd_apply_pool against
    brats_maxpool2_bwd_idx + brats_cbam_bwd_reduce / _bwd_apply (per pass: event pairs around the entry points), and whole
    cbam_fwd / cbam_bwd calls both ways;
  * the training step (bf16, fused Dice, Ranger2020, eager and as one hipGraph) of AttEquiUnet with fold_gate_pool on and off
    beside EquiUnet (--norm instance) at the same width: the whole-step cost of the six gates;
  * ops.probe_box in the same process: what the box delivers on the day.

    python scripts/time_att.py [--calls 20] [--patch 128] [--width 48] [--json profiles/att_time.json] [--no-step]"""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from brats21_amd import _lib, ops  # noqa: E402
from brats21_amd.networks import AttEquiUnet, EquiUnet  # noqa: E402


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


def gate_params(c, dev):
    ch = c // 16
    return [torch.randn((ch, c), device=dev) * (2.0 / ch) ** 0.5, torch.zeros(ch, device=dev), torch.randn((c, ch), device=dev) * (2.0 / c) ** 0.5,
            torch.zeros(c, device=dev), torch.randn((1, 2, 7, 7, 7), device=dev) * (2.0 / 343) ** 0.5, torch.ones(1, device=dev),
            torch.zeros(1, device=dev)]


def level_times(dev, c, size, calls, res):
    """One pooled level: [N, D, H, W, C] bf16."""
    n, (d, h, w) = 2, size
    tag = f"c{c}_{d}"
    x = torch.randn((n, d, h, w, c), device=dev).relu().bfloat16()
    p = gate_params(c, dev)
    d_skip = torch.randn((n, d, h, w, c), device=dev).bfloat16()
    d_pooled = torch.randn((n, d // 2, h // 2, w // 2, c), device=dev).bfloat16()
    l, code, st = _lib.lib(), _lib.BF16, None
    with torch.no_grad():
        out, pooled, sv = ops.cbam_fwd(x, *p, save=True, pool=True)
        out_c, sv_c = ops.cbam_fwd(x, *p, save=True)
        ops.maxpool2(out_c, want_argmax=True)
        dout = ops.maxpool2_bwd(out_c, d_pooled, dx_skip=d_skip)
        assert torch.equal(out, out_c) and torch.equal(sv.pidx, out_c._pool_argmax)
        # whole calls
        res[f"{tag}_fwd_fused_ms"] = time_calls(lambda: ops.cbam_fwd(x, *p, save=True, pool=True), calls)
        res[f"{tag}_fwd_composed_ms"] = time_calls(lambda: ops.maxpool2(ops.cbam_fwd(x, *p, save=True)[0], want_argmax=True), calls)
        res[f"{tag}_bwd_fused_ms"] = time_calls(lambda: ops.cbam_bwd(d_skip, x, sv, *p, d_pooled=d_pooled), calls)
        res[f"{tag}_bwd_composed_ms"] = time_calls(lambda: ops.cbam_bwd(ops.maxpool2_bwd(out_c, d_pooled, dx_skip=d_skip), x, sv_c, *p), calls)
        # the passes on their own (entry points, buffers of the calls above)
        f32 = dict(dtype=torch.float32, device=dev)
        v = d * h * w
        nb = l.brats_cbam_blocks(code, c, d, h, w)
        part = torch.empty(nb * n * (c + 2), **f32)
        dzn, asum, s12 = torch.empty((n, v), **f32), torch.empty((n, c), **f32), torch.empty((n, 2), **f32)
        dcomp, dpool = torch.randn((n, 2, v), **f32), torch.randn((n, 2, c), **f32)
        dx, idx = torch.empty_like(x), sv.pidx
        g, b = p[5], p[6]
        norm = (sv.scale.data_ptr(), sv.z.data_ptr(), sv.stats.data_ptr(), g.data_ptr(), b.data_ptr())
        shape = (code, n, c, d, h, w, st)

        def check(rc):
            _lib.check(rc, "time_att")

        passes = {
            "apply": lambda: check(l.brats_cbam_apply(x.data_ptr(), c, *norm, out.data_ptr(), c, *shape)),
            "maxpool2_fwd": lambda: check(l.brats_maxpool2_fwd(out.data_ptr(), c, pooled.data_ptr(), c, idx.data_ptr(), code, n, c, d, h, w, 0, st)),
            "apply_pool": lambda: check(l.brats_cbam_apply_pool(x.data_ptr(), c, *norm, out.data_ptr(), c, pooled.data_ptr(), c, idx.data_ptr(), *shape)),
            "maxpool2_bwd_idx": lambda: check(l.brats_maxpool2_bwd_idx(idx.data_ptr(), d_pooled.data_ptr(), c, d_skip.data_ptr(), c, dout.data_ptr(), c,
                                                                       code, n, c, d, h, w, 0, st)),
            "bwd_reduce": lambda: check(l.brats_cbam_bwd_reduce(dout.data_ptr(), c, x.data_ptr(), c, *norm, dzn.data_ptr(), part.data_ptr(),
                                                                asum.data_ptr(), s12.data_ptr(), *shape)),
            "bwd_reduce_pool": lambda: check(l.brats_cbam_bwd_reduce_pool(d_skip.data_ptr(), c, d_pooled.data_ptr(), c, idx.data_ptr(), x.data_ptr(), c,
                                                                          *norm, dzn.data_ptr(), part.data_ptr(), asum.data_ptr(), s12.data_ptr(), *shape)),
            "bwd_apply": lambda: check(l.brats_cbam_bwd_apply(dout.data_ptr(), c, *norm, dcomp.data_ptr(), sv.cidx.data_ptr(), dpool.data_ptr(),
                                                              sv.argvox.data_ptr(), dx.data_ptr(), c, *shape)),
            "bwd_apply_pool": lambda: check(l.brats_cbam_bwd_apply_pool(d_skip.data_ptr(), c, d_pooled.data_ptr(), c, idx.data_ptr(), *norm,
                                                                        dcomp.data_ptr(), sv.cidx.data_ptr(), dpool.data_ptr(), sv.argvox.data_ptr(),
                                                                        dx.data_ptr(), c, *shape)),
        }
        for name, fn in passes.items():
            res[f"{tag}_{name}_ms"] = time_calls(fn, calls)
    xb = x.numel() * 2  # bytes of one x-sized bf16 tensor
    res[f"{tag}_x_bytes"] = xb
    # bytes at x size (the pooled tensors are 1/8, the index plane 1/16 of it): fused apply_pool reads x, writes out + pooled + idx
    res[f"{tag}_apply_pool_TBps"] = round(xb * (2 + 1 / 8 + 1 / 16) / res[f"{tag}_apply_pool_ms"]["median"] / 1e9, 3)
    res[f"{tag}_bwd_reduce_pool_TBps"] = round(xb * (2 + 1 / 8 + 1 / 16) / res[f"{tag}_bwd_reduce_pool_ms"]["median"] / 1e9, 3)
    res[f"{tag}_bwd_apply_pool_TBps"] = round(xb * (2 + 1 / 8 + 1 / 16) / res[f"{tag}_bwd_apply_pool_ms"]["median"] / 1e9, 3)


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
        for name in ("equiunet", "att_fused", "att_composed"):
            torch.manual_seed(0)
            with contextlib.redirect_stdout(io.StringIO()):
                cls = EquiUnet if name == "equiunet" else AttEquiUnet
                m = cls(4, 3, feats, norm_layer="instance", act="relu", deep_supervision=True).to(dev).train()
                if name != "equiunet":
                    m.fold_gate_pool = name == "att_fused"
                opt = Ranger2020(m.parameters(), lr=1e-4, alpha=0.5, k=6, N_sma_threshhold=5, betas=(.95, 0.999), eps=1e-5, weight_decay=1e-5,
                                 capturable=graph)
            step = TrainStep(m, opt, amp=True)
            if graph:
                step = GraphedTrainStep(step, warmup=2)
            res[f"step_{name}{width}_{'graph' if graph else 'eager'}_ms"] = time_calls(lambda: step(x, t), calls)
            del m, opt, step
            torch.cuda.empty_cache()
    for kind in ("eager", "graph"):
        a, c, b = (res[f"step_{n}{width}_{kind}_ms"]["median"] for n in ("att_fused", "att_composed", "equiunet"))
        res[f"six_gates_{kind}_ms"] = round(a - b, 4)
        res[f"fold_gate_pool_saves_{kind}_ms"] = round(c - a, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--patch", type=int, default=128)
    ap.add_argument("--width", type=int, default=48)
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"shape": [2, 4] + [a.patch] * 3, "width": a.width, "calls": a.calls, "device": torch.cuda.get_device_name(0)}
    res["probe_box_before"] = ops.probe_box(dev)
    for lvl in range(3):
        level_times(dev, a.width << lvl, (a.patch >> lvl,) * 3, a.calls, res)
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
