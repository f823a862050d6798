"""Device-event timing of brats21_amd.networks.R2Unet and of the pass it adds, in the manner of scripts/time_unet.py and
scripts/time_rrcnn.py:

  * passes: ops.affine_act_add(pool=True, want_argmax=True) -- brats_affine_act_add_pool_fwd -- beside the two passes it replaces
    (ops.affine_act_add, then ops.maxpool2(want_argmax=True)), bf16, at the three encoder shapes of R2Unet-48 on 2 x 4 x 128^3:
    2 x 48 x 128^3, 2 x 96 x 64^3, 2 x 192 x 32^3.  Same process, ALTERNATING over `--rounds` rounds with warm-up before every timed
    window.  Per form: the median of the round medians and the spread of the rounds ((max - min) / min); algorithmic bytes (3.125
    activations against 4.125: y, add, s, pooled / 8 + the re-read of s) and TB/s.  ``keeps_fused``: the one-pass form's median is
    below the two passes' by more than the larger of the two spreads -- the rule by which ops.POOL_FUSED_MIN_BYTES is set;
  * network: R2Unet-48, 2 x 4 x 128^3, bf16, group / relu, t = 2: inference forward (eval, no_grad), training forward, forward +
    backward (the sum of the four heads as the loss: no criterion in the figure); median of `--calls` after 3 warm-ups, the peak
    allocation of each, and beside them the sum of the block times of profiles/rrcnn_time.json (four encoder blocks + the 64^3
    decoder block: the 128^3 and 32^3 decoder blocks are not in that file, so the sum is a floor, not an estimate);
  * --passes-only: just the two forms, `--calls` times per shape, no timing -- the run to put under
    ``rocprofv3 --kernel-trace --stats --output-format csv -d DIR --``; --merge-trace DIR then adds the per-shape kernel times of
    that trace (the dispatches in launch order) to the JSON.

    python scripts/time_r2unet.py [--calls 20] [--rounds 3] [--json profiles/r2unet_time.json] [--passes-only] [--merge-trace DIR]
                                  [--no-network]"""
import argparse
import contextlib
import csv
import glob
import io
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from brats21_amd import ops  # noqa: E402
from brats21_amd.networks import R2Unet  # noqa: E402

SHAPES = [("enc1_48_128", 48, 128), ("enc2_96_64", 96, 64), ("enc3_192_32", 192, 32)]  # (tag, C, extent)
N, T, WIDTH, PATCH = 2, 2, 48, 128
KERNELS = ("affine_act_pool_kernel", "affine_act_add_kernel", "maxpool2")


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
    return float(np.median(times))


def pass_runs(dev, c, size):
    shape = (N, size, size, size, c)
    g = torch.Generator(device=dev).manual_seed(1)
    y, add = (torch.randn(shape, device=dev, generator=g).bfloat16() for _ in range(2))
    ss = torch.randn((N, c, 2), device=dev, generator=g)
    out = torch.empty(shape, device=dev, dtype=torch.bfloat16)

    def two_passes():
        ops.affine_act_add(y, ss, add, "relu", out=out)
        ops.maxpool2(out, want_argmax=True)

    return {"fused": lambda: ops.affine_act_add(y, ss, add, "relu", out=out, pool=True, want_argmax=True), "two_passes": two_passes}


def pass_times(dev, calls, rounds, res):
    for tag, c, size in SHAPES:
        runs = pass_runs(dev, c, size)
        meds = {k: [] for k in runs}
        with torch.no_grad():
            for _ in range(rounds):
                for k, fn in runs.items():
                    meds[k].append(time_calls(fn, calls))
        x = N * size ** 3 * c * 2  # bytes of one activation
        for k, v in meds.items():
            res[f"{tag}_{k}_ms"] = {"median": round(float(np.median(v)), 4), "rounds": [round(t, 4) for t in v],
                                    "spread": round((max(v) - min(v)) / min(v), 4)}
        for k, acts in (("fused", 3.125), ("two_passes", 4.125)):
            res[f"{tag}_{k}_bytes"] = int(acts * x)
            res[f"{tag}_{k}_TBps"] = round(acts * x / res[f"{tag}_{k}_ms"]["median"] / 1e9, 3)
        f, t = res[f"{tag}_fused_ms"], res[f"{tag}_two_passes_ms"]
        res[f"{tag}_fused_over_two_passes"] = round(f["median"] / t["median"], 4)
        res[f"{tag}_keeps_fused"] = bool(f["median"] < t["median"] * (1 - max(f["spread"], t["spread"])))
        del runs
        torch.cuda.empty_cache()


def network_times(dev, calls, res):
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        m = R2Unet(4, 3, [WIDTH * 2 ** i for i in range(4)], t=T, norm_layer="group", act="relu", deep_supervision=True).to(dev)
    m.precision = "bf16"
    x = torch.randn((N, 4) + (PATCH,) * 3, device=dev)

    def infer():
        with torch.no_grad():
            m(x)

    def train_fwd():
        return m(x)

    def fwd_bwd():
        m.zero_grad(set_to_none=True)
        sum(h.sum() for h in m(x)).backward()

    for name, fn, mode in (("infer_fwd", infer, False), ("train_fwd", train_fwd, True), ("fwd_bwd", fwd_bwd, True)):
        m.train(mode)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        res[f"r2unet{WIDTH}_{name}_ms"] = round(time_calls(fn, calls), 4)
        res[f"r2unet{WIDTH}_{name}_peak_MiB"] = int(torch.cuda.max_memory_allocated(dev) >> 20)
    blocks = os.path.join(ROOT, "profiles", "rrcnn_time.json")
    if os.path.exists(blocks):
        b = json.load(open(blocks))
        tags = ["enc1_4_48_128", "enc2_48_96_64", "enc3_96_192_32", "enc4_192_384_16", "dec_96_96_96_64"]
        for kind in ("fwd_infer", "fwd_train", "fwd_bwd"):
            res[f"rrcnn_blocks_sum_{kind}_ms"] = round(sum(b[f"{t}_{kind}_ms"] for t in tags), 4)


def merge_trace(res, trace_dir, calls):
    """Per-shape kernel times of the two forms from a rocprofv3 kernel trace of a --passes-only run: per shape `calls` dispatches of
    the one-pass kernel, then `calls` pairs (affine_act_add_kernel, the pooling kernel)."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {trace_dir}")
    rows = []
    for f in files:
        for r in csv.DictReader(open(f)):
            if any(k in r["Kernel_Name"] for k in KERNELS):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    if len(rows) != len(SHAPES) * 3 * calls:
        raise SystemExit(f"{len(rows)} dispatches of the pass kernels in the trace, expected {len(SHAPES) * 3 * calls}")
    i = 0
    for tag, c, size in SHAPES:
        x = N * size ** 3 * c * 2
        fused, pairs = rows[i:i + calls], rows[i + calls:i + 3 * calls]
        i += 3 * calls
        assert all("affine_act_pool_kernel" in r[2] for r in fused) and all("affine_act_pool_kernel" not in r[2] for r in pairs), tag
        skip = calls // 4  # (the first quarter: warm-up)
        f_us = float(np.median([(e - s) / 1e3 for s, e, _ in fused[skip:]]))
        a_us = float(np.median([(e - s) / 1e3 for s, e, _ in pairs[2 * skip::2]]))
        p_us = float(np.median([(e - s) / 1e3 for s, e, _ in pairs[2 * skip + 1::2]]))
        res[f"{tag}_fused_kernel_us"], res[f"{tag}_fused_kernel_TBps"] = round(f_us, 2), round(3.125 * x / f_us / 1e6, 3)
        res[f"{tag}_add_kernel_us"], res[f"{tag}_pool_kernel_us"] = round(a_us, 2), round(p_us, 2)
        res[f"{tag}_two_passes_kernel_us"] = round(a_us + p_us, 2)
        res[f"{tag}_two_passes_kernel_TBps"] = round(4.125 * x / (a_us + p_us) / 1e6, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--passes-only", action="store_true")
    ap.add_argument("--merge-trace", default=None)
    ap.add_argument("--no-network", action="store_true")
    a = ap.parse_args()
    if a.merge_trace:
        res = json.load(open(a.json))
        merge_trace(res, a.merge_trace, res["trace_calls"])
        json.dump(res, open(a.json, "w"), indent=1)
        print(json.dumps({k: v for k, v in res.items() if "kernel" in k}))
        return
    if not torch.cuda.is_available():
        raise SystemExit("time_r2unet.py measures on the GPU; there is none here")
    dev = torch.device("cuda", 0)
    if a.passes_only:
        with torch.no_grad():
            for _, c, size in SHAPES:
                runs = pass_runs(dev, c, size)
                for name in ("fused", "two_passes"):
                    for _ in range(a.calls):
                        runs[name]()
                torch.cuda.synchronize()
        return
    res = {"batch": N, "t": T, "width": WIDTH, "patch": PATCH, "storage": "bf16", "calls": a.calls, "rounds": a.rounds,
           "trace_calls": a.calls, "device": torch.cuda.get_device_name(0), "pool_fused_min_bytes": ops.POOL_FUSED_MIN_BYTES}
    pass_times(dev, a.calls, a.rounds, res)
    if not a.no_network:
        network_times(dev, a.calls, res)
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
