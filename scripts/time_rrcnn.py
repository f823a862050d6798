"""Device-event timing of the recurrent residual block (ops.rrcnn_fwd / ops.rrcnn_bwd, brats21_amd.networks.RRCNNblock) and of the
two streaming passes it adds, in the manner of scripts/time_unet.py, at the shapes R2Unet-48 will run the block at on 2 x 4 x 128^3
in bf16: encoder 4 -> 48 @128^3, 48 -> 96 @64^3, 96 -> 192 @32^3, 192 -> 384 @16^3 and the decoder block 96 | 96 -> 96 @64^3.

  * block: median of `--calls` warm calls of the inference forward (save=False), the training forward (save=True) and the
    training forward + backward, on NDHWC tensors;
  * passes: ops.affine_act_add beside the composition it replaces (ops.affine_act + torch's add of the stored tensors), and
    ops.grad_sum with 3 and 4 sources beside chained torch adds, in the same process, ALTERNATING over `--rounds` rounds with
    warm-up before every timed window.  Per pass: the median of the round medians, the spread of the rounds ((max - min) / min: the
    composition's own spread is the yardstick of a difference), algorithmic bytes (three tensors; nsrc + 1 tensors) and TB/s;
  * --passes-only: just the new passes, `--calls` times per shape, no timing -- the run to put under
    ``rocprofv3 --kernel-trace --output-format csv -d DIR --``; --merge-trace DIR then adds the per-shape kernel times of that
    trace (the dispatches in launch order, `--calls` per pass and shape) to the JSON.

    python scripts/time_rrcnn.py [--calls 20] [--rounds 3] [--json profiles/rrcnn_time.json] [--passes-only] [--merge-trace DIR]"""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from brats21_amd import ops  # noqa: E402
from brats21_amd.networks import RRCNNblock  # noqa: E402

# (tag, c1, c2, cout, size)
SHAPES = [("enc1_4_48_128", 4, 0, 48, 128), ("enc2_48_96_64", 48, 0, 96, 64), ("enc3_96_192_32", 96, 0, 192, 32),
          ("enc4_192_384_16", 192, 0, 384, 16), ("dec_96_96_96_64", 96, 96, 96, 64)]
N, T = 2, 2


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


def rounds_of(fns, calls, rounds):
    """{name: {"median", "rounds", "spread"}}: the functions timed in turn, `rounds` times over."""
    meds = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            meds[k].append(time_calls(fn, calls))
    return {k: {"median": round(float(np.median(v)), 4), "rounds": [round(t, 4) for t in v],
                "spread": round((max(v) - min(v)) / min(v), 4)} for k, v in meds.items()}


def pass_inputs(dev, cout, size):
    shape = (N, size, size, size, cout)
    g = torch.Generator(device=dev).manual_seed(1)
    ts = [torch.randn(shape, device=dev, generator=g).bfloat16() for _ in range(4)]
    ss = torch.randn((N, cout, 2), device=dev, generator=g)
    return ts, ss, torch.empty(shape, device=dev, dtype=torch.bfloat16)


def pass_runs(ts, ss, out):
    y, a, b, c = ts
    z = torch.empty_like(out)

    def composition():
        ops.affine_act(y, ss, "relu", out=z)
        torch.add(z, a, out=out)

    def chain3():
        torch.add(y, a, out=out)
        out.add_(b)

    def chain4():
        torch.add(y, a, out=out)
        out.add_(b)
        out.add_(c)

    return {"affine_act_add": lambda: ops.affine_act_add(y, ss, a, "relu", out=out), "affine_act_then_add": composition,
            "grad_sum3": lambda: ops.grad_sum(y, a, b, out=out), "chained_adds3": chain3,
            "grad_sum4": lambda: ops.grad_sum(y, a, b, c, out=out), "chained_adds4": chain4}


def block_times(dev, c1, c2, cout, size, calls, res, tag):
    cin = c1 + c2
    torch.manual_seed(0)
    m = RRCNNblock(cin, cout, "group", "relu", T).to(dev)
    params = tuple(m.parameters())
    cp = c1 if c1 % 8 == 0 else 8
    x = torch.randn((N, size, size, size, cp), device=dev).bfloat16()
    if cp != c1:
        x[..., c1:] = 0
    x2 = torch.randn((N, size, size, size, c2), device=dev).bfloat16() if c2 else None
    dout = torch.randn((N, size, size, size, cout), device=dev).bfloat16()

    def fwd_bwd():
        _, saved = ops.rrcnn_fwd(x, x2, params, 8, "relu", T, save=True)
        ops.rrcnn_bwd(dout, saved, params)

    with torch.no_grad():
        res[f"{tag}_fwd_infer_ms"] = round(time_calls(lambda: ops.rrcnn_fwd(x, x2, params, 8, "relu", T, save=False), calls), 4)
        res[f"{tag}_fwd_train_ms"] = round(time_calls(lambda: ops.rrcnn_fwd(x, x2, params, 8, "relu", T, save=True), calls), 4)
        res[f"{tag}_fwd_bwd_ms"] = round(time_calls(fwd_bwd, calls), 4)


def merge_trace(res, trace_dir, calls):
    """Per-shape kernel times of the two new kernels from a rocprofv3 kernel trace of a --passes-only run."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {trace_dir}")
    rows = []
    for f in files:
        for r in csv.DictReader(open(f)):
            if "affine_act_add_kernel" in r["Kernel_Name"] or "grad_sum_kernel" in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    want = len(SHAPES) * 3 * calls
    if len(rows) != want:
        raise SystemExit(f"{len(rows)} dispatches of the new kernels in the trace, expected {want}")
    i = 0
    for tag, _, _, cout, size in SHAPES:
        elems = N * size ** 3 * cout
        for name, tensors in (("affine_act_add", 3), ("grad_sum3", 4), ("grad_sum4", 5)):
            chunk = rows[i:i + calls]
            i += calls
            assert all(("affine_act_add" in c[2]) == (name == "affine_act_add") for c in chunk), (tag, name)
            us = float(np.median([(e - s) / 1e3 for s, e, _ in chunk[calls // 4:]]))  # (the first quarter: warm-up)
            res[f"{tag}_{name}_kernel_us"] = round(us, 2)
            res[f"{tag}_{name}_kernel_TBps"] = round(tensors * elems * 2 / us / 1e6, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--passes-only", action="store_true")
    ap.add_argument("--merge-trace", default=None)
    a = ap.parse_args()
    if a.merge_trace:
        res = json.load(open(a.json))
        merge_trace(res, a.merge_trace, res["trace_calls"])
        json.dump(res, open(a.json, "w"), indent=1)
        print(json.dumps({k: v for k, v in res.items() if "kernel" in k}))
        return
    if not torch.cuda.is_available():
        raise SystemExit("time_rrcnn.py measures on the GPU; there is none here")
    dev = torch.device("cuda", 0)
    if a.passes_only:
        for _, _, _, cout, size in SHAPES:
            runs = pass_runs(*pass_inputs(dev, cout, size))
            for name in ("affine_act_add", "grad_sum3", "grad_sum4"):
                for _ in range(a.calls):
                    runs[name]()
            torch.cuda.synchronize()
        return
    res = {"batch": N, "t": T, "storage": "bf16", "calls": a.calls, "rounds": a.rounds, "trace_calls": a.calls,
           "device": torch.cuda.get_device_name(0)}
    for tag, c1, c2, cout, size in SHAPES:
        block_times(dev, c1, c2, cout, size, a.calls, res, tag)
        torch.cuda.empty_cache()
        elems = N * size ** 3 * cout
        with torch.no_grad():
            tm = rounds_of(pass_runs(*pass_inputs(dev, cout, size)), a.calls, a.rounds)
        for name, r in tm.items():
            res[f"{tag}_{name}_ms"] = r
        for name, tensors in (("affine_act_add", 3), ("grad_sum3", 4), ("grad_sum4", 5)):
            res[f"{tag}_{name}_bytes"] = tensors * elems * 2
            res[f"{tag}_{name}_TBps"] = round(tensors * elems * 2 / tm[name]["median"] / 1e9, 3)
        for new, old in (("affine_act_add", "affine_act_then_add"), ("grad_sum3", "chained_adds3"), ("grad_sum4", "chained_adds4")):
            res[f"{tag}_{new}_over_composition"] = round(tm[new]["median"] / tm[old]["median"], 4)
            # faster by more than the spread of the composition's own repeats?
            res[f"{tag}_{new}_faster_beyond_spread"] = bool(tm[new]["median"] < min(tm[old]["rounds"]) * (1 - tm[old]["spread"]))
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
