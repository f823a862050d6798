"""Event-timed ops.head / ops.head_bwd (scale 1) at the flagship head shape, N x C x S^3 in a 16-bit type, for several class
counts in one process: time, algorithmic bytes (activations read once + logits written; backward: activations and logit
gradients read + dx written) and TB/s per K, and the f32 FMA time of the class dot products beside it.

    python scripts/time_heads.py [--classes 3 16] [--size 128] [--channels 48] [--batch 2] [--dtype bf16] [--ms 300]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from brats21_amd import ops  # noqa: E402


def timed(fn, ms):
    """Mean time of fn() in ms: warm, then enough repetitions to fill `ms` of device time between two events."""
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    reps = max(5, int(ms / max(e0.elapsed_time(e1), 1e-3)))
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", type=int, nargs="+", default=[3, 16])
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--channels", type=int, default=48)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--dtype", choices=["bf16", "fp16", "fp32"], default="bf16")
    ap.add_argument("--ms", type=float, default=300.0)
    a = ap.parse_args()
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[a.dtype]
    dev = torch.device("cuda:0")
    n, c, s = a.batch, a.channels, a.size
    vox = n * s ** 3
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn((n, s, s, s, c), generator=g, device=dev).to(dt)
    xbytes = x.numel() * x.element_size()
    for k in a.classes:
        w = (torch.randn((k, c, 1, 1, 1), generator=g, device=dev) * 0.2)
        b = torch.randn((k,), generator=g, device=dev) * 0.1
        dout = torch.randn((n, k, s, s, s), generator=g, device=dev)
        lbytes = dout.numel() * 4
        fwd_ms, fr = timed(lambda: ops.head(x, w, b, 1), a.ms)
        bwd_ms, br = timed(lambda: ops.head_bwd(x, w, dout, 1), a.ms)
        fma_tflops = 157.3  # MI355X vector f32 peak (FMA = 2 FLOP)
        print(json.dumps({
            "shape": [n, c, s, s, s], "dtype": a.dtype, "K": k,
            "fwd_ms": round(fwd_ms, 4), "fwd_bytes": xbytes + lbytes, "fwd_TBps": round((xbytes + lbytes) / fwd_ms * 1e-9, 3), "fwd_reps": fr,
            "bwd_ms": round(bwd_ms, 4), "bwd_bytes": 2 * xbytes + lbytes, "bwd_TBps": round((2 * xbytes + lbytes) / bwd_ms * 1e-9, 3), "bwd_reps": br,
            "bwd_vector_fma_ms_at_peak": round(2 * 2 * vox * c * k / (fma_tflops * 1e12) * 1e3, 4),
        }), flush=True)


if __name__ == "__main__":
    main()
