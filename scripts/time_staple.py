"""Time of STAPLE fusion (csrc/staple.hip, ops.staple) at the reference's evaluation size, 240 x 240 x 160, for R = 10 (ten models)
and R = 160 (ten models x 16 TTA passes) synthetic raters (the recipe of tests/_staple_ref.py make_raters, drawn on the device:
jittered spheres, 1 % of the voxels flipped per rater -- with 160 raters four voxels in five carry a vote, far more than in a
real ensemble), three channels with different draws, beside the numpy float64 restatement of ITK's filter on the same input
(one channel, one CPU thread, as SimpleITK's STAPLEImageFilter runs in the reference).

Per R: time to pack one rater's three channels (f32 maps, the first add left out), wall time of ops.staple for the three channels (host loop and done-flag reads
included; median of --calls), the same per channel, the iterations per channel, the chunk length the host loop ran with, and
the time of one iteration's two launches from a capped run.  The oracle is timed on channel 0 only, for --oracle-iterations
iterations (it needs minutes at R = 160), and reported per iteration and extrapolated to the channel's iteration count.
Nothing is asserted about the times.

    python scripts/time_staple.py [--calls 5] [--json profiles/staple_time.json] [--size 240 240 160] [--raters 10 160]
    python scripts/time_staple.py --calls 1 --oracle-iterations 0     # without the oracle: for a kernel trace
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _staple_ref as R  # noqa: E402
from brats21_amd import ops  # noqa: E402


def wall(fn, calls):
    fn()
    times = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def device_rater(shape, gen, dev):
    """One rater [1, 3, *shape] f32 0 / 1: per channel a sphere of radius 0.3 min(shape) (x 1 + N(0, 0.1)), centre jittered by
    N(0, 1 voxel), every voxel flipped with probability 0.01."""
    axes = [torch.arange(s, dtype=torch.float32, device=dev) for s in shape]
    out = torch.empty((1, 3) + shape, dtype=torch.float32, device=dev)
    for c in range(3):
        jit = torch.randn(4, generator=gen, device=dev)
        r2 = sum(((axes[a] - (shape[a] - 1) / 2.0 - jit[a]) ** 2).reshape([-1 if b == a else 1 for b in range(3)]) for a in range(3))
        rad = 0.3 * min(shape) * (1.0 + 0.1 * jit[3])
        out[0, c] = ((r2 <= rad * rad) ^ (torch.rand(shape, generator=gen, device=dev) < 0.01)).float()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--size", type=int, nargs=3, default=[240, 240, 160])
    ap.add_argument("--raters", type=int, nargs="+", default=[10, 160])
    ap.add_argument("--oracle-iterations", type=int, default=2)
    ap.add_argument("--json")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    shape = tuple(args.size)
    out = {"shape": list(shape), "channels": 3, "chunk": ops.STAPLE_CHUNK, "device": torch.cuda.get_device_name(0)}
    for raters in args.raters:
        pk = ops.StaplePacker((1, 3) + shape, raters, dev)
        d0 = None
        pack_s = 0.0
        gen = torch.Generator(device=dev).manual_seed(7000 + raters)
        for j in range(raters):  # one rater at a time: the ensemble is never in memory as a whole
            t = device_rater(shape, gen, dev)
            if d0 is None:
                d0 = np.empty((raters,) + shape, dtype=np.uint8)  # channel 0 for the oracle
            d0[j] = t[0, 0].to(torch.uint8).cpu().numpy()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pk.add(t)
            torch.cuda.synchronize()
            pack_s += (time.perf_counter() - t0) if j else 0.0  # (the first add allocates and zeroes the planes)
        seg, info = ops.staple(pk)
        its = info["iterations"][0].tolist()
        med, lo, hi = wall(lambda: ops.staple(pk), args.calls)
        cap = 8
        capped, _, _ = wall(lambda: ops.staple(pk, max_iterations=cap, chunk=cap), args.calls)
        one, _, _ = wall(lambda: ops.staple(pk, max_iterations=1, chunk=1), args.calls)
        rec = {"pack_ms_per_rater": round(1e3 * pack_s / max(raters - 1, 1), 3), "staple_ms_3_channels": round(1e3 * med, 2),
               "staple_ms_min_max": [round(1e3 * lo, 2), round(1e3 * hi, 2)], "staple_ms_per_channel": round(1e3 * med / 3, 2),
               "iterations": its, "host_reads": info["host_reads"], "chunk": info["chunk"],
               "ms_per_iteration_3_channels": round(1e3 * (capped - one) / (cap - 1), 3),
               "voxels_marked_fraction": [round(1.0 - float((pk.bits[c] == 0).all(0).double().mean()), 4) for c in range(3)],
               "bits_MB": round(pk.bits.numel() * 4 / 1e6, 1)}
        if args.oracle_iterations < 1:
            out[f"R={raters}"] = rec
            print(f"R={raters}", rec, flush=True)
            continue
        t0 = time.perf_counter()
        w, p, q, it, g = R.staple(d0, max_iterations=args.oracle_iterations)
        oracle_s = time.perf_counter() - t0
        rec["oracle_iterations_timed"] = args.oracle_iterations
        rec["oracle_s_per_iteration_1_channel"] = round(oracle_s / args.oracle_iterations, 2)
        rec["oracle_s_per_channel_extrapolated"] = round(oracle_s / args.oracle_iterations * max(its[0], 1), 1)
        # the capped oracle against the capped kernels on channel 0: the same check as tests/test_staple_gpu.py, at full size
        _, ci = ops.staple(pk, max_iterations=args.oracle_iterations)
        rec["max_abs_dp_dq_vs_oracle_capped"] = float(max(np.abs(ci["p"][0, 0].cpu().numpy() - p).max(), np.abs(ci["q"][0, 0].cpu().numpy() - q).max()))
        rec["prior_equal"] = bool(float(ci["prior"][0, 0]) == g)
        out[f"R={raters}"] = rec
        print(f"R={raters}", rec, flush=True)
        del pk, seg, info, d0
        torch.cuda.empty_cache()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        json.dump(out, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
