"""Device-event timing of the flagship step's memory passes beside the convolutions, each one stand-alone at the shape it
runs at in `bench.py` (EquiUnet-48, 2 x 4 x 128^3, bf16): the x2 trilinear adjoint of the three decoder levels, the four
deep-supervision heads (forward up-sampling to 128^3 and its adjoint), the output head on the raw convolution output, the
x2 up-sampling into level 1 and normalise + act + pool.  Warm, median of `--calls` calls (HIP events around one call), with
the algorithmic bytes of the pass (every tensor read or written once) and the TB/s they give.

    python scripts/time_passes.py [--calls 30] [--json out.json] [--label NAME]

BRATS_HIP_LIB selects another build of the library (a same-box before / after, as scripts/ab_bench.sh does); the two
GroupNorm-backward reduce passes of the table need a taped layer around them and are read off a kernel trace of the step
instead (scripts/ab_profile.sh)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from brats21_amd import ops  # noqa: E402

N, K, F = 2, 3, 48  # batch, logit planes, base width


def time_call(fn, calls, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def act(dev, s, c, dtype=torch.bfloat16, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn((N, s, s, s, c), generator=g, device=dev, dtype=torch.float32).to(dtype)


def passes(dev):
    """[(name, callable, algorithmic bytes)]; the launches behind a call are in a kernel trace of this script, not here."""
    out = []
    # x2 adjoint: the gradient of the up-sampled half of a decoder level's concatenated input (a channel slice, pitch 2 C)
    for s, c in ((128, F), (64, 2 * F), (32, 4 * F)):
        cat = act(dev, s, 2 * c)
        dy = cat[..., c:]
        out.append((f"upsample_bwd_{s}to{s // 2}_c{c}", lambda dy=dy: ops.upsample_bwd(dy, 2), N * s ** 3 * c * 2 * (1 + 1 / 8)))
    # deep heads: (source edge, channels, scale) of bottom, bottom_2, up3, up2
    for name, s, c, sc in (("bottom", 16, 8 * F, 8), ("bottom2", 16, 4 * F, 8), ("up3", 32, 2 * F, 4), ("up2", 64, F, 2)):
        x = act(dev, s, c, seed=1)
        w = torch.randn((K, c, 1, 1, 1), device=dev) * 0.1
        b = torch.randn(K, device=dev)
        dout = torch.randn((N, K, 128, 128, 128), device=dev)
        low, full = N * K * s ** 3 * 4, N * K * 128 ** 3 * 4
        out.append((f"head_fwd_{name}_x{sc}", lambda x=x, w=w, b=b, sc=sc: ops.head(x, w, b, sc), x.numel() * 2 + 2 * low + full))
        out.append((f"head_bwd_{name}_x{sc}", lambda x=x, w=w, dout=dout, sc=sc: ops.head_bwd(x, w, dout, sc),
                    full + 2 * low + 2 * x.numel() * 2))
    # output head on the raw convolution output (GroupNorm + relu on load)
    y = act(dev, 128, F, seed=2)
    ss = torch.stack([torch.rand((N, F), device=dev) + 0.5, torch.randn((N, F), device=dev) * 0.1], -1).contiguous()
    w = torch.randn((K, F, 1, 1, 1), device=dev) * 0.1
    b = torch.randn(K, device=dev)
    out.append(("gn_head_fwd_128", lambda: ops.gn_head(y, ss, w, b, "relu"), y.numel() * 2 + N * K * 128 ** 3 * 4))
    # x2 up-sampling into level 1 (into the second half of the concatenated input) and normalise + act + pool at level 1
    src = act(dev, 64, F, seed=3)
    cat = torch.empty((N, 128, 128, 128, 2 * F), device=dev, dtype=torch.bfloat16)
    out.append(("upsample_fwd_64to128_c48", lambda: ops.upsample(src, 2, out=cat[..., F:]), src.numel() * 2 * 9))
    out.append(("affine_act_pool_128_c48", lambda: ops.affine_act_pool(y, ss, "relu", want_argmax=True),
                y.numel() * 2 * (2 + 1 / 8) + y.numel() / 8))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--json", default=None)
    ap.add_argument("--label", default=os.path.basename(os.environ.get("BRATS_HIP_LIB", "libbrats_hip.so")))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_passes.py measures on the GPU only")
    dev = torch.device("cuda", 0)
    res = {"label": a.label, "calls": a.calls, "shape": [N, 4, 128, 128, 128], "passes": {}}
    for name, fn, nbytes in passes(dev):
        med, lo, hi = time_call(fn, a.calls)
        res["passes"][name] = {"ms": round(med, 4), "min": round(lo, 4), "max": round(hi, 4), "MB": round(nbytes / 1e6, 1),
                               "TBps": round(nbytes / med / 1e9, 2)}
        print(f"{name:34s} {med:8.4f} ms  [{lo:.4f}, {hi:.4f}]  {nbytes / 1e6:8.1f} MB  {nbytes / med / 1e9:5.2f} TB/s", flush=True)
    rows = res["passes"]
    res["sum_ms"] = {k: round(sum(v["ms"] for n, v in rows.items() if n.startswith(k)), 4) for k in ("upsample_bwd", "head_fwd", "head_bwd")}
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
