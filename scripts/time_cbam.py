"""Times every pass of the CBAM block (ops.cbam_fwd / ops.cbam_bwd, csrc/cbam.hip) with ops.KernelTimer (HIP events on the launch
stream) at the six gate shapes of AttEquiUnet-48 on a 2 x 128^3 patch, bf16 storage, and prints one JSON line per shape: the mean
time of each pass, the bytes the pass has to move (computed from the shape: x-sized tensors at 2 bytes per element, planes of V
voxels at 4, the channel index plane at 2), the rate that gives and its fraction of the stream bandwidth ops.probe_box measures
on the same box in the same process.  One event pair per pass and call: for passes of a few microseconds (the 16^3 and 32^3 shapes)
the event overhead is comparable to the kernel and the figure is an upper bound.  DESIGN.md ("CBAM block") holds the table made from it.

    python scripts/time_cbam.py [--reps 20] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from brats21_amd import ops  # noqa: E402

SHAPES = ((2, 48, 128), (2, 96, 64), (2, 192, 32), (2, 384, 16), (2, 384, 16), (2, 192, 16))  # encoder1..4, bottom, bottom_2


def pass_bytes(n, c, v, tiles):
    """Bytes each pass must move at bf16 storage; the partials and [N, C] vectors are left out (below 1 % everywhere)."""
    xb, plane = 2 * n * c * v, 4 * n * v
    return {"cbam_pool": xb, "cbam_gate": 0, "cbam_compress": xb + 2 * plane + plane // 2, "cbam_spatial": 3 * plane,
            "cbam_apply": 2 * xb + plane, "cbam_bwd_reduce": 2 * xb + 2 * plane,
            "cbam_bwd_spatial": 6 * plane + 4 * n * tiles * 686, "cbam_bwd_chan": xb + 2 * plane + plane // 2, "cbam_bwd_gate": 0,
            "cbam_bwd_apply": 2 * xb + 3 * plane + plane // 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    box = ops.probe_box(dev, modes=())
    records = [{"box_stream_TBps": box["stream_TBps"]}]
    print(json.dumps(records[0]), flush=True)
    g = torch.Generator(device=dev).manual_seed(0)
    from brats21_amd import _lib
    for n, c, e in SHAPES:
        v, ch = e ** 3, c // 16
        x = (2 * torch.randn((n, e, e, e, c), device=dev, generator=g)).bfloat16()
        dout = torch.randn((n, e, e, e, c), device=dev, generator=g).bfloat16()
        params = [torch.randn(s, device=dev, generator=g) * k for s, k in (((ch, c), 0.2), ((ch,), 0.1), ((c, ch), 0.2), ((c,), 0.1),
                                                                          ((1, 2, 7, 7, 7), 0.05))]
        params += [torch.tensor([1.3], device=dev), torch.tensor([0.2], device=dev)]
        out = torch.empty_like(x)
        for _ in range(3):  # warm-up: code objects, allocator
            _, saved = ops.cbam_fwd(x, *params, out=out)
            ops.cbam_bwd(dout, x, saved, *params)
        ops.TIMER = ops.KernelTimer()
        for _ in range(args.reps):
            _, saved = ops.cbam_fwd(x, *params, out=out)
            ops.cbam_bwd(dout, x, saved, *params)
        summary, ops.TIMER = ops.TIMER.summary(), None
        need = pass_bytes(n, c, v, _lib.lib().brats_cbam_tiles(e, e, e))
        rec = {"shape": [n, c, e, e, e], "reps": args.reps, "passes": {}}
        for key, (_, mean_ms, _) in summary.items():
            b = need[key[0]]
            tbps = b / (mean_ms * 1e-3) / 1e12
            rec["passes"][key[0]] = {"ms": round(mean_ms, 4), "MB": round(b / 1e6, 2), "TBps": round(tbps, 3),
                                     "frac_of_box_stream": round(tbps / box["stream_TBps"], 3)}
        fwd = sum(p["ms"] for k, p in rec["passes"].items() if "bwd" not in k)
        rec["forward_ms"], rec["backward_ms"] = round(fwd, 4), round(sum(p["ms"] for p in rec["passes"].values()) - fwd, 4)
        records.append(rec)
        print(json.dumps(rec), flush=True)
        del x, dout, out, saved
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
