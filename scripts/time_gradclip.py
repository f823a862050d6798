"""Device-event timing of gradient clipping (csrc/gradclip.hip) on the parameter sets of EquiUnet-48 and EquiUnetASSPEvo-48:
global-norm clipping + adaptive gradient clipping as the step runs them (optim.clip_grad_norm_ then AGC.clip_(): 3 + 2
launches) and as one call (optim.clip_grad_norm_agc_: 3 launches), beside torch.nn.utils.clip_grad_norm_ + the reference's
per-tensor AGC loop (learning/lr_scheduler.py:198-213, restated in torch ops).  Median of `--calls` warm calls; the achieved
rate is bytes moved (stats pass 8 B/param, apply pass 8 B/param; the two-call form reads the gradient once more) over the time.

    python scripts/time_gradclip.py [--calls 30] [--json out.json]
    python scripts/time_gradclip.py --count 10     # only 10 calls of each of our forms: for a kernel trace (launches per call)
"""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from brats21_amd import get_model  # noqa: E402
from brats21_amd.optim import AGC, clip_grad_norm_, clip_grad_norm_agc_  # noqa: E402


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
    return {"median_ms": round(float(np.median(times)), 4), "min_ms": round(float(np.min(times)), 4), "max_ms": round(float(np.max(times)), 4)}


def unitwise_norm(x):
    if x.ndim <= 1:
        return torch.sum(x ** 2) ** 0.5
    dim = 0 if x.ndim in (2, 3) else list(range(1, x.ndim))
    return torch.sum(x ** 2, dim=dim, keepdim=True) ** 0.5


def torch_agc(params, clipping, eps):
    """the reference's loop, uploads included"""
    for p in params:
        param_norm = torch.max(unitwise_norm(p.detach()), torch.tensor(eps).to(p.device))
        grad_norm = unitwise_norm(p.grad.detach())
        max_norm = param_norm * clipping
        clipped = p.grad * (max_norm / torch.max(grad_norm, torch.tensor(1e-6).to(grad_norm.device)))
        p.grad.detach().data.copy_(torch.where(grad_norm > max_norm, clipped, p.grad))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--count", type=int, default=0)
    ap.add_argument("--json")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {}
    for model in ("equiunet", "equiunet_assp_evo"):
        with contextlib.redirect_stdout(io.StringIO()):
            m = get_model(argparse.Namespace(model=model, width=48, norm="group", act="relu", num_classes=3, dropout=0)).to(dev)
        params = list(m.parameters())
        gen = torch.Generator(device=dev).manual_seed(1)
        for p in params:
            p.grad = torch.randn(p.shape, generator=gen, device=dev) * 0.01
        n = sum(p.numel() for p in params)
        # max_norm far above the norm / clipping far above every ratio would skip nothing in the stats pass but the apply pass
        # returns early when there is nothing to scale: time the case in which both clip (gradients shrink a little per call)
        max_norm, clipping, eps = 1e-3, 1e-5, 1e-3
        agc = AGC(params, torch.optim.SGD(params, lr=0.0), clipping=clipping, eps=eps)

        def two_calls():
            clip_grad_norm_(params, max_norm)
            agc.clip_()

        def one_call():
            clip_grad_norm_agc_(params, max_norm, clipping, eps)

        def torch_ops():
            torch.nn.utils.clip_grad_norm_(params, max_norm)
            torch_agc(params, clipping, eps)

        if args.count:
            for _ in range(args.count):
                two_calls()
            for _ in range(args.count):
                one_call()
            torch.cuda.synchronize()
            print(f"{model}: {args.count} two-call and {args.count} one-call clips of {len(params)} tensors issued")
            continue
        res = {"tensors": len(params), "params": n}
        for name, fn, nbytes in (("clip_grad_norm_ + AGC.clip_ (5 launches)", two_calls, 28 * n), ("clip_grad_norm_agc_ (3 launches)", one_call, 16 * n),
                                 ("torch clip_grad_norm_ + torch-op AGC", torch_ops, None)):
            for p in params:  # every form starts from the same gradients
                p.grad.normal_(generator=gen).mul_(0.01)
            r = time_calls(fn, args.calls)
            if nbytes:
                r["MB_moved"] = round(nbytes / 1e6, 1)
                r["TB_per_s"] = round(nbytes / (r["median_ms"] * 1e-3) / 1e12, 3)
            res[name] = r
            print(model, name, r, flush=True)
        out[model] = res
    if args.json and out:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        json.dump(out, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
