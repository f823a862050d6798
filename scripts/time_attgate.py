"""Device-event timing of the attention gate's passes (ops.attgate_fwd / ops.attgate_bwd, csrc/attgate.hip) at the three gate sizes of
a width-48 network on a 2 x 128^3 patch, bf16 storage: (C = 48, f_int = 24, 128^3), (96, 48, 64^3), (192, 96, 32^3).  Per pass: warm,
median [min, max] of `--calls` launches (ops.KernelTimer: HIP events around each launch of a training-mode forward + backward), the
algorithmic bytes of the pass (every tensor read or written once; X = an x-sized tensor, I = an f_int-sized one, P = an f32 plane)
and the TB/s they give; then the whole forward and backward with the timer off, and ops.probe_box's stream rate from the same
process, which is what the TB/s are to be read against.

Then the fused pass of R2AttUnet's skip gradients, brats_attgate_dx_unpool, against its two parents in the same process and on the
same tensors: brats_attgate_dx (reads 2X + P, writes X), brats_maxpool2_bwd_idx with dx as its skip gradient (reads X + X/8 + the
arg-max bytes A = X/16 in bf16, writes X), the two queued behind each other inside ONE event pair, and the fused pass (reads 2X + P
+ X/8 + A, writes X).  Event pairs around the library entry points themselves (no wrapper code between the events), median [min,
max] of `--calls` launches each.

    python scripts/time_attgate.py [--calls 30] [--json out.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from brats21_amd import ops  # noqa: E402

N = 2
SIZES = ((48, 24, 128), (96, 48, 64), (192, 96, 32))  # (C = f_g = f_l, f_int, edge)
TRAFFIC = {  # pass -> (X, I, P) tensors moved
    "attgate_psi_fwd": (0, 2, 1), "attgate_apply_fwd": (2, 0, 1), "attgate_apply_bwd": (2, 0, 2), "attgate_psi_bwd_stats": (0, 2, 2),
    "attgate_psi_bwd_apply": (0, 4, 2), "attgate_dx": (3, 0, 1), "conv_igemm": (1, 1, 0), "conv_wgrad": (1, 1, 0)}


def setup(dev, c, fi, s, dtype=torch.bfloat16):
    gen = torch.Generator(device=dev).manual_seed(0)

    def rn(*shape, scale=1.0):
        return torch.randn(shape, generator=gen, device=dev) * scale
    shapes = ((fi, c, 1, 1, 1), (fi,), (fi,), (fi,), (fi, c, 1, 1, 1), (fi,), (fi,), (fi,), (1, fi, 1, 1, 1), (1,), (1,), (1,))
    params = []
    for i, shp in enumerate(shapes):
        if i in (2, 6, 10):
            params.append(1.0 + rn(*shp, scale=0.1))
        elif len(shp) == 5:
            params.append(rn(*shp, scale=(2.0 / shp[1]) ** 0.5))
        else:
            params.append(rn(*shp, scale=0.2))
    g, x, dout = (rn(N, s, s, s, c).to(dtype) for _ in range(3))
    return params, g, x, dout


def step(params, g, x, dout):
    _, saved, _ = ops.attgate_fwd(g, x, params, "relu")
    ops.attgate_bwd(dout, saved, params)


def events(fn, calls, warm=3):
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
    return [round(float(v), 4) for v in (np.median(times), np.min(times), np.max(times))]


def fused_rows(dev, c, s, calls):
    """-> {row: {ms, min, max, MB, TBps}} of brats_attgate_dx_unpool and its parents at [N, s, s, s, c], bf16."""
    from brats21_amd import _lib
    gen = torch.Generator(device=dev).manual_seed(1)

    def rn(*shape):
        return torch.randn(shape, generator=gen, device=dev)
    skip, dout, t = (rn(N, s, s, s, c).to(torch.bfloat16) for _ in range(3))
    d_pooled = rn(N, s // 2, s // 2, s // 2, c).to(torch.bfloat16)
    ops.maxpool2(skip, want_argmax=True)
    idx, q = skip._pool_argmax, rn(N * s ** 3)
    st1 = torch.tensor([0.0, 1.0, 1.0, 0.0, 1.3, -0.2, 0.0, 0.0], device=dev)
    dx, out = torch.empty_like(dout), torch.empty_like(dout)
    l, st, code, vox = _lib.lib(), ops._stream(), _lib.BF16, s ** 3
    ptr = {k: v.data_ptr() for k, v in dict(dout=dout, t=t, q=q, st1=st1, idx=idx, dp=d_pooled, dx=dx, out=out).items()}

    def run_dx():
        _lib.check(l.brats_attgate_dx(ptr["dout"], c, ptr["t"], c, ptr["q"], ptr["st1"], ptr["dx"], c, code, N, vox, c, st), "attgate_dx")

    def run_unpool():
        _lib.check(l.brats_maxpool2_bwd_idx(ptr["idx"], ptr["dp"], c, ptr["dx"], c, ptr["out"], c, code, N, c, s, s, s, 0, st), "maxpool2_bwd_idx")

    def run_pair():
        run_dx()
        run_unpool()

    def run_fused():
        _lib.check(l.brats_attgate_dx_unpool(ptr["dout"], c, ptr["t"], c, ptr["q"], ptr["st1"], ptr["idx"], ptr["dp"], c, ptr["out"], c, code,
                                             N, c, s, s, s, st), "attgate_dx_unpool")
    run_pair()
    want = out.clone()
    run_fused()
    torch.cuda.synchronize()
    if not torch.equal(out, want):
        raise SystemExit("brats_attgate_dx_unpool does not give its parents' bits")
    x, p = N * vox * c * 2, N * vox * 4
    a = x // 16  # one arg-max byte per pooled element
    traffic = {"attgate_dx": 3 * x + p, "maxpool2_bwd_idx(dx_skip)": 2 * x + x // 8 + a, "dx + unpool, one event pair": 5 * x + p + x // 8 + a,
               "attgate_dx_unpool": 3 * x + p + x // 8 + a}
    rows = {}
    for name, fn in (("attgate_dx", run_dx), ("maxpool2_bwd_idx(dx_skip)", run_unpool), ("dx + unpool, one event pair", run_pair),
                     ("attgate_dx_unpool", run_fused)):
        med, lo, hi = events(fn, calls)
        rows[name] = {"ms": med, "min": lo, "max": hi, "MB": round(traffic[name] / 1e6, 1), "TBps": round(traffic[name] / med / 1e9, 2)}
        print(f"  {name:32s} {med:8.4f} ms  [{lo:.4f}, {hi:.4f}]  {rows[name]['MB']:8.1f} MB  {rows[name]['TBps']:5.2f} TB/s", flush=True)
    rows["sum_of_parents_ms"] = round(rows["attgate_dx"]["ms"] + rows["maxpool2_bwd_idx(dx_skip)"]["ms"], 4)
    print(f"  sum of the parents' medians {rows['sum_of_parents_ms']:.4f} ms; fused / sum "
          f"{rows['attgate_dx_unpool']['ms'] / rows['sum_of_parents_ms']:.3f}", flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_attgate.py measures on the GPU only")
    dev = torch.device("cuda", 0)
    res = {"calls": a.calls, "storage": "bf16", "sizes": {}}
    for c, fi, s in SIZES:
        params, g, x, dout = setup(dev, c, fi, s)
        ci, m = (fi + 7) // 8 * 8, N * s ** 3
        unit = {"X": m * c * 2, "I": m * ci * 2, "P": m * 4}
        for _ in range(3):  # warm: code objects, allocator
            step(params, g, x, dout)
        torch.cuda.synchronize()
        ops.TIMER = ops.KernelTimer()
        for _ in range(a.calls):
            step(params, g, x, dout)
        torch.cuda.synchronize()
        records, ops.TIMER = ops.TIMER.records, None
        rows = {}
        print(f"C = {c}, f_int = {fi}, {N} x {s}^3: X = {unit['X'] / 1e6:.1f} MB, I = {unit['I'] / 1e6:.1f} MB, P = {unit['P'] / 1e6:.1f} MB")
        for key, evs in records.items():
            ms = [p.elapsed_time(q) for p, q in evs]
            # (the convolutions: forward C -> f_int, input gradient f_int -> C, each twice per step -- W_g and W_x -- under one key)
            name = key[0] if key[0].startswith("attgate") else f"{key[0]}_{key[1]}to{key[2]}"
            nx, ni, np_ = TRAFFIC[key[0]]
            nbytes = nx * unit["X"] + ni * unit["I"] + np_ * unit["P"]
            med = float(np.median(ms))
            rows[name] = {"per_step": len(ms) // a.calls, "ms": round(med, 4), "min": round(float(np.min(ms)), 4),
                          "max": round(float(np.max(ms)), 4), "traffic": f"{nx} X + {ni} I + {np_} P", "MB": round(nbytes / 1e6, 1),
                          "TBps": round(nbytes / med / 1e9, 2)}
            r = rows[name]
            print(f"  {name:28s} x{r['per_step']} {r['ms']:8.4f} ms  [{r['min']:.4f}, {r['max']:.4f}]  {r['traffic']:16s} {r['MB']:8.1f} MB  "
                  f"{r['TBps']:5.2f} TB/s", flush=True)
        saved = ops.attgate_fwd(g, x, params, "relu")[1]
        fwd = events(lambda: ops.attgate_fwd(g, x, params, "relu"), a.calls)
        bwd = events(lambda: ops.attgate_bwd(dout, saved, params), a.calls)
        print(f"  whole forward {fwd[0]:.4f} ms [{fwd[1]:.4f}, {fwd[2]:.4f}], whole backward {bwd[0]:.4f} ms [{bwd[1]:.4f}, {bwd[2]:.4f}]", flush=True)
        res["sizes"][f"{c}_{fi}_{s}"] = {"bytes": unit, "passes": rows, "forward_ms": fwd, "backward_ms": bwd}
        del params, g, x, dout, saved
        torch.cuda.empty_cache()
        res["sizes"][f"{c}_{fi}_{s}"]["dx_unpool"] = fused_rows(dev, c, s, a.calls)
        torch.cuda.empty_cache()
    res["box"] = {k: v for k, v in ops.probe_box(dev, modes=()).items() if k != "probe"}
    print("box:", res["box"])
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
