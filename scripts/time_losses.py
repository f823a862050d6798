"""Device-event timing of the distance transform and the distance-map criteria (csrc/edt.hip, csrc/dist_loss.hip) on a
training-sized batch [2, 3, 128, 128, 128]: median of `--calls` warm calls of
  * the transform alone: the target's field (f32 mask), the predicted field (arg-max one-hot + uint8 mask, truncated),
    the signed boundary map (both directions);
  * forward + backward of each criterion of definer.make_criterion for one head and for five heads (the deep-supervision
    count of EquiUnet), the target's field shared between the heads;
  * the EquiUnet-48 training step (bf16, Ranger2020, eager and as one hipGraph) with --criterion hd beside the fused-Dice
    step of the same run -- the comparison that matters.

  * the exclusive-class criterion losses.SoftmaxDiceCELoss (csrc/softmax_loss.hip) at [2, K, 128, 128, 128], K = 4 and 16:
    forward + backward over the main head + 4 deep heads beside the torch-eager composition of the same loss (softmax, one-hot,
    the Dice algebra, F.cross_entropy) on the same box, and the statistics and gradient kernels alone against their byte
    bounds (4K + 1 and 8K + 1 bytes per voxel).

  * the multi-label criteria losses.DiceCELoss, DiceFocalLoss, FocalLoss, TverskyLoss (csrc/sigmoid_loss.hip) at
    [2, K, 128, 128, 128], K = 3 and 16: the target pass, the statistics and gradient passes per term mask against their byte
    bounds (8K (+ 1) and 12K (+ 1) bytes per voxel), forward + backward of each criterion on one head beside the torch-eager
    composition of the same loss (tests/_sigmoid_losses_ref.py) on the same box.

    python scripts/time_losses.py [--calls 20] [--patch 128] [--json out.json] [--host] [--no-step] [--no-dist] [--no-softmax]
                                  [--no-sigmoid]

--host, where scipy is importable, also times what the reference does instead on every head (learning/losses.py:153-162):
device -> host copy, scipy.ndimage.distance_transform_edt per (sample, class), host -> device copy."""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from brats21_amd import definer, get_model, losses, ops, transforms  # noqa: E402


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


def tumour(n, size, dev):
    """[n, 3, *size] nested balls (TC / WT / ET), a different centre per sample."""
    z, y, x = torch.meshgrid(*[torch.arange(s, dtype=torch.float32, device=dev) for s in size], indexing="ij")
    out = []
    for i in range(n):
        c = [s * (0.45 + 0.1 * i) for s in size]
        r2 = (z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2
        out.append(torch.stack([r2 <= (0.12 * size[0]) ** 2, r2 <= (0.25 * size[0]) ** 2, r2 <= (0.05 * size[0]) ** 2]))
    return torch.stack(out).float()


def criterion(name):
    with contextlib.redirect_stdout(io.StringIO()):
        return definer.make_criterion(argparse.Namespace(criterion=name, num_classes=3))


def host_round_trip(target):
    """seconds for one head's target field the reference's way: to the host, scipy per (sample, class), back"""
    from scipy.ndimage import distance_transform_edt
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m = target.cpu().numpy()
    out = np.zeros_like(m)
    for n in range(m.shape[0]):
        for k in range(m.shape[1]):
            pos = m[n, k].astype(bool)
            if pos.any():
                out[n, k] = distance_transform_edt(pos)
    torch.tensor(out, device=target.device, dtype=torch.float32)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def step_times(dev, patch, calls, res):
    from brats21_amd.engine import GraphedTrainStep, TrainStep
    from brats21_amd.optim import Ranger2020
    size = (patch,) * 3
    x = torch.randn((2, 4) + size, device=dev)
    t = tumour(2, size, dev)
    for graph in (False, True):
        for name in ("dice", "hd"):
            torch.manual_seed(0)
            with contextlib.redirect_stdout(io.StringIO()):
                m = get_model(argparse.Namespace(model="equiunet", width=48, norm="group", act="relu", num_classes=3, dropout=0)).to(dev).train()
                opt = Ranger2020(m.parameters(), lr=1e-4, alpha=0.5, k=6, N_sma_threshhold=5, betas=(.95, 0.999), eps=1e-5, weight_decay=1e-5,
                                 capturable=graph)
            step = TrainStep(m, opt, criterion=None if name == "dice" else criterion(name), amp=True)
            if graph:
                step = GraphedTrainStep(step, warmup=2)
            res[f"step_equiunet48_{name}_{'graph' if graph else 'eager'}_ms"] = time_calls(lambda: step(x, t), calls)
            del m, opt, step
            torch.cuda.empty_cache()


def eager_softmax_dice_ce(x, y, smooth=1e-5):
    """what a user composes in torch without the criterion: DiceLoss(softmax, to_onehot_y, squared_pred, batch) + cross-entropy"""
    k = x.shape[1]
    valid = y != 255
    m = valid.unsqueeze(1).float()
    p = torch.softmax(x.float(), 1) * m
    t = torch.nn.functional.one_hot(torch.where(valid, y, 0), k).movedim(-1, 1).float() * m
    inter, den = (p * t).sum((0, 2, 3, 4)), t.sum((0, 2, 3, 4)) + (p * p).sum((0, 2, 3, 4))
    return (1.0 - (2.0 * inter + smooth) / (den + smooth)).mean() + torch.nn.functional.cross_entropy(x.float(), y, ignore_index=255)


def softmax_times(dev, patch, calls, res):
    from brats21_amd import _lib
    lib = _lib.lib()
    size = (patch,) * 3
    n, vox = 2, patch ** 3
    crit = losses.SoftmaxDiceCELoss()
    st = torch.cuda.current_stream().cuda_stream
    for k in (4, 16):
        g = torch.Generator(device=dev).manual_seed(k)
        y = torch.randint(0, k, (n,) + size, device=dev, generator=g)
        y[torch.rand((n,) + size, device=dev, generator=g) < 0.02] = 255
        heads = [(torch.randn((n, k) + size, device=dev, generator=g) * 3).requires_grad_(True) for _ in range(5)]

        def fwd_bwd(loss_fn):
            for h in heads:
                h.grad = None
            loss_fn().backward()
        res[f"softmax_dice_ce_k{k}_fwd_bwd_5head_ms"] = time_calls(
            lambda: fwd_bwd(lambda: losses.deep_supervision_prepared_loss(crit, (heads[0], heads[1:]), y)[0]), calls)
        res[f"softmax_dice_ce_k{k}_torch_eager_fwd_bwd_5head_ms"] = time_calls(
            lambda: fwd_bwd(lambda: torch.stack([eager_softmax_dice_ce(h, y) for h in heads]).mean()), calls)
        # the two streaming kernels alone on one head, against 4K + 1 and 8K + 1 bytes per voxel
        x, y8 = heads[0].detach(), y.to(torch.uint8)
        sums = torch.empty((n, 3 * k + 1), device=dev)
        ws = torch.empty(lib.brats_softmax_ws_floats(n, k), device=dev)
        coef = torch.full((n, 2 * k + 1), 1e-3, device=dev)
        dx = torch.empty_like(x)
        for name, per_voxel, fn in (
                ("stats", 4 * k + 1, lambda: lib.brats_softmax_stats(x.data_ptr(), y8.data_ptr(), sums.data_ptr(), ws.data_ptr(), n, k, vox, st)),
                ("grad", 8 * k + 1, lambda: lib.brats_softmax_grad(x.data_ptr(), y8.data_ptr(), coef.data_ptr(), dx.data_ptr(), n, k, vox, 1, st))):
            t = time_calls(fn, calls)
            t["bytes"] = per_voxel * n * vox
            t["tb_per_s"] = round(t["bytes"] / (t["median"] * 1e-3) / 1e12, 3)
            res[f"softmax_{name}_k{k}_1head_ms"] = t
        del heads, x, dx
        torch.cuda.empty_cache()


def sigmoid_times(dev, patch, calls, res):
    """the four multi-label criteria (csrc/sigmoid_loss.hip) at [2, K, patch^3], K = 3 and 16: the statistics and the gradient pass
    alone per term mask against 8K (+ 1) and 12K (+ 1) bytes per voxel, the target pass, forward + backward of each criterion on
    one head, and the plain-torch composition of the same loss (tests/_sigmoid_losses_ref.py) on the same box"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import _sigmoid_losses_ref as ref
    from brats21_amd import _lib
    lib = _lib.lib()
    size = (patch,) * 3
    n, vox = 2, patch ** 3
    st = torch.cuda.current_stream().cuda_stream
    kwargs = dict(include_background=True, sigmoid=True, softmax=False, squared_pred=True, reduction="mean")
    criteria = {"dice_ce": lambda: losses.DiceCELoss(batch=True, **kwargs), "dice_focal": lambda: losses.DiceFocalLoss(batch=False, **kwargs),
                "focal": lambda: losses.FocalLoss(gamma=2.0, reduction="mean"),
                "tversky": lambda: losses.TverskyLoss(include_background=True, sigmoid=True, softmax=False, alpha=0.5, beta=0.5, reduction="mean")}
    for k in (3, 16):
        g = torch.Generator(device=dev).manual_seed(k)
        r = torch.rand((n, 1) + size, device=dev, generator=g)
        t = (r < torch.arange(1, k + 1, device=dev).view(1, k, 1, 1, 1) / (k + 1.0)).float()  # nested binary channels
        x = (torch.randn((n, k) + size, device=dev, generator=g) * 3).requires_grad_(True)
        xd = x.detach()
        sums, tsums = torch.empty((n, 4 * k + 1), device=dev), torch.empty((n, k, 2), device=dev)
        ws = torch.empty(lib.brats_sigmoid_loss_ws_floats(n, k), device=dev)
        ymap = torch.empty((n,) + size, dtype=torch.uint8, device=dev)
        coef = torch.full((n, 4 * k + 1), 1e-3, device=dev)
        dx = torch.empty_like(xd)
        passes = [("target_prepare", 4 * k, lambda: lib.brats_sigmoid_target_prepare(t.data_ptr(), tsums.data_ptr(), None, ws.data_ptr(), n, k, vox, st)),
                  ("target_prepare_classmap", 4 * k + 1,
                   lambda: lib.brats_sigmoid_target_prepare(t.data_ptr(), tsums.data_ptr(), ymap.data_ptr(), ws.data_ptr(), n, k, vox, st))]
        for label, terms in (("dice", 0), ("focal", losses.SIG_FOCAL), ("ce", losses.SIG_CE)):
            ce = 1 if terms & losses.SIG_CE else 0
            passes.append((f"stats_{label}", 8 * k + ce, lambda terms=terms: lib.brats_sigmoid_loss_stats(
                xd.data_ptr(), t.data_ptr(), ymap.data_ptr(), sums.data_ptr(), ws.data_ptr(), n, k, vox, terms, 2.0, st)))
            passes.append((f"grad_{label}", 12 * k + ce, lambda terms=terms: lib.brats_sigmoid_loss_grad(
                xd.data_ptr(), t.data_ptr(), ymap.data_ptr(), coef.data_ptr(), dx.data_ptr(), n, k, vox, terms, 2.0, st)))
        for name, per_voxel, fn in passes:
            tm = time_calls(fn, calls)
            tm["bytes"] = per_voxel * n * vox
            tm["tb_per_s"] = round(tm["bytes"] / (tm["median"] * 1e-3) / 1e12, 3)
            res[f"sigmoid_{name}_k{k}_ms"] = tm

        def fwd_bwd(loss_fn):
            x.grad = None
            loss_fn().backward()
        for name, make in criteria.items():
            crit = make()
            res[f"{name}_k{k}_fwd_bwd_1head_ms"] = time_calls(lambda: fwd_bwd(lambda: crit(x, t)), calls)
            res[f"{name}_k{k}_torch_eager_fwd_bwd_1head_ms"] = time_calls(lambda: fwd_bwd(lambda: ref.CRITERIA[name](x, t)), calls)
        del x, xd, dx, t, r
        torch.cuda.empty_cache()


def dist_times(dev, size, a, res):
    t = tumour(2, size, dev)
    heads = [torch.randn((2, 3) + size, device=dev).requires_grad_(True) for _ in range(5)]
    oh = losses.sigmoid_one_hot(heads[0])
    res["edt_target_f32_ms"] = time_calls(lambda: ops.distance_transform_edt(t), a.calls)
    res["onehot_ms"] = time_calls(lambda: losses.sigmoid_one_hot(heads[0]), a.calls)
    res["edt_predicted_u8_ms"] = time_calls(lambda: ops.distance_transform_edt(oh, mode=2), a.calls)
    res["boundary_map_ms"] = time_calls(lambda: transforms.one_hot_to_dist(t), a.calls)
    dist = transforms.one_hot_to_dist(t)
    for name in ("hd", "dice_hd", "boundary", "dice_boundary"):
        c = criterion(name)
        label = [t, dist] if "boundary" in name else t
        for nh in (1, 5):
            def fwd_bwd():
                for h in heads:
                    h.grad = None
                losses.deep_supervision_prepared_loss(c, (heads[0], heads[1:nh]), label)[0].backward()
            res[f"{name}_fwd_bwd_{nh}head_ms"] = time_calls(fwd_bwd, a.calls)
    if a.host:
        try:
            import scipy  # noqa: F401
            res["host_scipy_round_trip_1head_target_s"] = round(host_round_trip(t), 3)
            res["host_scipy_round_trip_1head_prediction_s"] = round(host_round_trip(oh.float()), 3)
            res["host_cores"] = os.cpu_count()
        except ImportError:
            res["host_scipy_round_trip_1head_target_s"] = None
    del heads
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--patch", type=int, default=128)
    ap.add_argument("--json", default=None)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-dist", action="store_true", help="skip the distance-transform and distance-map criterion legs")
    ap.add_argument("--no-softmax", action="store_true", help="skip the exclusive-class criterion leg")
    ap.add_argument("--no-sigmoid", action="store_true", help="skip the dice_ce / dice_focal / focal / tversky leg")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    size = (a.patch,) * 3
    res = {"shape": [2, 3] + list(size), "calls": a.calls}
    if not a.no_dist:
        dist_times(dev, size, a, res)
    if not a.no_softmax:
        softmax_times(dev, a.patch, a.calls, res)
    if not a.no_sigmoid:
        sigmoid_times(dev, a.patch, a.calls, res)
    if not a.no_step:
        step_times(dev, a.patch, a.calls, res)
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
