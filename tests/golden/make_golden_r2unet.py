"""Generates tests/golden/r2unet_w8_*.npz: the reference's own ``R2Unet`` (networks/unet_family.py, imported under oracle/refshim.py)
at width 8 (features 8, 16, 32, 64), t = 2, 4 -> 3 channels, deep supervision, in training mode, on the 2 x 4 x 16 x 24 x 32 image of
tests/_unet_ref.py (seed 28) with the nested-sphere target and the closed-form weights, in the configurations group / relu and
instance / leakyrelu -- in the manner of make_golden_unet.py.

Run where the reference source is available only:  python tests/golden/make_golden_r2unet.py
The fixtures hold arrays and JSON metadata only: the reference's state-dict key list and shapes (the tests take the list from
here), the four heads (the deep ones at their own resolution: nearest up-sampling repeats every value, so ::s loses nothing), the
four-head Dice loss, every parameter's gradient norm, the gradients of at most 2048 elements; the reference's own float32 error
against tests/_r2unet_ref.py in float64 ("ref_err_*": the room the bars of tests/test_r2unet_gpu.py have); the same class in float64
("loss64", "d1_64" ::2, "grad_norms64", "grad64:*" for the gradients of at most 64 elements: what tests/test_r2unet_cpu.py holds the
restatement to); and "ref_bf16_dev": the mean |bf16 - f32| of the reference's d1 under torch.autocast("cpu", bfloat16).  The input
is not stored: it regenerates from the seed (tests/test_unet_cpu.py pins the regenerated image against a committed copy)."""
import contextlib
import copy
import io
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import refshim  # noqa: E402
import _r2unet_ref as R  # noqa: E402

refshim.install()
refshim._mod("monai.networks.nets", DynUNet=None)  # (networks/unet_family.py:503 imports the name for its DynUNet wrapper)
from networks.unet_family import R2Unet  # noqa: E402
from monai.losses import DiceLoss  # noqa: E402  (the stub)

OUT = os.path.dirname(os.path.abspath(__file__))
torch.set_num_threads(8)


def fixture(case):
    norm, act = case
    feats = [R.WIDTH * 2 ** i for i in range(4)]
    with contextlib.redirect_stdout(io.StringIO()):
        model = R2Unet(4, 3, feats, t=R.T, norm_layer=norm, act=act, deep_supervision=True)
        plain = R2Unet(4, 3, feats, t=R.T, norm_layer=norm, act=act, deep_supervision=False)
    ref_sd = model.state_dict()
    shapes = {k: tuple(v.shape) for k, v in ref_sd.items()}
    assert len(shapes) == 90 and list(plain.state_dict()) == list(shapes)[:84]
    sd = R.weights(shapes)
    model.load_state_dict(sd, strict=True)
    model.train()
    x, t = R.image(), R.target()
    heads = model(x)
    assert isinstance(heads, tuple) and len(heads) == 4 and all(h.shape == (R.BATCH, 3, *R.SIZE) for h in heads)
    crit = DiceLoss(include_background=True, sigmoid=True, softmax=False, squared_pred=True, jaccard=False, batch=True)  # src/definer.py:184-193
    loss = torch.mean(torch.stack([crit(h, t) for h in heads]))  # learning/engine.py:322-330
    loss.backward()
    out = {
        "meta": json.dumps({"width": R.WIDTH, "t": R.T, "norm": norm, "act": act, "batch": R.BATCH, "size": list(R.SIZE), "seed": 28,
                            "keys": list(shapes), "shapes": [list(s) for s in shapes.values()], "scales": list(R.SCALES)}),
        "loss": np.float64(loss.item()),
    }
    for i, (h, s) in enumerate(zip(heads, R.SCALES)):
        low = h.detach()[:, :, ::s, ::s, ::s]
        assert torch.equal(torch.nn.functional.interpolate(low, scale_factor=s, mode="nearest"), h.detach())
        out[f"d{i + 1}"] = low.numpy().copy()
    params = dict(model.named_parameters())
    names = list(params)
    assert names == list(shapes) and all(p.grad is not None for p in params.values())
    out["grad_norms"] = np.array([float(params[n].grad.double().norm()) for n in names])
    for n in names:
        if params[n].grad.numel() <= 2048:
            out["grad:" + n] = params[n].grad.numpy().copy()
    # the reference's own f32 error against the f64 restatement, in the measures of the bars of tests/test_r2unet_gpu.py: heads 1e-3
    # abs, loss 1e-4, gradient norms rtol 2e-3, small gradients 2e-3 of their maximum
    h64, loss64, g64 = R.run64(sd, x, t, case)
    out["ref_err_heads"] = np.float64(max(float((h.detach().double() - e).abs().max()) for h, e in zip(heads, h64)))
    out["ref_err_loss"] = np.float64(abs(loss.item() - loss64))
    out["ref_err_grad_rel"] = np.float64(max(float((params[n].grad.double() - g64[n]).norm() / g64[n].norm()) for n in names
                                             if float(g64[n].norm()) > 1e-9))
    # (a gradient that is zero in exact arithmetic -- a convolution bias in front of a per-channel normalisation -- has no relative
    #  measure: it is held to the absolute part of the bars)
    live = [n for n in names if float(g64[n].norm()) > 1e-9]
    out["ref_err_gnorm_rel"] = np.float64(max(abs(float(params[n].grad.double().norm()) / float(g64[n].norm()) - 1.0) for n in live))
    out["ref_err_grad_small"] = np.float64(max(float((params[n].grad.double() - g64[n]).abs().max() / g64[n].abs().max())
                                               for n in live if params[n].grad.numel() <= 2048))
    out["ref_err_grad_dead"] = np.float64(max([float(params[n].grad.abs().max()) for n in names if n not in live] or [0.0]))
    errs = {k: float(v) for k, v in out.items() if k.startswith("ref_err")}
    assert out["ref_err_heads"] < 2.5e-4 and out["ref_err_loss"] < 2.5e-5, errs
    assert out["ref_err_gnorm_rel"] < 2e-3 and out["ref_err_grad_small"] < 2e-3, errs
    # the reference class itself in float64: what tests/test_r2unet_cpu.py holds the restatement to (1e-12)
    model64 = copy.deepcopy(model).double()
    model64.zero_grad()
    res64 = model64(x.double())
    l64 = torch.mean(torch.stack([crit(h, t.double()) for h in res64]))
    l64.backward()
    p64 = dict(model64.named_parameters())
    assert abs(float(l64) - loss64) < 1e-12 and max(float((a.detach() - b).abs().max()) for a, b in zip(res64, h64)) < 1e-12
    assert all(float((p64[n].grad - g64[n]).abs().max()) <= 1e-12 * max(1.0, float(g64[n].abs().max())) for n in names)
    out["loss64"] = np.float64(float(l64))
    out["d1_64"] = res64[0].detach().numpy()[:, :, ::2, ::2, ::2].copy()
    out["grad_norms64"] = np.array([float(p64[n].grad.norm()) for n in names])
    for n in names:
        if p64[n].grad.numel() <= 64:
            out["grad64:" + n] = p64[n].grad.numpy().copy()
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
        rb = model(x)
    out["ref_bf16_dev"] = np.float64((rb[0].float() - heads[0].detach()).abs().mean())
    path = os.path.join(OUT, R.fname(case))
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < (1 << 20), (path, os.path.getsize(path))
    print(R.fname(case), os.path.getsize(path), "bytes;", len(names), "keys; loss", loss.item(), "d1 absmax", float(heads[0].abs().max()),
          errs, "bf16 dev", float(out["ref_bf16_dev"]), "dead gradients", [n for n in names if n not in live])


if __name__ == "__main__":
    for case in R.CASES:
        fixture(case)
