"""Generates tests/golden/attunet_w8_*.npz and r2attunet_w8_*.npz: the reference's own ``AttUnet`` and ``R2AttUnet``
(networks/unet_family.py, imported under oracle/refshim.py) at width 8 (features 8, 16, 32, 64: Att2 has f_int 4), t = 2, 4 -> 3
channels, deep supervision, on the 2 x 4 x 16 x 24 x 32 image of tests/_unet_ref.py (seed 28) with the nested-sphere target and the
closed-form weights of tests/_attunet_ref.py (BatchNorm weights, biases and running buffers included), in the configurations group /
relu and instance / leakyrelu -- in the manner of make_golden_r2unet.py.

Run where the reference source is available only:  python tests/golden/make_golden_attunet.py
The fixtures hold arrays and JSON metadata only.  From ONE training-mode forward and backward: the reference's state-dict key list
and shapes (the tests take the list from here), the four heads (the deep ones at their own resolution), the four-head Dice loss,
every parameter's gradient norm, the gradients of at most 2048 elements, the nine BatchNorm buffers of each gate after that forward
("buf:*"); the reference's own float32 error against tests/_attunet_ref.py in float64 ("ref_err_*", "ref_err_buf:*" per buffer: the
room the bars of tests/test_attunet_gpu.py have); the same class in float64 ("loss64", "d1_64" ::2, "grad_norms64", "grad64:*" for the
gradients of at most 64 elements, "buf64:*": what tests/test_attunet_cpu.py holds the restatement to); "ref_bf16_dev": the mean |bf16 -
f32| of the reference's d1 under torch.autocast("cpu", bfloat16).  From an EVAL-mode forward with the loaded running buffers -- the
inference path --: the four heads ("eval_d1" .. "eval_d4", the deep ones at their own resolution), the reference's float32 error
there against the restatement ("ref_err_eval") and "eval_d1_64" ::2.  The input is not stored: it regenerates from the seed.  The
closed-form weight gain differs per configuration: tests/_attunet_ref.py, GAIN, says why and how each was chosen."""
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
import _attunet_ref as R  # noqa: E402

refshim.install()
refshim._mod("monai.networks.nets", DynUNet=None)  # (networks/unet_family.py:503 imports the name for its DynUNet wrapper)
from networks.unet_family import AttUnet, R2AttUnet  # noqa: E402
from monai.losses import DiceLoss  # noqa: E402  (the stub)

OUT = os.path.dirname(os.path.abspath(__file__))
torch.set_num_threads(8)


def _make(kind, case, deep_supervision=True):
    norm, act = case
    feats = [R.WIDTH * 2 ** i for i in range(4)]
    with contextlib.redirect_stdout(io.StringIO()):
        if kind == "attunet":
            return AttUnet(4, 3, feats, norm_layer=norm, act=act, deep_supervision=deep_supervision)
        return R2AttUnet(4, 3, feats, t=R.T, norm_layer=norm, act=act, deep_supervision=deep_supervision)


def fixture(kind, case):
    norm, act = case
    nkeys, nparams = R.NKEYS[kind]
    model = _make(kind, case)
    ref_sd = model.state_dict()
    shapes = {k: tuple(v.shape) for k, v in ref_sd.items()}
    assert len(shapes) == nkeys and list(_make(kind, case, False).state_dict()) == list(shapes)[:-6]
    sd = R.weights(shapes, R.GAIN.get((kind, case), 1.2))
    assert all(float(v.min()) > 0 for k, v in sd.items() if k.endswith("running_var"))
    buffers = [k for k in shapes if R.is_buffer(k)]
    assert len(buffers) == 27 == nkeys - nparams
    model.load_state_dict(sd, strict=True)
    model.train()
    x, t = R.image(), R.target()
    heads = model(x)
    assert isinstance(heads, tuple) and len(heads) == 4 and all(h.shape == (R.BATCH, 3, *R.SIZE) for h in heads)
    crit = DiceLoss(include_background=True, sigmoid=True, softmax=False, squared_pred=True, jaccard=False, batch=True)  # src/definer.py:184-193
    loss = torch.mean(torch.stack([crit(h, t) for h in heads]))  # learning/engine.py:322-330
    loss.backward()
    out = {
        "meta": json.dumps({"kind": kind, "width": R.WIDTH, "t": R.T, "norm": norm, "act": act, "batch": R.BATCH, "size": list(R.SIZE),
                            "seed": 28, "keys": list(shapes), "shapes": [list(s) for s in shapes.values()], "scales": list(R.SCALES),
                            "gain": R.GAIN.get((kind, case), 1.2)}),
        "loss": np.float64(loss.item()),
    }
    for i, (h, s) in enumerate(zip(heads, R.SCALES)):
        low = h.detach()[:, :, ::s, ::s, ::s]
        assert torch.equal(torch.nn.functional.interpolate(low, scale_factor=s, mode="nearest"), h.detach())
        out[f"d{i + 1}"] = low.numpy().copy()
    params = dict(model.named_parameters())
    names = list(params)
    assert names == [k for k in shapes if not R.is_buffer(k)] and len(names) == nparams and all(p.grad is not None for p in params.values())
    out["grad_norms"] = np.array([float(params[n].grad.double().norm()) for n in names])
    for n in names:
        if params[n].grad.numel() <= 2048:
            out["grad:" + n] = params[n].grad.numpy().copy()
    after = {k: v.detach().clone() for k, v in model.state_dict().items() if R.is_buffer(k)}
    for k in buffers:
        out["buf:" + k] = after[k].numpy().copy()
    # the reference's own f32 error against the f64 restatement, in the measures of the bars of tests/test_attunet_gpu.py: heads 1e-3
    # abs, loss 1e-4, gradient norms rtol 2e-3, small gradients 2e-3 of their maximum; the buffers: max abs per buffer
    h64, loss64, g64, b64 = R.run64(sd, x, t, kind, case)
    out["ref_err_heads"] = np.float64(max(float((h.detach().double() - e).abs().max()) for h, e in zip(heads, h64)))
    out["ref_err_loss"] = np.float64(abs(loss.item() - loss64))
    live = [n for n in names if float(g64[n].norm()) > 1e-9]
    out["ref_err_grad_rel"] = np.float64(max(float((params[n].grad.double() - g64[n]).norm() / g64[n].norm()) for n in live))
    # (a gradient that is zero in exact arithmetic -- a convolution bias in front of a per-channel normalisation or of a
    #  training-mode BatchNorm -- has no relative measure: it is held to the absolute part of the bars)
    out["ref_err_gnorm_rel"] = np.float64(max(abs(float(params[n].grad.double().norm()) / float(g64[n].norm()) - 1.0) for n in live))
    out["ref_err_grad_small"] = np.float64(max(float((params[n].grad.double() - g64[n]).abs().max() / g64[n].abs().max())
                                               for n in live if params[n].grad.numel() <= 2048))
    out["ref_err_grad_dead"] = np.float64(max([float(params[n].grad.abs().max()) for n in names if n not in live] or [0.0]))
    for k in buffers:
        assert k in b64
        if k.endswith("num_batches_tracked"):
            assert int(after[k]) == int(b64[k]) == 1
        else:
            out["ref_err_buf:" + k] = np.float64(float((after[k].double() - b64[k]).abs().max()))
    errs = {k: float(v) for k, v in out.items() if k.startswith("ref_err") and not k.startswith("ref_err_buf")}
    errs["worst"] = max(live, key=lambda n: abs(float(params[n].grad.double().norm()) / float(g64[n].norm()) - 1.0))
    assert out["ref_err_heads"] < 2.5e-4 and out["ref_err_loss"] < 2.5e-5, errs
    assert out["ref_err_gnorm_rel"] < 2e-3 and out["ref_err_grad_small"] < 2e-3, errs
    # the reference class itself in float64: what tests/test_attunet_cpu.py holds the restatement to (1e-12)
    model64 = _make(kind, case).double()
    model64.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}, strict=True)
    model64.train()
    res64 = model64(x.double())
    l64 = torch.mean(torch.stack([crit(h, t.double()) for h in res64]))
    l64.backward()
    p64 = dict(model64.named_parameters())
    s64 = model64.state_dict()
    assert abs(float(l64) - loss64) < 1e-12 and max(float((a.detach() - b).abs().max()) for a, b in zip(res64, h64)) < 1e-12
    assert all(float((p64[n].grad - g64[n]).abs().max()) <= 1e-12 * max(1.0, float(g64[n].abs().max())) for n in names)
    assert all(float((s64[k].double() - b64[k].double()).abs().max()) <= 1e-12 for k in buffers)
    out["loss64"] = np.float64(float(l64))
    out["d1_64"] = res64[0].detach().numpy()[:, :, ::2, ::2, ::2].copy()
    out["grad_norms64"] = np.array([float(p64[n].grad.norm()) for n in names])
    for n in names:
        if p64[n].grad.numel() <= 64:
            out["grad64:" + n] = p64[n].grad.numpy().copy()
    for k in buffers:
        out["buf64:" + k] = s64[k].detach().numpy().copy()
    # bf16 autocast, training mode as above, from the loaded buffers
    model.load_state_dict(sd, strict=True)
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
        rb = model(x)
    out["ref_bf16_dev"] = np.float64((rb[0].float() - heads[0].detach()).abs().mean())
    # the inference path: eval mode, the loaded running buffers
    model.load_state_dict(sd, strict=True)
    model.eval()
    with torch.no_grad():
        ev = model(x)
    assert all(torch.equal(model.state_dict()[k], sd[k]) for k in buffers), "an eval-mode forward leaves the buffers alone"
    e64 = R.run64(sd, x, t, kind, case, training=False, backward=False)[0]
    out["ref_err_eval"] = np.float64(max(float((h.double() - e).abs().max()) for h, e in zip(ev, e64)))
    model64.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}, strict=True)
    model64.eval()
    with torch.no_grad():
        ev64 = model64(x.double())
    assert max(float((a - b).abs().max()) for a, b in zip(ev64, e64)) < 1e-12
    out["eval_d1_64"] = ev64[0].numpy()[:, :, ::2, ::2, ::2].copy()
    for i, (h, s) in enumerate(zip(ev, R.SCALES)):
        out[f"eval_d{i + 1}"] = h[:, :, ::s, ::s, ::s].numpy().copy()
    path = os.path.join(OUT, R.fname(kind, case))
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < (1 << 20), (path, os.path.getsize(path))
    berr = max(float(v) for k, v in out.items() if k.startswith("ref_err_buf"))
    print(R.fname(kind, case), os.path.getsize(path), "bytes;", len(shapes), "keys; loss", loss.item(), "d1 absmax", float(heads[0].abs().max()),
          errs, "eval", float(out["ref_err_eval"]), "buffers", berr, "bf16 dev", float(out["ref_bf16_dev"]),
          "dead gradients", len([n for n in names if n not in live]))


if __name__ == "__main__":
    for kind in R.KINDS:
        for case in R.CASES:
            fixture(kind, case)
