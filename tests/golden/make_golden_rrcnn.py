"""Generates tests/golden/rrcnn_*.npz: the reference's own ``RRCNNblock`` (networks/unet_family.py:89-101, imported under
oracle/refshim.py) in the two configurations of tests/_rrcnn_ref.py -- 4 -> 16 group / relu on 2 x 4 x 8 x 8 x 16 and 32 -> 16
instance / leakyrelu on 2 x 32 x 8 x 16 x 16, t = 2 -- with the closed-form weights, input and upstream gradient g of that file,
loss = (out * g).sum(), in the manner of make_golden_unet.py.

Run where the reference source is available only:  python tests/golden/make_golden_rrcnn.py
The fixtures hold arrays and JSON metadata only: the reference's state-dict key list and shapes (the tests take the list from here),
``out``, ``dx``, every parameter's gradient ("grad:<key>"); the same from the reference class in float64 ("out64", "dx64",
"grad64:<key>"); dx and the float64 tensors of more than 32768 elements on the ::2 lattice of their three spatial axes
(metadata "lattice"); the reference's own float32 error against tests/_rrcnn_ref.py in float64 ("ref_err_*": the room the bars of
tests/test_rrcnn_gpu.py have); and "ref_bf16_dev": the mean |bf16 - f32| of the reference's out under torch.autocast("cpu",
bfloat16)."""
import copy
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import refshim  # noqa: E402
import _rrcnn_ref as R  # noqa: E402

refshim.install()
refshim._mod("monai.networks.nets", DynUNet=None)  # (networks/unet_family.py:503 imports the name for its DynUNet wrapper)
from networks.factory import get_norm_layer  # noqa: E402
from networks.unet_family import RRCNNblock  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
torch.set_num_threads(8)


def _lat(a, step):
    return a[:, :, ::step, ::step, ::step]


def fixture(case):
    ch_in, ch_out, norm, act, t, dims = case
    torch.manual_seed(0)  # (the constructor's own initial values are overwritten below)
    model = RRCNNblock(ch_in, ch_out, get_norm_layer(norm), act, t=t)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = R.weights(shapes)
    model.load_state_dict(sd, strict=True)
    model.train()
    x, g = R.image(ch_in, dims).requires_grad_(True), R.upstream(ch_out, dims)
    res = model(x)
    assert res.shape == g.shape
    (res * g).sum().backward()
    params = dict(model.named_parameters())
    names = list(params)
    assert names == list(shapes) and all(p.grad is not None for p in params.values())
    lat = {"dx": 2 if x.numel() > R.LATTICE_FROM else 1, "out64": 2 if res.numel() > R.LATTICE_FROM else 1}
    out = {"out": res.detach().numpy().copy(), "dx": _lat(x.grad, lat["dx"]).numpy().copy()}
    for n_ in names:
        out["grad:" + n_] = params[n_].grad.numpy().copy()
    # the reference's own f32 error against the f64 restatement, in the measures of the bars of tests/test_rrcnn_gpu.py: out 1e-3
    # abs, gradient norms rtol 2e-3, small gradients (and dx) 2e-3 of their maximum; a gradient that is zero in exact arithmetic
    # (the 3x3x3 biases under instance norm) is held to the absolute part, against the maximum of the unit's norm-shift gradient
    o64, dx64, _, g64 = R.run64(sd, x, g, norm, act, t)
    live = [n_ for n_ in names if float(g64[n_].abs().max()) > 1e-9 * max(1.0, float(g64[n_.replace("conv.0.bias", "conv.1.bias")].abs().max()))]
    dead = [n_ for n_ in names if n_ not in live]
    assert dead == ([] if norm == "group" else ["RCNN.0.conv.0.bias", "RCNN.1.conv.0.bias"]), dead
    out["ref_err_out"] = np.float64((res.detach().double() - o64).abs().max())
    out["ref_err_dx"] = np.float64((x.grad.double() - dx64).abs().max() / dx64.abs().max())
    out["ref_err_gnorm_rel"] = np.float64(max(abs(float(params[n_].grad.double().norm()) / float(g64[n_].norm()) - 1.0) for n_ in live))
    out["ref_err_grad_small"] = np.float64(max(float((params[n_].grad.double() - g64[n_]).abs().max() / g64[n_].abs().max())
                                               for n_ in live if params[n_].grad.numel() <= 2048))
    out["ref_err_grad_dead"] = np.float64(max([float(params[n_].grad.abs().max() / g64[n_.replace("conv.0.bias", "conv.1.bias")].abs().max())
                                               for n_ in dead] or [0.0]))
    errs = {k: float(v) for k, v in out.items() if k.startswith("ref_err")}
    # a quarter of the bar each
    assert out["ref_err_out"] <= 2.5e-4 and out["ref_err_dx"] <= 5e-4 and out["ref_err_gnorm_rel"] <= 5e-4, errs
    assert out["ref_err_grad_small"] <= 5e-4 and out["ref_err_grad_dead"] <= 5e-4, errs
    # the reference class itself in float64: what tests/test_rrcnn_cpu.py holds the restatement to (1e-12)
    model64 = copy.deepcopy(model).double()
    model64.zero_grad()
    x64 = x.detach().double().requires_grad_(True)
    r64 = model64(x64)
    (r64 * g.double()).sum().backward()
    p64 = dict(model64.named_parameters())
    assert float((r64.detach() - o64).abs().max()) < 1e-12 and float((x64.grad - dx64).abs().max()) <= 1e-12 * float(dx64.abs().max())
    assert all(float((p64[n_].grad - g64[n_]).abs().max()) <= 1e-12 * max(1.0, float(g64[n_].abs().max())) for n_ in names)
    out["out64"] = _lat(r64.detach(), lat["out64"]).numpy().copy()
    out["dx64"] = _lat(x64.grad, lat["dx"]).numpy().copy()
    for n_ in names:
        out["grad64:" + n_] = p64[n_].grad.numpy().copy()
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
        rb = model(x.detach())
    out["ref_bf16_dev"] = np.float64((rb.float() - res.detach()).abs().mean())
    out["meta"] = json.dumps({"ch_in": ch_in, "ch_out": ch_out, "norm": norm, "act": act, "t": t, "dims": list(dims), "keys": names,
                              "shapes": [list(s) for s in shapes.values()], "lattice": lat, "dead": dead})
    path = os.path.join(OUT, R.fname(case))
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < (1 << 20), (path, os.path.getsize(path))
    print(R.fname(case), os.path.getsize(path), "bytes;", len(names), "keys; out absmax", float(res.detach().abs().max()), errs,
          "bf16 dev", float(out["ref_bf16_dev"]), "dead gradients", dead)


if __name__ == "__main__":
    for case in R.CASES:
        fixture(case)
