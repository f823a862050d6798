"""Generates tests/golden/attgate_*.npz: the reference's own ``AttentionBlock`` (networks/unet_family.py:104-131, imported under
oracle/refshim.py) in the two configurations of tests/_attgate_ref.py -- (f_g, f_l, f_int, act) = (16, 16, 8, relu) on 2 x . x 4 x 8 x 8
and (8, 8, 4, leakyrelu) on 2 x . x 8 x 8 x 16 -- with the closed-form weights and the inputs of that file, loss = (out * dout).sum(),
in the manner of make_golden_rrcnn.py.

Run where the reference source is available only:  python tests/golden/make_golden_attgate.py
The fixtures hold arrays and JSON metadata only: the reference's state-dict key list and shapes; ``out``, ``dg``, ``dx`` and every
parameter's gradient ("grad:<key>") of one training-mode step in float32, the same from the class in float64 ("out64", "dg64",
"dx64", "grad64:<key>"); the buffers after that step ("buf:<key>", "buf64:<key>"); the eval-mode output after it ("out_eval",
"out_eval64"); the reference's own float32 error against tests/_attgate_ref.py in float64, each as max |error| over the tensor's
max |value| ("ref_err_*": the room the fixture bars of tests/test_attgate_gpu.py have); and "ref_bf16_dev_out" / "_dg" / "_dx": the
mean |bf16 - f32| of the reference's out, dg and dx under torch.autocast("cpu", bfloat16)."""
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
import _attgate_ref as R  # noqa: E402

refshim.install()
refshim._mod("monai.networks.nets", DynUNet=None)  # (networks/unet_family.py:503 imports the name for its DynUNet wrapper)
from networks.unet_family import AttentionBlock  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
torch.set_num_threads(8)


def step(model, g, x, dout, autocast=False):
    """One training-mode forward + backward of the class: -> (out, dg, dx, {key: grad})."""
    model.train()
    model.zero_grad()
    g_, x_ = g.detach().clone().requires_grad_(True), x.detach().clone().requires_grad_(True)
    if autocast:
        with torch.autocast("cpu", dtype=torch.bfloat16):
            out = model(g_, x_)
    else:
        out = model(g_, x_)
    (out.to(dout.dtype) * dout).sum().backward()
    return out.detach(), g_.grad, x_.grad, {k: p.grad.clone() for k, p in model.named_parameters()}


def rel(a, b):
    return float((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-300))


def fixture(case):
    f_g, f_l, f_int, act, dims = case
    torch.manual_seed(0)  # (the constructor's own initial values are overwritten below)
    model = AttentionBlock(f_g, f_l, f_int, act)
    keys = list(model.state_dict().keys())
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert keys == R.KEYS and shapes == R.shapes_of(f_g, f_l, f_int), keys
    sd, g, x, dout = R.fixture_inputs(case)
    model.load_state_dict(sd, strict=True)
    model64 = copy.deepcopy(model).double()
    mbf = copy.deepcopy(model)
    res, dg, dx, grads = step(model, g, x, dout)
    names = list(grads)
    assert names == R.PARAMS
    out = {"out": res.numpy().copy(), "dg": dg.numpy().copy(), "dx": dx.numpy().copy()}
    for k in names:
        out["grad:" + k] = grads[k].numpy().copy()
    bufs = {k: v.clone() for k, v in model.state_dict().items() if k in R.BUFFERS}
    for k, v in bufs.items():
        out["buf:" + k] = v.numpy().copy()
    model.eval()
    with torch.no_grad():
        out["out_eval"] = model(g, x).numpy().copy()
    # the class in float64: what tests/test_attgate_cpu.py holds the restatement to (1e-12)
    r64, dg64, dx64, g64 = step(model64, g.double(), x.double(), dout.double())
    out["out64"], out["dg64"], out["dx64"] = r64.numpy().copy(), dg64.numpy().copy(), dx64.numpy().copy()
    for k in names:
        out["grad64:" + k] = g64[k].numpy().copy()
    for k, v in model64.state_dict().items():
        if k in R.BUFFERS:
            out["buf64:" + k] = v.numpy().copy()
    model64.eval()
    with torch.no_grad():
        out["out_eval64"] = model64(g.double(), x.double()).numpy().copy()
    # the restatement against the class, and the class's own float32 error against it
    ref = R.run(sd, g, x, dout, torch.float64, act, True)
    assert rel(r64, ref["out"]) < 1e-12 and rel(dg64, ref["dg"]) < 1e-12 and rel(dx64, ref["dx"]) < 1e-12
    out["ref_err_out"], out["ref_err_dg"], out["ref_err_dx"] = (np.float64(rel(a, b)) for a, b in
                                                                 ((res, ref["out"]), (dg, ref["dg"]), (dx, ref["dx"])))
    for k in names:
        den = ref["grads"][R.DEAD[k]] if k in R.DEAD else ref["grads"][k]
        out["ref_err_grad:" + k] = np.float64(float((grads[k].double() - ref["grads"][k]).abs().max() / den.abs().max()))
    for k in R.BUFFERS:
        if not k.endswith("num_batches_tracked"):
            out["ref_err_buf:" + k] = np.float64(rel(bufs[k], ref["buffers"][k]))
    ev = R.run({**sd, **ref["buffers"]}, g, x, dout, torch.float64, act, False, parts=("out",))
    out["ref_err_out_eval"] = np.float64(rel(torch.from_numpy(out["out_eval"]), ev["out"]))
    errs = {k: float(v) for k, v in out.items() if k.startswith("ref_err")}
    assert max(errs.values()) < 1e-4, errs
    rb, dgb, dxb, _ = step(mbf, g, x, dout, autocast=True)
    out["ref_bf16_dev_out"] = np.float64((rb.float() - res).abs().mean())
    out["ref_bf16_dev_dg"] = np.float64((dgb.float() - dg).abs().mean())
    out["ref_bf16_dev_dx"] = np.float64((dxb.float() - dx).abs().mean())
    out["meta"] = json.dumps({"f_g": f_g, "f_l": f_l, "f_int": f_int, "act": act, "dims": list(dims), "keys": keys,
                              "shapes": [list(shapes[k]) for k in keys], "params": names})
    path = os.path.join(OUT, R.fname(case))
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < (1 << 20), (path, os.path.getsize(path))
    print(R.fname(case), os.path.getsize(path), "bytes;", len(keys), "keys; out absmax", float(res.abs().max()),
          "worst ref_err", max(errs.values()), "bf16 dev", float(out["ref_bf16_dev_out"]), float(out["ref_bf16_dev_dg"]),
          float(out["ref_bf16_dev_dx"]))


if __name__ == "__main__":
    for case in R.CASES:
        fixture(case)
