"""Generates tests/golden/att_w16_instance_relu.npz: the reference's own ``AttEquiUnet`` (imported under oracle/refshim.py) at
width 16 with ``--norm instance``, ``--act relu`` and deep supervision, in training mode, on a 1 x 4 x 16^3 seeded image
(tests/_att_ref.py: image) with the nested-sphere target and the seeded weights of tests/_att_ref.py (weights), in the manner of
make_golden_refine.py.

Run where the reference source is available only:  python tests/golden/make_golden_att.py
The fixture holds arrays and JSON metadata only: the logits, the four deep heads ::2, the five-head Dice loss, the gradient-norm
list, the small gradients and the key / shape lists; the reference's own float32 error against tests/_att_ref.py evaluated in
float64 ("ref_err_*": the room the bars of tests/test_att_gpu.py have -- asserted below to take at most a quarter of the forward
bars and to stay under the gradient bars); the same class in float64 ("loss64", "logits64" ::2, "grad_norms64", "grad64:*" for the
gradients of at most 64 elements); and "ref_bf16_dev": the mean |bf16 - f32| of the reference's logits under
torch.autocast("cpu", bfloat16)."""
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
from oracle import refshim, synth  # noqa: E402
import _att_ref as R  # noqa: E402

refshim.install()
from networks.equiunet2020 import AttEquiUnet  # noqa: E402
from monai.losses import DiceLoss  # noqa: E402  (the stub)

OUT = os.path.dirname(os.path.abspath(__file__))
torch.set_num_threads(8)


def fixture():
    feats = [R.WIDTH * 2 ** i for i in range(4)]
    with contextlib.redirect_stdout(io.StringIO()):
        model = AttEquiUnet(4, 3, feats, norm_layer=R.NORM, act=R.ACT, deep_supervision=True, dropout=0)
    sd = R.weights()
    ref_sd = model.state_dict()
    assert list(ref_sd.keys()) == list(sd.keys()), "state-dict key order/name mismatch vs reference"
    for key in sd:
        assert tuple(ref_sd[key].shape) == tuple(sd[key].shape), key
    model.load_state_dict(sd, strict=True)
    model.train()
    x, t = R.image(), synth.nested_spheres(1, R.SIZE)
    res = model(x)
    assert len(res) == 2 and len(res[1]) == 4
    hs = R.heads(res)
    crit = DiceLoss(include_background=True, sigmoid=True, softmax=False, squared_pred=True, jaccard=False, batch=True)  # src/definer.py:184-193
    loss = torch.mean(torch.stack([crit(h, t) for h in hs]))  # learning/engine.py:322-330
    loss.backward()
    out = {
        "meta": json.dumps({"width": R.WIDTH, "norm": R.NORM, "act": R.ACT, "size": list(R.SIZE), "keys": list(sd.keys()),
                            "shapes": [list(v.shape) for v in sd.values()]}),
        "logits": hs[0].detach().numpy(),
        "loss": np.float64(loss.item()),
    }
    for i, d in enumerate(hs[1:]):
        out[f"deep{i}"] = d.detach().numpy()[:, :, ::2, ::2, ::2]
    params = dict(model.named_parameters())
    names = list(params)
    assert all(p.grad is not None for p in params.values()) and len(names) == 103
    out["grad_names"] = json.dumps(names)
    out["grad_norms"] = np.array([float(params[n].grad.double().norm()) for n in names])
    for n in names:
        if params[n].grad.numel() <= 2048:
            out["grad:" + n] = params[n].grad.numpy().copy()
    # the reference's own f32 error against the f64 restatement, in the measures of the bars of tests/test_att_gpu.py: logits and
    # deep heads 1e-3 abs, loss 1e-4, gradient norms rtol 2e-3, small gradients 2e-3 of their maximum
    h64, loss64, g64 = R.run64(sd, x, t)
    out["ref_err_logits"] = np.float64((hs[0].detach().double() - h64[0]).abs().max())
    out["ref_err_deep"] = np.float64(max(float((d.detach().double() - e).abs().max()) for d, e in zip(hs[1:], h64[1:])))
    out["ref_err_loss"] = np.float64(abs(loss.item() - loss64))
    out["ref_err_grad_rel"] = np.float64(max(float((params[n].grad.double() - g64[n]).norm() / g64[n].norm()) for n in names))
    out["ref_err_gnorm_rel"] = np.float64(max(abs(float(params[n].grad.double().norm()) / float(g64[n].norm()) - 1.0) for n in names))
    out["ref_err_grad_small"] = np.float64(max(float((params[n].grad.double() - g64[n]).abs().max() / g64[n].abs().max())
                                               for n in names if params[n].grad.numel() <= 2048))
    errs = {k: float(v) for k, v in out.items() if k.startswith("ref_err")}
    assert out["ref_err_logits"] < 2.5e-4 and out["ref_err_deep"] < 2.5e-4 and out["ref_err_loss"] < 2.5e-5, errs
    assert out["ref_err_gnorm_rel"] < 2e-3 and out["ref_err_grad_small"] < 2e-3, errs
    # the reference class itself in float64: what tests/test_att_cpu.py holds the restatement to (1e-12)
    model64 = copy.deepcopy(model).double()
    model64.zero_grad()
    res64 = model64(x.double())
    l64 = torch.mean(torch.stack([crit(h, t.double()) for h in R.heads(res64)]))
    l64.backward()
    p64 = dict(model64.named_parameters())
    assert abs(float(l64) - loss64) < 1e-12 and float((res64[0].detach() - h64[0]).abs().max()) < 1e-12
    assert all(float((p64[n].grad - g64[n]).abs().max()) <= 1e-12 * max(1.0, float(g64[n].abs().max())) for n in names)
    out["loss64"] = np.float64(float(l64))
    out["logits64"] = res64[0].detach().numpy()[:, :, ::2, ::2, ::2]
    out["grad_norms64"] = np.array([float(p64[n].grad.norm()) for n in names])
    for n in names:
        if p64[n].grad.numel() <= 64:
            out["grad64:" + n] = p64[n].grad.numpy().copy()
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
        rb = model(x)
    out["ref_bf16_dev"] = np.float64((rb[0].float() - hs[0].detach()).abs().mean())
    path = os.path.join(OUT, R.FNAME)
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < (1 << 20), (path, os.path.getsize(path))
    print(R.FNAME, os.path.getsize(path), "bytes; loss", loss.item(), "logits absmax", float(hs[0].abs().max()), errs,
          "bf16 dev", float(out["ref_bf16_dev"]))


if __name__ == "__main__":
    fixture()
