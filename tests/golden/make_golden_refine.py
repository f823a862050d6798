"""Generates tests/golden/refine_*.npz: the reference's own ``EquiUnet(refinement=True)`` (imported under oracle/refshim.py) at
width 8 on a 1 x 4 x 32^3 closed-form image with the nested-sphere target, in the configurations of tests/_refine_ref.py
(group / relu and instance / leakyrelu), in the manner of make_golden_general.py.

Run where the reference source is available only:  python tests/golden/make_golden_refine.py
The fixtures hold arrays only: the refined head at full resolution, the unrefined head on every second z plane (the committed-
file limit), the four deep heads ::2, the six-head Dice loss, the gradient-norm list, the small gradients and the key list; the
reference's own float32 error against tests/_refine_ref.py evaluated in float64 ("ref_err_*": the room the bars of
tests/test_refine_gpu.py have); and "ref_bf16_ratio": under torch.autocast("cpu", bfloat16) the reference's mean deviation of
the refined head from its f32 self over that of the unrefined head -- how much of the 16-bit error the stage adds.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import refshim, synth  # noqa: E402
import _refine_ref as R  # noqa: E402

refshim.install()
from networks.equiunet2020 import EquiUnet  # noqa: E402
from monai.losses import DiceLoss  # noqa: E402  (the stub)

OUT = os.path.dirname(os.path.abspath(__file__))
torch.set_num_threads(8)
OUT_Z = 2  # the unrefined head is stored on every second z plane


def _oracle64(case, sd, x, t):
    norm, act = case
    sd64 = {k: (v.double().requires_grad_(True) if v.is_floating_point() else v) for k, v in sd.items()}
    res = R.forward(sd64, x.double(), act=act, norm=norm)
    loss = R.ds_loss(res, t.double())
    loss.backward()
    return [h.detach() for h in R.flat(res)], float(loss.detach()), {k: v.grad for k, v in sd64.items() if getattr(v, "grad", None) is not None}


def fixture(case):
    norm, act = case
    feats = [R.WIDTH * 2 ** i for i in range(4)]
    model = EquiUnet(4, 3, feats, norm_layer=norm, act=act, deep_supervision=True, dropout=0, refinement=True)
    sd = synth.fill_state_dict(R.state_shapes(R.WIDTH, 4, 3, act, norm))
    ref_sd = model.state_dict()
    assert list(ref_sd.keys()) == list(sd.keys()), "state-dict key order/name mismatch vs reference"
    for key in sd:
        assert tuple(ref_sd[key].shape) == tuple(sd[key].shape), key
    model.load_state_dict(sd, strict=True)
    model.train()
    x, t = R.image(), synth.nested_spheres(1, R.SIZE)
    res = model(x)
    assert isinstance(res[0], list) and len(res[0]) == 2 and len(res[1]) == 4
    heads = R.flat(res)
    crit = DiceLoss(include_background=True, sigmoid=True, softmax=False, squared_pred=True, jaccard=False, batch=True)  # src/definer.py:184-193
    loss = torch.mean(torch.stack([crit(h, t) for h in heads]))  # learning/engine.py:322-330
    loss.backward()
    out = {
        "meta": json.dumps({"width": R.WIDTH, "norm": norm, "act": act, "size": list(R.SIZE), "keys": list(sd.keys()),
                            "shapes": [list(v.shape) for v in sd.values()], "out_z_stride": OUT_Z}),
        "refined": heads[0].detach().numpy(),
        "out": heads[1].detach().numpy()[:, :, ::OUT_Z],
        "loss": np.float64(loss.item()),
    }
    for i, d in enumerate(heads[2:]):
        out[f"deep{i}"] = d.detach().numpy()[:, :, ::2, ::2, ::2]
    names, gn = [], []
    for key, p in model.named_parameters():
        if p.grad is None:
            continue
        names.append(key)
        gn.append(float(p.grad.double().norm()))
        if p.grad.numel() <= 2048:
            out["grad:" + key] = p.grad.numpy().copy()
    out["grad_names"] = json.dumps(names)
    out["grad_norms"] = np.array(gn)
    # the reference's own f32 error against the f64 restatement
    h64, loss64, g64 = _oracle64(case, sd, x, t)
    params = dict(model.named_parameters())
    out["ref_err_refined"] = np.float64((heads[0].detach().double() - h64[0]).abs().max())
    out["ref_err_out"] = np.float64((heads[1].detach().double() - h64[1]).abs().max())
    out["ref_err_deep"] = np.float64(max(float((d.detach().double() - e).abs().max()) for d, e in zip(heads[2:], h64[2:])))
    out["ref_err_loss"] = np.float64(abs(loss.item() - loss64))
    out["ref_err_grad_rel"] = np.float64(max(float((params[n].grad.double() - g64[n]).norm() / g64[n].norm()) for n in names))
    # ... and in the gradient bars' own measures: the norm of every gradient, the small gradients relative to their maximum
    out["ref_err_gnorm_rel"] = np.float64(max(abs(float(params[n].grad.double().norm()) / float(g64[n].norm()) - 1.0) for n in names))
    out["ref_err_grad_small"] = np.float64(max(float((params[n].grad.double() - g64[n]).abs().max() / g64[n].abs().max())
                                               for n in names if params[n].grad.numel() <= 2048))
    # room under the bars of tests/test_refine_gpu.py (logits and deep heads 1e-3, loss 1e-4, gradient norms rtol 2e-3,
    # small gradients 2e-3 of their maximum): the
    # reference's own f32 error takes at most a quarter of the forward bars and stays under the gradient bars (measured: group /
    # relu 4.0e-4 and 6.3e-4, instance / leakyrelu 9.7e-4 and 1.56e-3 -- the closed-form volume is full of activation and
    # max-pool ties, which a rounding difference in a forward value breaks differently)
    errs = {k: float(v) for k, v in out.items() if k.startswith("ref_err")}
    assert out["ref_err_refined"] < 2.5e-4 and out["ref_err_out"] < 2.5e-4 and out["ref_err_deep"] < 2.5e-4, errs
    assert out["ref_err_loss"] < 2.5e-5 and out["ref_err_gnorm_rel"] < 2e-3 and out["ref_err_grad_small"] < 2e-3, errs
    # how much of the 16-bit deviation the stage adds, in the reference itself
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
        rb = model(x)
    e_ref = float((rb[0][0].float() - heads[0].detach()).abs().mean())
    e_out = float((rb[0][1].float() - heads[1].detach()).abs().mean())
    out["ref_bf16_err_refined"], out["ref_bf16_err_out"] = np.float64(e_ref), np.float64(e_out)
    out["ref_bf16_ratio"] = np.float64(e_ref / e_out)
    path = os.path.join(OUT, R.fname(case))
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < (1 << 20), (path, os.path.getsize(path))
    print(R.fname(case), os.path.getsize(path), "bytes; loss", loss.item(), "refined absmax", float(heads[0].abs().max()),
          "residual absmax", float((heads[0] - heads[1]).abs().max()), {k: float(v) for k, v in out.items() if k.startswith("ref_")})


if __name__ == "__main__":
    for case in R.CASES:
        fixture(case)
