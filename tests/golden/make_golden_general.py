"""Generates tests/golden/general_*.npz: the reference's own EquiUnet / EquiUnetASSPEvo classes (imported under
oracle/refshim.py) at input-channel and class counts other than BraTS' (4, 3) -- the cases of tests/_general_cases.py -- on
closed-form weights, images and nested-sphere targets, in the manner of make_golden.py's _model_fixture.

Run where the reference source is available only:  python tests/golden/make_golden_general.py
The fixtures hold the cases' recipes (names / sizes) and the reference's outputs -- arrays only -- and, per case, the reference's
own float32 error against oracle.unet.*_forward evaluated in float64 (keys "ref_err_*"): the room the bars of
tests/test_general_channels_gpu.py have.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import refshim, synth, unet  # noqa: E402
import _general_cases as G  # noqa: E402

refshim.install()
from networks.equiunet2020 import EquiUnet  # noqa: E402
from networks.equiunet2021 import EquiUnetASSPEvo  # noqa: E402
from monai.losses import DiceLoss  # noqa: E402  (the stub)

OUT = os.path.dirname(os.path.abspath(__file__))
torch.set_num_threads(8)


def _ds_loss(outputs, target, crit):
    # learning/engine.py:322-330 (flatten -> mean over heads)
    heads = [outputs[0]] + list(outputs[1])
    return torch.mean(torch.stack([crit(h, target) for h in heads]))


def _oracle64(case, sd, x, t):
    """oracle.unet.*_forward in float64 on the same weights and inputs: (logits, deep heads, loss, {name: gradient})"""
    sd64 = {k: (v.double().requires_grad_(True) if v.is_floating_point() else v) for k, v in sd.items()}
    out = G.oracle_forward(case)(sd64, x.double())
    loss = unet.deep_supervision_loss(out, t.double())
    loss.backward()
    return out[0].detach(), [d.detach() for d in out[1]], float(loss.detach()), {k: v.grad for k, v in sd64.items() if getattr(v, "grad", None) is not None}


def fixture(case):
    net, width, c, k = case
    cls = EquiUnet if net == "equiunet" else EquiUnetASSPEvo
    model = cls(c, k, G.features(case), norm_layer="group", act="relu", deep_supervision=True, dropout=0)
    sd = synth.fill_state_dict(G.shapes(case))
    ref_sd = model.state_dict()
    assert list(ref_sd.keys()) == list(sd.keys()), "state-dict key order/name mismatch vs reference"
    for key in sd:
        assert tuple(ref_sd[key].shape) == tuple(sd[key].shape), key
    model.load_state_dict(sd, strict=True)
    model.train()
    x, t = G.image(case), G.nested_targets(1, k)
    out = model(x)
    crit = DiceLoss(include_background=True, sigmoid=True, softmax=False, squared_pred=True, jaccard=False, batch=True)  # src/definer.py:184-193
    loss = _ds_loss(out, t, crit)
    loss.backward()
    res = {
        "meta": json.dumps({"net": net, "width": width, "inplanes": c, "num_classes": k, "size": list(G.SIZE),
                            "keys": list(sd.keys()), "shapes": [list(v.shape) for v in sd.values()]}),
        "logits": out[0].detach().numpy(),
        "loss": np.float64(loss.item()),
    }
    for i, d in enumerate(out[1]):
        res[f"deep{i}"] = d.detach().numpy()[:, :, ::2, ::2, ::2]
    names, gn = [], []
    for key, p in model.named_parameters():
        if p.grad is None:
            continue
        names.append(key)
        gn.append(float(p.grad.double().norm()))
        if p.grad.numel() <= 4096:
            res["grad:" + key] = p.grad.numpy().copy()
    res["grad_names"] = json.dumps(names)
    res["grad_norms"] = np.array(gn)
    # the reference's own f32 error against the f64 oracle
    l64, d64, loss64, g64 = _oracle64(case, sd, x, t)
    params = dict(model.named_parameters())
    res["ref_err_logits"] = np.float64((out[0].detach().double() - l64).abs().max())
    res["ref_err_deep"] = np.float64(max(float((d.detach().double() - e).abs().max()) for d, e in zip(out[1], d64)))
    res["ref_err_loss"] = np.float64(abs(loss.item() - loss64))
    res["ref_err_grad_rel"] = np.float64(max(float((params[n].grad.double() - g64[n]).norm() / g64[n].norm()) for n in names))
    path = os.path.join(OUT, G.fname(case))
    np.savez_compressed(path, **res)
    assert os.path.getsize(path) < (1 << 20), (path, os.path.getsize(path))
    print(G.fname(case), os.path.getsize(path), "bytes; loss", loss.item(), "logits absmax", float(out[0].abs().max()),
          {k2: float(v) for k2, v in res.items() if k2.startswith("ref_err")})


if __name__ == "__main__":
    for case in G.CASES + [G.BRATS_CASE]:
        fixture(case)
