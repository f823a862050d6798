"""Generates tests/golden/cbam.npz from the reference's own ``CBAM`` class (networks/equiunet2020.py:224-235, imported under
oracle/refshim.py) with ``get_norm_layer("instance")``, in float64, in the manner of make_golden_refine.py.

Run where the reference source is available only:  python tests/golden/make_golden_cbam.py
Three cases, arrays only: "c16" (2 x 16 x 3 x 5 x 7) and "c48" (1 x 48 x 4 x 3 x 5) with random parameters and inputs, and "tie"
(2 x 16 x 4 x 5 x 6): small-integer inputs with W2 = 0 and b2 = 0, so that the channel scale is exactly 0.5 and every tie of x --
equal maxima over the voxels of a channel, equal maxima over the channels of a voxel -- is a tie of the tensors the two max
operations see.  Per case: the state dict, x, dout, out, dx and the seven parameter gradients of sum(out * dout)."""
import contextlib
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
import _cbam_ref as R  # noqa: E402

refshim.install()
from networks.equiunet2020 import CBAM  # noqa: E402
from networks.factory import get_norm_layer  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cbam.npz")
CASES = {"c16": (2, 16, 3, 5, 7), "c48": (1, 48, 4, 3, 5), "tie": (2, 16, 4, 5, 6)}


def reference_block(c):
    with contextlib.redirect_stdout(io.StringIO()):  # (get_norm_layer prints its argument)
        return CBAM(c, norm_layer=get_norm_layer("instance")).double()


def make_case(name, shape, g):
    n, c = shape[:2]
    sd = {k: torch.randn(s, generator=g, dtype=torch.float64) * (0.3 if len(s) > 1 else 0.1) for k, s in R.shapes(c).items()}
    sd[R.KEYS[4]] = torch.randn((1, 2, 7, 7, 7), generator=g, dtype=torch.float64) * 0.05
    sd[R.KEYS[5]], sd[R.KEYS[6]] = torch.tensor([1.3], dtype=torch.float64), torch.tensor([0.2], dtype=torch.float64)
    if name == "tie":
        x = torch.randint(-3, 4, shape, generator=g).double()
        dout = torch.randint(-2, 3, shape, generator=g).double()
        sd[R.KEYS[2]], sd[R.KEYS[3]] = torch.zeros(c, c // 16, dtype=torch.float64), torch.zeros(c, dtype=torch.float64)
        sd[R.KEYS[4]] = torch.randint(-2, 3, (1, 2, 7, 7, 7), generator=g).double() / 8
    else:
        x = torch.randn(shape, generator=g, dtype=torch.float64) * 2
        dout = torch.randn(shape, generator=g, dtype=torch.float64)
    return sd, x, dout


def main():
    g = torch.Generator().manual_seed(2021)
    out = {"meta": json.dumps({"cases": {k: list(v) for k, v in CASES.items()}, "keys": list(R.KEYS)})}
    for name, shape in CASES.items():
        sd, x, dout = make_case(name, shape, g)
        m = reference_block(shape[1])
        assert list(m.state_dict().keys()) == list(R.KEYS), list(m.state_dict().keys())
        assert all(tuple(m.state_dict()[k].shape) == tuple(sd[k].shape) for k in R.KEYS)
        m.load_state_dict(sd, strict=True)
        m.train()
        xx = x.clone().requires_grad_(True)
        y = m(xx)
        y.backward(dout)
        grads = dict(m.named_parameters())
        # the restatement agrees with the class it restates
        y2, dx2, g2 = R.run(sd, x, dout)
        assert float((y2 - y.detach()).abs().max()) < 1e-12 and float((dx2 - xx.grad).abs().max()) < 1e-12
        assert all(float((g2[k] - grads[k].grad).abs().max()) < 1e-12 for k in R.KEYS)
        if name == "tie":  # both kinds of tie are really there
            flat = x.flatten(2)
            assert bool(((flat == flat.max(2, keepdim=True)[0]).sum(2) > 1).any())
            assert bool(((x == x.max(1, keepdim=True)[0]).sum(1) > 1).any())
        for k in R.KEYS:
            out[f"{name}/sd/{k}"] = sd[k].numpy()
            out[f"{name}/grad/{k}"] = grads[k].grad.numpy()
        out[f"{name}/x"], out[f"{name}/dout"] = x.numpy(), dout.numpy()
        out[f"{name}/out"], out[f"{name}/dx"] = y.detach().numpy(), xx.grad.numpy()
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
