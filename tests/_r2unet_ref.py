"""Plain-torch restatement of the reference's ``R2Unet`` (networks/unet_family.py:220-308) for the tests of
brats21_amd.networks.R2Unet: the forward in any dtype (float64 included), gradients through autograd.  It composes the pieces the
block's and the plain U-Net's tests already pin: tests/_rrcnn_ref.py's ``forward`` (RRCNNblock) and tests/_unet_ref.py's ``up_conv``,
``_nearest``, ``ds_loss``.  Pinned against the reference's own class by tests/golden/make_golden_r2unet.py ->
tests/golden/r2unet_w8_*.npz.  The cases, weights and input of those fixtures are tests/_unet_ref.py's; the state-dict key list is
NOT stated here: it is the reference class's own, recorded in the fixtures' metadata.

The input.  The deepest level of the 16 x 24 x 32 volume is 2 x 3 x 4 voxels: one max-pool or activation tie that two float32
evaluations break differently moves a gradient by percents -- a discontinuity of the gradient, not an error of either.  The seed
is chosen by the float32 error of the REFERENCE ARITHMETIC itself -- the reference class in float32 against this file's forward in
float64 on the CPU.  At seed 28 (tests/_unet_ref.py's, t = 2), against the bars of tests/test_unet_gpu.py:
    measure                                  group / relu    instance / leakyrelu    bar
    heads (max abs)                          2.4e-5          3.2e-5                  1e-3
    loss                                     2e-8            6e-9                    1e-4
    gradient norms (relative)                9.1e-6          2.2e-5                  2e-3
    small gradients (of their maximum)       1.7e-5          7.5e-5                  2e-3
Seeds at which the reference ITSELF breaks a gradient bar, and which must therefore not be used:
    group / relu            21, 26, 27, 30
    instance / leakyrelu    25, 30
Other t at seed 28, group / relu, (gradient norms, small gradients): t = 1: 5e-6, 1.1e-5; t = 3: 1.8e-5, 2.5e-5.  instance /
leakyrelu at t = 3 is NOT usable with this seed: the reference itself is at 9.7e-3, 3.6e-2 there."""
import contextlib
import io
import json
import os
import warnings

import numpy as np
import torch
import torch.nn.functional as F

import _rrcnn_ref as B
import _unet_ref as U
from oracle import unet

WIDTH, BATCH, SIZE, CASES, IDS, SCALES, T = U.WIDTH, U.BATCH, U.SIZE, U.CASES, U.IDS, U.SCALES, 2
image, target, weights, ds_loss, dice_loss = U.image, U.target, U.weights, U.ds_loss, U.dice_loss


def fname(case):
    return f"r2unet_w{WIDTH}_{case[0]}_{case[1]}.npz"


def golden(case):
    """(npz, metadata) of a committed fixture."""
    z = np.load(os.path.join(U.GOLDEN, fname(case)), allow_pickle=False)
    return z, json.loads(str(z["meta"]))


def fixture_shapes(case=CASES[0]):
    """Ordered {key: shape} of the reference class, as the fixture generator recorded it."""
    meta = golden(case)[1]
    return {k: tuple(s) for k, s in zip(meta["keys"], meta["shapes"])}


def _block(sd, pre, x, act, norm, t, x2=None):
    """RRCNNblock `pre` of the network's state dict: tests/_rrcnn_ref.py's forward on its ten entries."""
    sub = {k[len(pre) + 1:]: v for k, v in sd.items() if k.startswith(pre + ".")}
    return B.forward(sub, x, act, norm, t, x2)


def forward(sd, x, act="relu", norm="group", t=T, deep_supervision=True):
    """R2Unet.forward (:270-308): (d1, d2, d3, d4), or d1."""
    x1 = _block(sd, "RRCNN1", x, act, norm, t)
    x2 = _block(sd, "RRCNN2", F.max_pool3d(x1, 2, 2), act, norm, t)
    x3 = _block(sd, "RRCNN3", F.max_pool3d(x2, 2, 2), act, norm, t)
    x4 = _block(sd, "RRCNN4", F.max_pool3d(x3, 2, 2), act, norm, t)
    d4_up = _block(sd, "Up_RRCNN4", x3, act, norm, t, x2=U.up_conv(sd, "Up4", x4, act, norm))
    d3_up = _block(sd, "Up_RRCNN3", x2, act, norm, t, x2=U.up_conv(sd, "Up3", d4_up, act, norm))
    d2_up = _block(sd, "Up_RRCNN2", x1, act, norm, t, x2=U.up_conv(sd, "Up2", d3_up, act, norm))
    d1 = unet._c1(sd, "Conv_1x1", d2_up)
    if not deep_supervision:
        return d1
    return (d1, U._nearest(unet._c1(sd, "outconv2", d3_up), 2), U._nearest(unet._c1(sd, "outconv3", d4_up), 4),
            U._nearest(unet._c1(sd, "outconv4", x4), 8))


def run64(sd, x, t, case=CASES[0], rec=T):
    """-> (heads, loss, {key: gradient}) of the restatement in float64 on the CPU; rec: the blocks' t."""
    norm, act = case
    sd64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in sd.items()}
    res = forward(sd64, x.detach().cpu().double(), act=act, norm=norm, t=rec)
    loss = ds_loss(res, t.detach().cpu().double())
    loss.backward()
    return [h.detach() for h in res], float(loss.detach()), {k: v.grad for k, v in sd64.items()}


_RUN64 = {}


def fixture_run64(case, rec=T):
    """run64 on the fixture's weights and input (the shapes do not depend on t), computed once per process and shared by the tests
    that need it (read only)."""
    if (case, rec) not in _RUN64:
        _RUN64[case, rec] = run64(weights(fixture_shapes(case)), image(), target(), case, rec)
    return _RUN64[case, rec]


def build(case=CASES[0], img_ch=4, output_ch=3, width=WIDTH, t=T, deep_supervision=True, load=True):
    """brats21_amd's R2Unet of the case (on the CPU, f32 precision mode), the closed-form weights loaded."""
    from brats21_amd.networks import R2Unet
    norm, act = case
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = R2Unet(img_ch, output_ch, [width * 2 ** i for i in range(4)], t=t, norm_layer=norm, act=act, deep_supervision=deep_supervision)
    if load:
        sd = weights({k: tuple(v.shape) for k, v in m.state_dict().items()})
        m.load_state_dict(sd, strict=True)
    m.precision = "fp32"
    return m
