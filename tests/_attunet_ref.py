"""Plain-torch restatement of the reference's ``AttUnet`` and ``R2AttUnet`` (networks/unet_family.py:311-402, :405-499) for the tests of
brats21_amd.networks.AttUnet / R2AttUnet: the forward in any dtype (float64 included) in training or eval mode, gradients through
autograd, the BatchNorm buffers after the call.  It composes what the members' own tests already pin: tests/_unet_ref.py
(``conv_block``, ``up_conv``, ``_nearest``, ``ds_loss``), tests/_r2unet_ref.py (``_block``) and tests/_attgate_ref.py (``forward`` of
the gate, with nn.BatchNorm3d's rules).  Pinned against the reference's own classes by tests/golden/make_golden_attunet.py ->
tests/golden/attunet_w8_*.npz, r2attunet_w8_*.npz.  The cases, the input and the target are tests/_unet_ref.py's; the state-dict key
lists are NOT stated here: they are the reference classes' own, recorded in the fixtures' metadata.

Width 8 gives Att2 an f_int of 4: below a channel vector, the padded path of ops.attgate_fwd."""
import contextlib
import io
import json
import os
import warnings

import numpy as np
import torch
import torch.nn.functional as F

import _attgate_ref as G
import _r2unet_ref as R2
import _unet_ref as U
from oracle import synth, unet

WIDTH, BATCH, SIZE, CASES, IDS, SCALES, T = U.WIDTH, U.BATCH, U.SIZE, U.CASES, U.IDS, U.SCALES, R2.T
image, target, ds_loss, dice_loss = U.image, U.target, U.ds_loss, U.dice_loss
KINDS = ("attunet", "r2attunet")
NKEYS = {"attunet": (139, 112), "r2attunet": (153, 126)}  # state-dict keys, parameters
BUFFER_TAILS = ("running_mean", "running_var", "num_batches_tracked")
GATES = ("Att4", "Att3", "Att2")
# The closed-form convolution-weight gain, sqrt(2 / fan_in) * GAIN, per (kind, case).  tests/_unet_ref.py's 1.2 is not usable here:
# with it the REFERENCE ITSELF (the reference class in float32 against this file's forward in float64, CPU) misses the gradient
# bars of tests/test_unet_gpu.py (2e-3, 2e-3) in three of the four configurations.  The one-element gradients of psi.1.weight /
# psi.1.bias are sums over all voxels that cancel to a small remainder, and the deepest level is 2 x 3 x 4 voxels, where one tie
# broken the other way moves a gradient by percents (tests/_unet_ref.py: image).  Gains 0.5 .. 2.0 in steps of 0.025 were scanned
# for (a) the reference's own float32 error and (b) the response of the float64 restatement to a relative perturbation of 6e-8 (one
# float32 rounding) of input and weights, two draws; a gain is usable where both are far below the bars.  Chosen, with (gradient
# norms, small gradients, eval-mode heads) of (a) and the worst gradient change over its maximum of (b):
#     attunet    group / relu            0.8      7.0e-6, 4.5e-5, 3.8e-5    1.1e-5
#     attunet    instance / leakyrelu    0.65     2.9e-5, 4.9e-5, 9.7e-5    3.9e-5
#     r2attunet  group / relu            1.525    2.0e-5, 2.2e-5, 2.8e-4    1.1e-5
#     r2attunet  instance / leakyrelu    1.925    6.6e-5, 1.8e-4, 3.3e-4    1.9e-4
# Not usable (the reference itself breaks a gradient bar): e.g. attunet group / relu 0.7, 0.85, 1.05, 1.25, 1.3; r2attunet
# instance / leakyrelu everything from 0.6 to 1.05.
GAIN = {("attunet", CASES[0]): 0.8, ("attunet", CASES[1]): 0.65, ("r2attunet", CASES[0]): 1.525, ("r2attunet", CASES[1]): 1.925}


def fname(kind, case):
    return f"{kind}_w{WIDTH}_{case[0]}_{case[1]}.npz"


def golden(kind, case):
    """(npz, metadata) of a committed fixture."""
    z = np.load(os.path.join(U.GOLDEN, fname(kind, case)), allow_pickle=False)
    return z, json.loads(str(z["meta"]))


def fixture_shapes(kind, case=CASES[0]):
    """Ordered {key: shape} of the reference class, as the fixture generator recorded it."""
    meta = golden(kind, case)[1]
    return {k: tuple(s) for k, s in zip(meta["keys"], meta["shapes"])}


def is_buffer(key):
    return key.endswith(BUFFER_TAILS)


def weights(shapes, gain=1.2):
    """Closed-form float32 values (oracle.synth.closed_form) for an ordered {key: shape}: tests/_unet_ref.py's rule for the
    convolutions and norms (weights of magnitude sqrt(2 / fan_in) * gain, scales 1 +- 0.15, biases +- 0.08 -- the gates' BatchNorm
    weights and biases included), tests/_attgate_ref.py's for the gates' buffers: running means +- 0.05, running variances 1 +- 0.2
    (positive), no batch tracked yet."""
    sd = {}
    for k, shp in shapes.items():
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.tensor(0, dtype=torch.long)
        elif k.endswith("running_var"):
            sd[k] = synth.closed_form(k, shp, 0.2, 1.0)
        elif k.endswith("running_mean"):
            sd[k] = synth.closed_form(k, shp, 0.05, 0.0)
        elif k.endswith(".bias"):
            sd[k] = synth.closed_form(k, shp, 0.08, 0.0)
        elif len(shp) == 1:
            sd[k] = synth.closed_form(k, shp, 0.15, 1.0)
        else:
            sd[k] = synth.closed_form(k, shp, float(np.sqrt(2.0 / int(np.prod(shp[1:])))) * gain, 0.0)
    return sd


def fixture_weights(kind, case):
    return weights(fixture_shapes(kind, case), GAIN.get((kind, case), 1.2))


def _gate(sd, pre, g, x, act, training, new):
    """AttentionBlock `pre` of the network's state dict: tests/_attgate_ref.py's forward on its 21 entries; the buffers after the
    call go to `new` under the network's keys."""
    sub = {k[len(pre) + 1:]: v for k, v in sd.items() if k.startswith(pre + ".")}
    out, buffers = G.forward(sub, g, x, act, training)
    new.update({f"{pre}.{k}": v for k, v in buffers.items()})
    return out


def forward(sd, x, kind, act="relu", norm="group", t=T, training=True, deep_supervision=True):
    """AttUnet.forward (:361-402) / R2AttUnet.forward (:459-499): -> ((d1, d2, d3, d4) or d1, {buffer key: value after the call})."""
    if kind == "attunet":
        names = ("Conv1", "Conv2", "Conv3", "Conv4", "Up_conv4", "Up_conv3", "Up_conv2")

        def block(pre, a, b=None):
            return U.conv_block(sd, pre, a if b is None else torch.cat((a, b), 1), act, norm)
    elif kind == "r2attunet":
        names = ("RRCNN1", "RRCNN2", "RRCNN3", "RRCNN4", "Up_RRCNN4", "Up_RRCNN3", "Up_RRCNN2")

        def block(pre, a, b=None):
            return R2._block(sd, pre, a, act, norm, t, x2=b)
    else:
        raise ValueError(kind)
    new = {}
    x1 = block(names[0], x)
    x2 = block(names[1], F.max_pool3d(x1, 2, 2))
    x3 = block(names[2], F.max_pool3d(x2, 2, 2))
    x4 = block(names[3], F.max_pool3d(x3, 2, 2))
    d4 = U.up_conv(sd, "Up4", x4, act, norm)
    d4_up = block(names[4], _gate(sd, "Att4", d4, x3, act, training, new), d4)
    d3 = U.up_conv(sd, "Up3", d4_up, act, norm)
    d3_up = block(names[5], _gate(sd, "Att3", d3, x2, act, training, new), d3)
    d2 = U.up_conv(sd, "Up2", d3_up, act, norm)
    d2_up = block(names[6], _gate(sd, "Att2", d2, x1, act, training, new), d2)
    d1 = unet._c1(sd, "Conv_1x1", d2_up)
    if not deep_supervision:
        return d1, new
    return (d1, U._nearest(unet._c1(sd, "outconv2", d3_up), 2), U._nearest(unet._c1(sd, "outconv3", d4_up), 4),
            U._nearest(unet._c1(sd, "outconv4", x4), 8)), new


def run64(sd, x, t, kind, case=CASES[0], training=True, backward=True):
    """-> (heads, loss, {parameter key: gradient}, {buffer key: value after the call}) of the restatement in float64 on the CPU;
    backward=False: no gradients ({})."""
    norm, act = case
    sd64 = {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()) for k, v in sd.items()}
    for k, v in sd64.items():
        if not is_buffer(k):
            v.requires_grad_(backward)
    res, new = forward(sd64, x.detach().cpu().double(), kind, act=act, norm=norm, training=training)
    loss = ds_loss(res, t.detach().cpu().double())
    if backward:
        loss.backward()
    grads = {k: v.grad for k, v in sd64.items() if not is_buffer(k)} if backward else {}
    return [h.detach() for h in res], float(loss.detach()), grads, {k: v.detach() for k, v in new.items()}


_RUN64 = {}


def fixture_run64(kind, case, training=True):
    """run64 on the fixture's weights and input, computed once per process and shared by the tests that need it (read only); the
    eval-mode run has no backward."""
    key = (kind, case, training)
    if key not in _RUN64:
        _RUN64[key] = run64(fixture_weights(kind, case), image(), target(), kind, case, training, backward=training)
    return _RUN64[key]


def build(kind, case=CASES[0], img_ch=4, output_ch=3, width=WIDTH, t=T, deep_supervision=True, load=True):
    """brats21_amd's AttUnet / R2AttUnet of the case (on the CPU, f32 precision mode), the closed-form weights and buffers loaded."""
    from brats21_amd.networks import AttUnet, R2AttUnet
    norm, act = case
    feats = [width * 2 ** i for i in range(4)]
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if kind == "attunet":
            m = AttUnet(img_ch, output_ch, feats, norm_layer=norm, act=act, deep_supervision=deep_supervision)
        else:
            m = R2AttUnet(img_ch, output_ch, feats, t=t, norm_layer=norm, act=act, deep_supervision=deep_supervision)
    if load:
        sd = weights({k: tuple(v.shape) for k, v in m.state_dict().items()}, GAIN.get((kind, case), 1.2))
        m.load_state_dict(sd, strict=True)
    m.precision = "fp32"
    return m
