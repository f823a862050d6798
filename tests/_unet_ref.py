"""Plain-torch restatement of the reference's ``Unet`` (networks/unet_family.py:13-57,134-217) for the tests of
brats21_amd.networks.Unet: the forward in any dtype (float64 included), gradients through autograd.  Pinned against the
reference's own class by tests/golden/make_golden_unet.py -> tests/golden/unet_w8_*.npz.  Also: the cases, the closed-form weights
and the input of those fixtures, stated once for the generator and the tests.  The state-dict key list is NOT stated here: it is
the reference class's own, recorded in the fixtures' metadata."""
import contextlib
import io
import json
import os
import warnings

import numpy as np
import torch
import torch.nn.functional as F

from oracle import synth, unet

WIDTH, BATCH, SIZE = 8, 2, (16, 24, 32)
CASES = [("group", "relu"), ("instance", "leakyrelu")]  # (norm, act) of the two committed fixtures
IDS = [f"{n}_{a}" for n, a in CASES]
SCALES = (1, 2, 4, 8)  # nearest up-sampling of the heads (d1, d2, d3, d4)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fname(case):
    return f"unet_w{WIDTH}_{case[0]}_{case[1]}.npz"


def golden(case):
    """(npz, metadata) of a committed fixture."""
    z = np.load(os.path.join(GOLDEN, fname(case)), allow_pickle=False)
    return z, json.loads(str(z["meta"]))


def fixture_shapes(case=CASES[0]):
    """Ordered {key: shape} of the reference class, as the fixture generator recorded it."""
    meta = golden(case)[1]
    return {k: tuple(s) for k, s in zip(meta["keys"], meta["shapes"])}


def weights(shapes):
    """Closed-form float32 values (oracle.synth.closed_form, regenerated bit for bit wherever the tests run) for an ordered
    {key: shape}: convolution weights of magnitude sqrt(2 / fan_in) * 1.2, norm scales (the 1-D ``weight`` entries) 1 +- 0.15,
    every bias +- 0.08 -- the rule of oracle.synth.fill_state_dict, told apart by shape because this network's keys are index
    paths."""
    sd = {}
    for k, shp in shapes.items():
        if k.endswith(".bias"):
            sd[k] = synth.closed_form(k, shp, 0.08, 0.0)
        elif len(shp) == 1:
            sd[k] = synth.closed_form(k, shp, 0.15, 1.0)
        else:
            sd[k] = synth.closed_form(k, shp, float(np.sqrt(2.0 / int(np.prod(shp[1:])))) * 1.2, 0.0)
    return sd


def image(n=BATCH, inplanes=4, size=SIZE, seed=28):
    """oracle.synth.random_image.  The deepest level of this volume is 2 x 3 x 4 voxels: one max-pool or activation tie that two
    float32 evaluations break differently moves a gradient by percents -- a discontinuity of the gradient, not an error of either.
    The seed is the one of 21 .. 32 with the smallest float32 error of the REFERENCE ARITHMETIC itself -- the reference class in
    float32 against this file's forward in float64 on the CPU, (gradient norms, small gradients) against the bars (2e-3, 2e-3):
        seed   group / relu        instance / leakyrelu        seed   group / relu        instance / leakyrelu
        21     3.2e-4, 9.8e-4      1.0e-3, 1.3e-3              27     4.6e-4, 5.1e-4      2.2e-4, 4.6e-4
        22     1.5e-3, 3.5e-3      2.4e-4, 6.0e-4              28     2.4e-5, 6.2e-5  <-  1.0e-4, 3.4e-4  <-
        23     1.3e-3, 4.8e-3      5.4e-6, 9.5e-6              29     3.4e-4, 4.6e-4      3.6e-4, 4.9e-4
        24     6.4e-3, 1.6e-2      3.1e-3, 1.2e-2              30     5.5e-4, 3.0e-3      3.8e-4, 9.3e-4
        25     4.2e-3, 4.5e-3      1.0e-3, 2.6e-3              31     5.9e-4, 1.7e-3      4.0e-4, 9.1e-4
        26     1.7e-4, 6.4e-4      8.1e-3, 1.6e-2              32     1.3e-4, 1.3e-4      4.5e-5, 5.1e-4
    (oracle.synth.closed_form_image: 9.9e-6, 1.4e-5 and 1.1e-3, 2.6e-3 -- over the bar in the second configuration.)"""
    return synth.random_image(n, inplanes, size, seed=seed)


def target(n=BATCH, size=SIZE):
    return synth.nested_spheres(n, size)


def _unit(sd, conv, norm_key, x, act, norm):
    """conv3x3x3 with bias -> GroupNorm(8) | InstanceNorm3d(affine) -> act (networks/unet_family.py:18-23)."""
    y = F.conv3d(x, sd[conv + ".weight"], sd[conv + ".bias"], padding=1)
    if norm == "group":
        y = F.group_norm(y, 8, sd[norm_key + ".weight"], sd[norm_key + ".bias"], 1e-5)
    elif norm == "instance":
        y = F.instance_norm(y, None, None, sd[norm_key + ".weight"], sd[norm_key + ".bias"], True, 0.1, 1e-5)
    else:
        raise ValueError(norm)
    return unet._act(y, act)


def conv_block(sd, pre, x, act, norm):
    """ConvBlock (:13-35): Sequential entries 0 / 1 and 3 / 4."""
    return _unit(sd, pre + ".conv.3", pre + ".conv.4", _unit(sd, pre + ".conv.0", pre + ".conv.1", x, act, norm), act, norm)


def _nearest(x, s):
    return F.interpolate(x, scale_factor=s, mode="nearest")  # nn.Upsample(scale_factor=s): the default mode


def up_conv(sd, pre, x, act, norm):
    """UpConv (:38-57): nearest x2 (entry 0), then entries 1 / 2."""
    return _unit(sd, pre + ".up.1", pre + ".up.2", _nearest(x, 2), act, norm)


def forward(sd, x, act="relu", norm="group", deep_supervision=True):
    """Unet.forward (:180-217): (d1, d2, d3, d4), or d1."""
    x1 = conv_block(sd, "Conv1", x, act, norm)
    x2 = conv_block(sd, "Conv2", F.max_pool3d(x1, 2, 2), act, norm)
    x3 = conv_block(sd, "Conv3", F.max_pool3d(x2, 2, 2), act, norm)
    x4 = conv_block(sd, "Conv4", F.max_pool3d(x3, 2, 2), act, norm)
    d4_up = conv_block(sd, "Up_conv4", torch.cat((x3, up_conv(sd, "Up4", x4, act, norm)), 1), act, norm)
    d3_up = conv_block(sd, "Up_conv3", torch.cat((x2, up_conv(sd, "Up3", d4_up, act, norm)), 1), act, norm)
    d2_up = conv_block(sd, "Up_conv2", torch.cat((x1, up_conv(sd, "Up2", d3_up, act, norm)), 1), act, norm)
    d1 = unet._c1(sd, "Conv_1x1", d2_up)
    if not deep_supervision:
        return d1
    return (d1, _nearest(unet._c1(sd, "outconv2", d3_up), 2), _nearest(unet._c1(sd, "outconv3", d4_up), 4),
            _nearest(unet._c1(sd, "outconv4", x4), 8))


def dice_loss(logits, target, smooth=1e-5):
    """oracle.unet.dice_loss (the criterion of src/definer.py:184-203) in the dtype of its arguments: float64 stays float64."""
    p, t, axes = torch.sigmoid(logits), target.to(logits.dtype), (0, 2, 3, 4)
    return (1.0 - (2.0 * (t * p).sum(axes) + smooth) / ((t * t).sum(axes) + (p * p).sum(axes) + smooth)).mean()


def ds_loss(heads, target):
    """Engine._compute_loss (learning/engine.py:312-333): the mean of the criterion over the heads."""
    heads = list(heads) if isinstance(heads, (tuple, list)) else [heads]
    return torch.stack([dice_loss(h, target) for h in heads]).mean()


def run64(sd, x, t, case=CASES[0]):
    """-> (heads, loss, {key: gradient}) of the restatement in float64 on the CPU."""
    norm, act = case
    sd64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in sd.items()}
    res = forward(sd64, x.detach().cpu().double(), act=act, norm=norm)
    loss = ds_loss(res, t.detach().cpu().double())
    loss.backward()
    return [h.detach() for h in res], float(loss.detach()), {k: v.grad for k, v in sd64.items()}


_RUN64 = {}


def fixture_run64(case):
    """run64 on the fixture's weights and input, computed once per process and shared by the tests that need it (read only)."""
    if case not in _RUN64:
        _RUN64[case] = run64(weights(fixture_shapes(case)), image(), target(), case)
    return _RUN64[case]


def build(case=CASES[0], img_ch=4, output_ch=3, width=WIDTH, deep_supervision=True, load=True):
    """brats21_amd's Unet of the case (on the CPU, f32 precision mode), the closed-form weights loaded."""
    from brats21_amd.networks import Unet
    norm, act = case
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = Unet(img_ch, output_ch, [width * 2 ** i for i in range(4)], norm_layer=norm, act=act, deep_supervision=deep_supervision)
    if load:
        sd = weights({k: tuple(v.shape) for k, v in m.state_dict().items()})
        m.load_state_dict(sd, strict=True)
    m.precision = "fp32"
    return m
