"""Plain-torch restatement of the reference's ``AttEquiUnet`` (networks/equiunet2020.py:238-249,503-561; ``Unet.forward`` :374-405)
for the tests of brats21_amd.networks.AttEquiUnet: the state-dict shapes in the reference's order and the forward, in any dtype
(float64 included).  Built on oracle/unet.py (the units, the decoder, the heads) and tests/_cbam_ref.py (the gate); pinned against
the reference's own class by tests/golden/make_golden_att.py -> tests/golden/att_w16_instance_relu.npz.  Also: the case and the
seeded input of that fixture, stated once for the generator and the tests."""
import contextlib
import io
import warnings

import torch
import torch.nn.functional as F

import _cbam_ref as C
from oracle import synth, unet

WIDTH, SIZE = 16, (16, 16, 16)  # width 16: the narrowest the gates take (C // 16 >= 1)
NORM, ACT = "instance", "relu"
FNAME = f"att_w{WIDTH}_{NORM}_{ACT}.npz"
GATED = ("encoder1", "encoder2", "encoder3", "encoder4", "bottom")


def state_shapes(width=WIDTH, inplanes=4, num_classes=3, act=ACT, norm=NORM):
    """Ordered {key: shape}: EquiUnet's keys with ``UBlock.`` inside the gated blocks and ``bottom_2.0.`` for the unit of bottom_2,
    each followed by its gate's seven keys (``<block>.CBAM.*``, ``bottom_2.1.*``)."""
    f = [width * 2 ** i for i in range(4)]
    base = unet.equiunet_state_shapes(width, inplanes=inplanes, num_classes=num_classes, act=act, norm=norm)
    gate_c = dict(zip(GATED, (f[0], f[1], f[2], f[3], f[3])))
    shapes, blocks = {}, {}
    for key, shp in base.items():
        blocks.setdefault(key.split(".")[0], []).append((key, shp))
    for blk, items in blocks.items():
        if blk in gate_c:
            for key, shp in items:
                shapes[f"{blk}.UBlock.{key[len(blk) + 1:]}"] = shp
            for k, shp in C.shapes(gate_c[blk]).items():
                shapes[f"{blk}.CBAM.{k}"] = shp
        elif blk == "bottom_2":
            for key, shp in items:
                shapes["bottom_2.0." + key[len("bottom_2."):]] = shp
            for k, shp in C.shapes(f[2]).items():
                shapes["bottom_2.1." + k] = shp
        else:
            shapes.update(items)
    return shapes


def _sub(sd, pre):
    return {k[len(pre) + 1:]: v for k, v in sd.items() if k.startswith(pre + ".")}


def forward(sd, x, act=ACT, deep_supervision=True, norm=NORM, training=True, drop=None):
    """AttEquiUnet.forward = Unet.forward over the gated blocks: (logits, [4 deep heads]), or logits."""
    kw = dict(act=act, norm=norm, training=training, drop=drop)

    def block(pre, t, dil=(1, 1)):
        return C.forward(_sub(sd, pre + ".CBAM"), unet.ublock(sd, pre + ".UBlock", t, dil, **kw))

    down1 = block("encoder1", x)
    down2 = block("encoder2", F.max_pool3d(down1, 2, 2))
    down3 = block("encoder3", F.max_pool3d(down2, 2, 2))
    down4 = block("encoder4", F.max_pool3d(down3, 2, 2))
    bottom = block("bottom", down4, (2, 2))
    bottom_2 = C.forward(_sub(sd, "bottom_2.1"), unet.conv_gn_act(sd, "bottom_2.0", torch.cat([down4, bottom], 1), 1, act, norm, training, None, drop))
    up3 = unet.ublock(sd, "decoder3", torch.cat([down3, unet._up(bottom_2, 2)], 1), **kw)
    up2 = unet.ublock(sd, "decoder2", torch.cat([down2, unet._up(up3, 2)], 1), **kw)
    up1 = unet.ublock(sd, "decoder1", torch.cat([down1, unet._up(up2, 2)], 1), **kw)
    out = unet._c1(sd, "outconv", up1)
    if not deep_supervision:
        return out
    return out, [unet._up(unet._c1(sd, "deep_bottom.0", bottom), 8), unet._up(unet._c1(sd, "deep_bottom2.0", bottom_2), 8),
                 unet._up(unet._c1(sd, "deep3.0", up3), 4), unet._up(unet._c1(sd, "deep2.0", up2), 2)]


def heads(outputs):
    """[logits, deep heads...]"""
    return [outputs[0]] + list(outputs[1]) if isinstance(outputs, (tuple, list)) else [outputs]


def dice_loss(logits, target, smooth=1e-5):
    """oracle.unet.dice_loss (the criterion of src/definer.py:184-203) in the dtype of its arguments: float64 stays float64."""
    p, t, axes = torch.sigmoid(logits), target.to(logits.dtype), (0, 2, 3, 4)
    return (1.0 - (2.0 * (t * p).sum(axes) + smooth) / ((t * t).sum(axes) + (p * p).sum(axes) + smooth)).mean()


def ds_loss(outputs, target):
    """Engine._compute_loss (learning/engine.py:312-333): the mean of the criterion over the five heads."""
    return torch.stack([dice_loss(h, target) for h in heads(outputs)]).mean()


def image(n=1, inplanes=4, size=SIZE, seed=23):
    """Seeded N(0, 1) on the whole volume.  Not oracle.synth.random_image: its zero background makes whole regions of every
    activation exactly equal, so the maxima the gates and the pooling take (over the voxels of a channel, over a window) sit on
    exact ties there, which two float32 evaluations that sum in different orders break differently -- a discontinuity of the
    gradient, not an error of either (measured: 2e-3 of a gradient's norm between two CPUs' float32 runs of the reference).
    The fixture's seed is the one of 21 .. 28 with the smallest float32 error of the REFERENCE ARITHMETIC itself -- this file's
    forward in float32 against float64 on the CPU, worst parameter-gradient |delta| / |g|: 1.7e-4, 2.6e-5, 1.5e-5 <-, 1.8e-4, 6.5e-3,
    8.9e-3, 5.2e-5, 1.2e-5 (the large ones are scalar gradients of the gates' norm that cancel to 1e-5 and below; at seed 23 the
    smallest gradient norm is 3.4e-4)."""
    return torch.randn((n, inplanes) + tuple(size), generator=torch.Generator().manual_seed(seed))


def weights(width=WIDTH, inplanes=4, num_classes=3, seed=7):
    """A float32 state dict in the manner of the reference's init_weights("kaiming") from a private seeded CPU generator, key by
    key in state-dict order (regenerated by the generator script and the tests alike; the network is too large to commit):
    convolution and Linear weights N(0, 2 / fan_out), norm scales 1 + 0.1 N(0, 1), biases and norm shifts 0.05 N(0, 1).
    (oracle.synth.fill_state_dict's closed-form weights leave the single hidden unit of two gates' MLPs dead at width 16: six
    gradients are exactly zero and nothing about them would be tested.)"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shp in state_shapes(width, inplanes, num_classes).items():
        r = torch.randn(shp, generator=g)
        if len(shp) > 1:
            fan_out = shp[0] * int(torch.tensor(shp[2:]).prod()) if len(shp) > 2 else shp[0]
            sd[k] = r * (2.0 / fan_out) ** 0.5
        elif k.endswith("bn.weight"):
            sd[k] = 1.0 + 0.1 * r
        else:
            sd[k] = 0.05 * r
    return sd


def build(inplanes=4, num_classes=3, width=WIDTH, deep_supervision=True, dropout=0, sd=None):
    """brats21_amd's AttEquiUnet (on the CPU, f32 precision mode), optionally with a state dict loaded."""
    from brats21_amd.networks import AttEquiUnet
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = AttEquiUnet(inplanes, num_classes, [width * 2 ** i for i in range(4)], norm_layer=NORM, act=ACT,
                        deep_supervision=deep_supervision, dropout=dropout)
    if sd is not None:
        m.load_state_dict({k: sd[k] for k in m.state_dict()}, strict=True)
    m.precision = "fp32"
    return m


def run64(sd, x, target):
    """-> (heads, loss, {key: gradient}) of the restatement in float64 on the CPU."""
    sd64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in sd.items()}
    res = forward(sd64, x.detach().cpu().double())
    loss = ds_loss(res, target.detach().cpu().double())
    loss.backward()
    return [h.detach() for h in heads(res)], float(loss.detach()), {k: v.grad for k, v in sd64.items()}
