"""Unet (``--model modified_unet``): the plain U-Net of the reference's networks/unet_family.py:134-217 on the HIP kernels -- same
constructor, same ``state_dict`` keys / shapes / order (the reference's containers are nn.Sequentials, so the names are index
paths: ``Conv1.conv.0.weight``, ``Up4.up.1.bias``, ...), same ``forward(x) -> (d1, d2, d3, d4)`` flat tuple.

The units are EquiUnet's programs (networks/equiunet.py: _cgr_fwd / _cgr_bwd) with a learnable convolution bias; what differs from
EquiUnet is the shape of the program: no bottom block, an ``UpConv`` (nearest-neighbour x2 -> one unit) in front of every decoder
block, and deep heads that are 1x1x1 convolutions followed by NEAREST up-sampling of the logits (ops.upsample_nearest /
ops.planes_nearest and their adjoints, csrc/nearest.hip).  That shape is the family's (_UnetFamily: R2Unet, networks/r2unet.py,
runs it too, and AttUnet / R2AttUnet, networks/attunet.py, with an attention gate on every skip tensor through the family's two
gate hooks); Unet's own part is its block, two units, and the output head folded onto the last of them.

Built: ``--norm group | instance``, ``--act relu | leakyrelu | elu | swish | mish``, f32 / bf16 / fp16 storage and the split-precision
modes.  ``batch``, ``bcn``, ``none``, ``prelu`` and the e4m3 convolutions raise NotImplementedError.
"""
import functools
import os

import torch.nn as nn

from .. import ops
from ._program import _PackedWeightsModule
from .attgate import AttentionBlock
from .equiunet import (_cgr_bwd, _cgr_fwd, _ConvParams, _deep_heads_on, _level_bwd, _NormParams, _top_head_bwd,
                       _top_head_fwd)


class _Unit:
    """One conv (bias) -> norm -> act stretch of a reference nn.Sequential, as the unit programs read a ConvBnRelu: .conv, .bn,
    .groups, .dilation.  Not a module: the parameters are registered under the Sequential's index names."""
    batch_norm = bcn = False
    dilation = 1

    def __init__(self, conv, bn, groups):
        self.conv, self.bn, self.groups = conv, bn, groups


def _entries(first, chans, norm):
    """({index name: module}, [units]) of a Sequential of conv -> norm -> act triples starting at index `first`."""
    mods, units = {}, []
    for i, (cin, cout) in enumerate(chans):
        conv, bn = _ConvParams(cin, cout, 3, bias=True), _NormParams(cout)
        mods[str(first + 3 * i)], mods[str(first + 3 * i + 1)] = conv, bn
        units.append(_Unit(conv, bn, 8 if norm == "group" else cout))
    return mods, units


class ConvBlock(nn.Module):
    """networks/unet_family.py:13-35: keys ``conv.0.*`` (convolution), ``conv.1.*`` (norm), ``conv.3.*``, ``conv.4.*``."""

    def __init__(self, ch_in, ch_out, norm, act):
        super().__init__()
        mods, self.units = _entries(0, [(ch_in, ch_out), (ch_out, ch_out)], norm)
        self.conv = nn.ModuleDict(mods)


class UpConv(nn.Module):
    """networks/unet_family.py:38-57: nn.Upsample is entry 0, so the keys are ``up.1.*`` (convolution) and ``up.2.*`` (norm)."""

    def __init__(self, ch_in, ch_out, norm, act):
        super().__init__()
        mods, self.units = _entries(1, [(ch_in, ch_out)], norm)
        self.up = nn.ModuleDict(mods)


class _UnetFamily(_PackedWeightsModule):
    """The U-Net family of networks/unet_family.py: four encoder blocks, three UpConv + decoder block pairs, the 1x1x1 output head
    and three deep heads with nearest up-sampling of their logits -- the constructor's common part, forward() and the forward and
    backward programs.  A member names its blocks (ENCODER, DECODER) and supplies _make_block, _block_fwd, _block_bwd,
    _level_bwd, _top_fwd and _top_bwd.  A member with GATED set (networks/attunet.py) gets an AttentionBlock ``Att{i}`` between
    ``Up{i}`` and the decoder block of every level and supplies the two hooks _gate_fwd / _gate_bwd, which do nothing here."""
    _cpu_hint = "; move input/model to cuda"
    ENCODER = DECODER = ()  # attribute names of encoder blocks 1..4 / of decoder blocks 4..2
    GATED = False

    def __init__(self, norm_layer, act):
        """The family's refusals; the member's own come next, then _build."""
        super().__init__()
        if norm_layer in ("batch", "bcn", "none"):
            raise NotImplementedError(f"brats21_amd.{self.name}: --norm {norm_layer} is not built for this network (group | instance are)")
        if norm_layer not in ("group", "instance"):
            raise NotImplementedError(f"brats21_amd.{self.name} implements --norm group|instance (got {norm_layer!r})")
        if act == "prelu":
            raise NotImplementedError(f"brats21_amd.{self.name}: --act prelu is not built for this network")
        if act not in ("relu", "leakyrelu", "elu", "swish", "mish"):
            raise NotImplementedError(f"brats21_amd.{self.name} implements --act relu|leakyrelu|elu|swish|mish (got {act!r})")

    def _build(self, img_ch, output_ch, features, norm_layer, act, deep_supervision):
        self._check_shape_limits(img_ch, output_ch, features, 8)
        f = self.features = list(features)
        if len(f) != 4:
            raise ValueError(f"brats21_amd.{self.name}: features must hold four widths (got {f})")
        print(f"{self.name} features: {features}")
        self.deep_supervision = deep_supervision
        self.act = act
        self._init_dropout(0)  # (the reference's classes have no dropout)
        self._init_switches(pack_plan="0")
        for name, cin, cout in zip(self.ENCODER, (img_ch, f[0], f[1], f[2]), f):
            setattr(self, name, self._make_block(cin, cout, norm_layer, act))
        for i, name in zip((3, 2, 1), self.DECODER):
            setattr(self, f"Up{i + 1}", UpConv(f[i], f[i - 1], norm_layer, act))
            if self.GATED:  # (networks/unet_family.py:332-343, :430-441: f_int is the width of the level below, half of it at the top)
                setattr(self, f"Att{i + 1}", AttentionBlock(f[i - 1], f[i - 1], f[i - 2] if i > 1 else f[0] // 2, act))
            setattr(self, name, self._make_block(f[i], f[i - 1], norm_layer, act))
        self.Conv_1x1 = _ConvParams(f[0], output_ch, 1, bias=True)
        if deep_supervision:
            self.outconv4 = _ConvParams(f[3], output_ch, 1, bias=True)
            self.outconv3 = _ConvParams(f[2], output_ch, 1, bias=True)
            self.outconv2 = _ConvParams(f[1], output_ch, 1, bias=True)
        # init_weights(self, "kaiming"), networks/factory.py:203-224: kaiming-normal fan_out on the convolution weights; the biases
        # keep nn.Conv3d's default
        print("initialize network with kaiming")
        for mod in self.modules():
            if isinstance(mod, _ConvParams):
                nn.init.kaiming_normal_(mod.weight.data, a=0.0, mode="fan_out")

    def forward(self, x):
        if self.conv_fp8:
            raise NotImplementedError(f"brats21_amd.{self.name} with the e4m3 convolution path (conv_fp8) is not implemented")
        res = self._run(x)
        if not self.deep_supervision:
            return res
        out, deeps = res  # the reference returns the flat tuple (d1, d2, d3, d4)
        return (out, *deeps) if deeps else out

    def _gate_fwd(self, cx, level, g, x):
        """The skip tensor x of decoder level `level` (4, 3, 2) as its block reads it; g: the UpConv output beside it."""
        return x

    def _gate_bwd(self, cx, level, d_skip, d_u):
        """(d_skip, d_u) of the level's decoder block -> what _level_bwd and the UpConv's backward receive."""
        return d_skip, d_u

    def _program_fwd(self, ctx, cx, x0):
        enc, dec = [getattr(self, n) for n in self.ENCODER], [getattr(self, n) for n in self.DECODER]
        block = functools.partial(self._block_fwd, cx)

        def up(b, t):
            return _cgr_fwd(cx, b.units[0], ops.upsample_nearest(t, 2))

        # encoder (networks/unet_family.py:182-191, :270-281): the last pass of a level's block writes the skip tensor and its
        # max-pooled form
        x1, p1 = block(enc[0], x0, pool=True)
        x2, p2 = block(enc[1], p1, pool=True)
        x3, p3 = block(enc[2], p2, pool=True)
        x4 = block(enc[3], p3)
        # decoder (:194-204, :283-294): the blocks read the virtual concat [skip | up] from two pointers
        u4 = up(self.Up4, x4)
        d4_up = block(dec[0], self._gate_fwd(cx, 4, g=u4, x=x3), x2=u4)
        u3 = up(self.Up3, d4_up)
        d3_up = block(dec[1], self._gate_fwd(cx, 3, g=u3, x=x2), x2=u3)
        u2 = up(self.Up2, d3_up)
        outs = [self._top_fwd(ctx, cx, dec[2], self._gate_fwd(cx, 2, g=u2, x=x1), u2)]
        ctx.deep_scales = []
        if _deep_heads_on(self):
            # (:207-213, :298-304) 1x1x1 convolution at the source's resolution, then nearest up-sampling of the logit planes
            for hd, src, sc in ((self.outconv2, d3_up, 2), (self.outconv3, d4_up, 4), (self.outconv4, x4, 8)):
                outs.append(ops.planes_nearest(ops.head(src, hd.weight, hd.bias, 1), sc))
                ctx.heads.append((hd, src, 1))
                ctx.deep_scales.append(sc)
        ctx.bufs = (x1, x2, x3, x4, d4_up, d3_up)
        return tuple(outs)

    def _program_bwd(self, ctx, cx, *douts):
        enc, dec = [getattr(self, n) for n in self.ENCODER], [getattr(self, n) for n in self.DECODER]
        x1, x2, x3, x4, d4_up, d3_up = ctx.bufs
        # the deep heads' logit gradients at their sources' resolution, then all heads and the top of the decoder
        low = [douts[0]] + [None if d is None else ops.planes_nearest_bwd(d, sc) for d, sc in zip(douts[1:], ctx.deep_scales)]
        (d_x1, d_u), dsrc = self._top_bwd(ctx, cx, dec[2], low)
        d_x1, d_u = self._gate_bwd(cx, 2, d_x1, d_u)

        def up_bwd(b, d_up, src):  # (add: the gradient a deep head produced for the same activation)
            return ops.upsample_nearest_bwd(_cgr_bwd(cx, b.units[0], d_up), 2, add=dsrc.get(src.data_ptr()))

        d_x2, d_u = self._gate_bwd(cx, 3, *self._block_bwd(cx, dec[1], up_bwd(self.Up2, d_u, d3_up)))
        d_x3, d_u = self._gate_bwd(cx, 4, *self._block_bwd(cx, dec[0], up_bwd(self.Up3, d_u, d4_up)))
        d_p3, _ = self._block_bwd(cx, enc[3], up_bwd(self.Up4, d_u, x4))
        d_p2 = self._level_bwd(cx, enc[2], x3, d_p3, d_x3)
        d_p1 = self._level_bwd(cx, enc[1], x2, d_p2, d_x2)
        self._level_bwd(cx, enc[0], x1, d_p1, d_x1, need_dx=False)
        ctx.bufs = None


class Unet(_UnetFamily):
    """Constructor signature of networks/unet_family.py:135."""
    name = "Unet"
    ENCODER, DECODER = ("Conv1", "Conv2", "Conv3", "Conv4"), ("Up_conv4", "Up_conv3", "Up_conv2")
    _make_block = staticmethod(ConvBlock)

    def __init__(self, img_ch, output_ch, features, norm_layer="group", act="relu", deep_supervision=True):
        super().__init__(norm_layer, act)
        self._build(img_ch, output_ch, features, norm_layer, act, deep_supervision)
        self.norm_on_load = os.environ.get("BRATS_NORM_ON_LOAD", "1") != "0"

    def _block_fwd(self, cx, b, t, x2=None, pool=False):
        # (lazy: the activation between the two units has ONE reader, the block's second convolution)
        u1, u2 = b.units
        return _cgr_fwd(cx, u2, _cgr_fwd(cx, u1, t, x2=x2, lazy=True), pool=pool)

    def _block_bwd(self, cx, b, dout):
        c1, c2 = b.units
        dx = _cgr_bwd(cx, c1, _cgr_bwd(cx, c2, dout, bst=c1))
        return dx if isinstance(dx, tuple) else (dx, None)  # (the first unit read one tensor, or the pair [skip | up])

    def _level_bwd(self, cx, b, skip, d_pooled, d_skip, need_dx=True):
        c1, c2 = b.units
        return _cgr_bwd(cx, c1, _level_bwd(cx, c2, skip, d_pooled, d_skip, bst=c1), need_dx=need_dx)

    def _top_fwd(self, ctx, cx, b, x1, u):
        # d2_up feeds only the output head: where the fold is built the head reads the last unit's raw convolution output
        u1, last = b.units
        return _top_head_fwd(ctx, cx, last, _cgr_fwd(cx, u1, x1, x2=u, lazy=True), self.Conv_1x1)[0]

    def _top_bwd(self, ctx, cx, b, low):
        return _top_head_bwd(ctx, cx, *b.units, self.Conv_1x1, low)
