"""Unet (``--model modified_unet``): the plain U-Net of the reference's networks/unet_family.py:134-217 on the HIP kernels -- same
constructor, same ``state_dict`` keys / shapes / order (the reference's containers are nn.Sequentials, so the names are index
paths: ``Conv1.conv.0.weight``, ``Up4.up.1.bias``, ...), same ``forward(x) -> (d1, d2, d3, d4)`` flat tuple.

The units are EquiUnet's programs (networks/equiunet.py: _cgr_fwd / _cgr_bwd) with a learnable convolution bias; what differs from
EquiUnet is the shape of the program: no bottom block, an ``UpConv`` (nearest-neighbour x2 -> one unit) in front of every decoder
block, and deep heads that are 1x1x1 convolutions followed by NEAREST up-sampling of the logits (ops.upsample_nearest /
ops.planes_nearest and their adjoints, csrc/nearest.hip).

Built: ``--norm group | instance``, ``--act relu | leakyrelu | elu | swish | mish``, f32 / bf16 / fp16 storage and the split-precision
modes.  ``batch``, ``bcn``, ``none``, ``prelu`` and the e4m3 convolutions raise NotImplementedError.
"""
import functools
import os

import torch
import torch.nn as nn

from .. import ops
from ._program import _PackedWeightsModule, _fn_backward, _fn_forward, _heads_bwd
from .equiunet import _cgr_bwd, _cgr_fwd, _ConvParams, _deep_heads_on, _level_bwd, _NormParams, _unit_act


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


def _fold_top(cx, last):
    """May the output head ride on the last unit's raw convolution output (forward) / in its norm backward?  EquiUnet's rule."""
    m = cx.m
    kact, slope_t = _unit_act(last, cx.act)
    return (m.fold_head_fwd and kact in ("relu", "leakyrelu") and m.Conv_1x1.weight.shape[0] <= 4
            and (not cx.will_bwd or (m.fold_head_bwd and ops.head_fold_ok(m.Conv_1x1.weight, kact, slope_t))))


class _UnetFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, x, dtype, *params):
        return _fn_forward(_UnetFn._forward, ctx, model, x, dtype, params)

    @staticmethod
    def backward(ctx, *douts):
        return _fn_backward(_UnetFn._backward, ctx, douts)

    @staticmethod
    def _forward(ctx, cx, x0):
        m = cx.m
        cgr = functools.partial(_cgr_fwd, cx)

        def block(b, t, x2=None, pool=False):
            # (lazy: the activation between the two units has ONE reader, the block's second convolution)
            u1, u2 = b.units
            return cgr(u2, cgr(u1, t, x2=x2, lazy=True), pool=pool)

        def up(b, t):
            return cgr(b.units[0], ops.upsample_nearest(t, 2))

        # encoder (networks/unet_family.py:182-191): the last unit of a level writes the skip tensor and its max-pooled form
        x1, p1 = block(m.Conv1, x0, pool=True)
        x2, p2 = block(m.Conv2, p1, pool=True)
        x3, p3 = block(m.Conv3, p2, pool=True)
        x4 = block(m.Conv4, p3)
        # decoder (:194-204): the blocks read the virtual concat [skip | up] from two pointers
        d4_up = block(m.Up_conv4, x3, x2=up(m.Up4, x4))
        d3_up = block(m.Up_conv3, x2, x2=up(m.Up3, d4_up))
        u1, last = m.Up_conv2.units
        t = cgr(u1, x1, x2=up(m.Up2, d3_up), lazy=True)
        # d2_up feeds only the output head: where the fold is built the head reads the last unit's raw convolution output
        ctx.top_fused = _fold_top(cx, last)
        if ctx.top_fused:
            kact, _ = _unit_act(last, cx.act)
            d2_up = None
            outs = [ops.gn_head(cgr(last, t, no_act=True), cx.recs[last][5], m.Conv_1x1.weight, m.Conv_1x1.bias, kact)]
        else:
            d2_up = cgr(last, t)
            outs = [ops.head(d2_up, m.Conv_1x1.weight, m.Conv_1x1.bias, 1)]
        ctx.out_shape = tuple(outs[0].shape)
        ctx.heads = [(m.Conv_1x1, d2_up, 1)]
        ctx.deep_scales = []
        if _deep_heads_on(m):
            # (:207-213) 1x1x1 convolution at the source's resolution, then nearest up-sampling of the logit planes
            for hd, src, sc in ((m.outconv2, d3_up, 2), (m.outconv3, d4_up, 4), (m.outconv4, x4, 8)):
                outs.append(ops.planes_nearest(ops.head(src, hd.weight, hd.bias, 1), sc))
                ctx.heads.append((hd, src, 1))
                ctx.deep_scales.append(sc)
        ctx.bufs = (x1, x2, x3, x4, d4_up, d3_up, d2_up)
        return tuple(outs)

    @staticmethod
    def _backward(ctx, cx, *douts):
        m = cx.m
        x1, x2, x3, x4, d4_up, d3_up, d2_up = ctx.bufs
        cbw = functools.partial(_cgr_bwd, cx)
        level_bwd = functools.partial(_level_bwd, cx)
        # the deep heads' logit gradients at their sources' resolution, then all heads (the output head's backward rides in the
        # norm backward of the last unit where that is built)
        low = [douts[0]] + [None if d is None else ops.planes_nearest_bwd(d, sc) for d, sc in zip(douts[1:], ctx.deep_scales)]
        c1, c2 = m.Up_conv2.units
        top, dsrc = _heads_bwd(ctx, cx, low, m.fold_head_bwd and ops.head_fold_ok(m.Conv_1x1.weight, *_unit_act(c2, cx.act)))

        def extra(t):  # the gradient a deep head produced for the same activation
            return dsrc.get(t.data_ptr())

        def up_bwd(b, d_up, src):
            return ops.upsample_nearest_bwd(cbw(b.units[0], d_up), 2, add=extra(src))

        if top is not None:
            d = cbw(c2, None, head=top, bst=c1)
        else:
            d = cbw(c2, extra(d2_up) if extra(d2_up) is not None else torch.zeros_like(d2_up), bst=c1)
        d_x1, d_u = cbw(c1, d)
        c1, c2 = m.Up_conv3.units
        d_x2, d_u = cbw(c1, cbw(c2, up_bwd(m.Up2, d_u, d3_up), bst=c1))
        c1, c2 = m.Up_conv4.units
        d_x3, d_u = cbw(c1, cbw(c2, up_bwd(m.Up3, d_u, d4_up), bst=c1))
        c1, c2 = m.Conv4.units
        d_p3 = cbw(c1, cbw(c2, up_bwd(m.Up4, d_u, x4), bst=c1))
        c1, c2 = m.Conv3.units
        d_p2 = cbw(c1, level_bwd(c2, x3, d_p3, d_x3, bst=c1))
        c1, c2 = m.Conv2.units
        d_p1 = cbw(c1, level_bwd(c2, x2, d_p2, d_x2, bst=c1))
        c1, c2 = m.Conv1.units
        cbw(c1, level_bwd(c2, x1, d_p1, d_x1, bst=c1), need_dx=False)
        ctx.bufs = None


class Unet(_PackedWeightsModule):
    """Constructor signature of networks/unet_family.py:135."""
    name = "Unet"
    _cpu_hint = "; move input/model to cuda"

    def __init__(self, img_ch, output_ch, features, norm_layer="group", act="relu", deep_supervision=True):
        super().__init__()
        if norm_layer in ("batch", "bcn", "none"):
            raise NotImplementedError(f"brats21_amd.Unet: --norm {norm_layer} is not built for this network (group | instance are)")
        if norm_layer not in ("group", "instance"):
            raise NotImplementedError(f"brats21_amd.Unet implements --norm group|instance (got {norm_layer!r})")
        if act == "prelu":
            raise NotImplementedError("brats21_amd.Unet: --act prelu is not built for this network")
        if act not in ("relu", "leakyrelu", "elu", "swish", "mish"):
            raise NotImplementedError(f"brats21_amd.Unet implements --act relu|leakyrelu|elu|swish|mish (got {act!r})")
        self._check_shape_limits(img_ch, output_ch, features, 8)
        f = self.features = list(features)
        if len(f) != 4:
            raise ValueError(f"brats21_amd.Unet: features must hold four widths (got {f})")
        print(f"Unet features: {features}")
        self.deep_supervision = deep_supervision
        self.act = act
        self._init_dropout(0)  # (the reference's class has no dropout)
        self._init_switches(pack_plan="0")
        self.norm_on_load = os.environ.get("BRATS_NORM_ON_LOAD", "1") != "0"
        nl = norm_layer
        self.Conv1 = ConvBlock(img_ch, f[0], nl, act)
        self.Conv2 = ConvBlock(f[0], f[1], nl, act)
        self.Conv3 = ConvBlock(f[1], f[2], nl, act)
        self.Conv4 = ConvBlock(f[2], f[3], nl, act)
        self.Up4 = UpConv(f[3], f[2], nl, act)
        self.Up_conv4 = ConvBlock(f[3], f[2], nl, act)
        self.Up3 = UpConv(f[2], f[1], nl, act)
        self.Up_conv3 = ConvBlock(f[2], f[1], nl, act)
        self.Up2 = UpConv(f[1], f[0], nl, act)
        self.Up_conv2 = ConvBlock(f[1], f[0], nl, act)
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
            raise NotImplementedError("brats21_amd.Unet with the e4m3 convolution path (conv_fp8) is not implemented")
        res = self._run(_UnetFn, x)
        if not self.deep_supervision:
            return res
        out, deeps = res  # the reference returns the flat tuple (d1, d2, d3, d4)
        return (out, *deeps) if deeps else out
