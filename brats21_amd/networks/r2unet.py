"""R2Unet: the recurrent residual U-Net of the reference's networks/unet_family.py:220-308 on the HIP kernels -- same constructor,
same ``state_dict`` keys / shapes / order (``RRCNN1.RCNN.0.conv.0.weight`` ... ``Up4.up.1.bias`` ... ``outconv2.bias``), same
``forward(x) -> (d1, d2, d3, d4)`` flat tuple.

The program is Unet's (networks/unet.py) with every ConvBlock replaced by an RRCNNblock: the blocks are ops.rrcnn_fwd / ops.rrcnn_bwd
on the network's own NDHWC tensors -- the decoder blocks read the virtual concat [skip | up] from two pointers --, an encoder block's
last normalise pass writes the skip tensor AND its max-pooled form (ops.rrcnn_fwd(pool=True)), the ``UpConv`` units, the 1x1x1 heads
with nearest up-sampling of the logits and the deep heads' gradients are Unet's.  There is no head fold: a block's last pass is a
residual sum, not a plain normalise + act.

Built: ``--norm group | instance``, ``--act relu | leakyrelu | elu | swish | mish``, t >= 1, f32 / bf16 / fp16 storage.  ``batch``,
``bcn``, ``none``, ``prelu``, the split-precision modes and the e4m3 convolutions raise NotImplementedError.
"""
import torch
import torch.nn as nn

from .. import ops
from ._program import _PackedWeightsModule, _fn_backward, _fn_forward, _heads_bwd
from .equiunet import _cgr_bwd, _cgr_fwd, _ConvParams, _deep_heads_on
from .rrcnn import RRCNNblock
from .unet import UpConv


class _R2UnetFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, x, dtype, *params):
        return _fn_forward(_R2UnetFn._forward, ctx, model, x, dtype, params, cpad=model._cpad)

    @staticmethod
    def backward(ctx, *douts):
        return _fn_backward(_R2UnetFn._backward, ctx, douts)

    @staticmethod
    def _forward(ctx, cx, x0):
        m = cx.m
        save = cx.will_bwd
        ctx.saved = {}

        def block(b, t, x2=None, pool=False):
            out, ctx.saved[b] = ops.rrcnn_fwd(t, x2, tuple(b.parameters()), b.groups, cx.act, b.t, save=save, pool=pool)
            return out

        def up(b, t):
            return _cgr_fwd(cx, b.units[0], ops.upsample_nearest(t, 2))

        # encoder (networks/unet_family.py:270-281): the last pass of a level's block writes the skip tensor and its max-pooled form
        x1, p1 = block(m.RRCNN1, x0, pool=True)
        x2, p2 = block(m.RRCNN2, p1, pool=True)
        x3, p3 = block(m.RRCNN3, p2, pool=True)
        x4 = block(m.RRCNN4, p3)
        # decoder (:283-294): the blocks' 1x1x1 convolutions read the virtual concat [skip | up] from two pointers
        d4_up = block(m.Up_RRCNN4, x3, x2=up(m.Up4, x4))
        d3_up = block(m.Up_RRCNN3, x2, x2=up(m.Up3, d4_up))
        d2_up = block(m.Up_RRCNN2, x1, x2=up(m.Up2, d3_up))
        ctx.top_fused = False  # (the last pass is a residual sum: no head fold)
        outs = [ops.head(d2_up, m.Conv_1x1.weight, m.Conv_1x1.bias, 1)]
        ctx.out_shape = tuple(outs[0].shape)
        ctx.heads = [(m.Conv_1x1, d2_up, 1)]
        ctx.deep_scales = []
        if _deep_heads_on(m):
            # (:298-304) 1x1x1 convolution at the source's resolution, then nearest up-sampling of the logit planes
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
        low = [douts[0]] + [None if d is None else ops.planes_nearest_bwd(d, sc) for d, sc in zip(douts[1:], ctx.deep_scales)]
        _, dsrc = _heads_bwd(ctx, cx, low, False)

        def extra(t):  # the gradient a head produced for the activation
            return dsrc.get(t.data_ptr())

        def block_bwd(b, dout, need_dx=True):
            # every parameter gradient of the block is finished by rrcnn_bwd: one cx.put each
            dx, dx2, grads = ops.rrcnn_bwd(dout, ctx.saved.pop(b), tuple(b.parameters()), need_dx=need_dx)
            for p, g in zip(b.parameters(), grads):
                cx.put(p, g)
            return dx, dx2

        def up_bwd(b, d_up, src):
            return ops.upsample_nearest_bwd(_cgr_bwd(cx, b.units[0], d_up), 2, add=extra(src))

        def level_bwd(b, skip, d_pooled, d_skip, need_dx=True):
            # the level's output gradient: ONE tensor, read by the block's last norm backward and by the residual's sum
            return block_bwd(b, ops.maxpool2_bwd(skip, d_pooled, dx_skip=d_skip), need_dx)[0]

        d = extra(d2_up)
        d_x1, d_u = block_bwd(m.Up_RRCNN2, d if d is not None else torch.zeros_like(d2_up))
        d_x2, d_u = block_bwd(m.Up_RRCNN3, up_bwd(m.Up2, d_u, d3_up))
        d_x3, d_u = block_bwd(m.Up_RRCNN4, up_bwd(m.Up3, d_u, d4_up))
        d_p3, _ = block_bwd(m.RRCNN4, up_bwd(m.Up4, d_u, x4))
        d_p2 = level_bwd(m.RRCNN3, x3, d_p3, d_x3)
        d_p1 = level_bwd(m.RRCNN2, x2, d_p2, d_x2)
        level_bwd(m.RRCNN1, x1, d_p1, d_x1, need_dx=False)
        ctx.bufs = ctx.saved = None


class R2Unet(_PackedWeightsModule):
    """Constructor signature of networks/unet_family.py:221."""
    name = "R2Unet"
    _cpu_hint = "; move input/model to cuda"

    def __init__(self, img_ch, output_ch, features, t=2, norm_layer="group", act="relu", deep_supervision=True):
        super().__init__()
        if norm_layer in ("batch", "bcn", "none"):
            raise NotImplementedError(f"brats21_amd.R2Unet: --norm {norm_layer} is not built for this network (group | instance are)")
        if norm_layer not in ("group", "instance"):
            raise NotImplementedError(f"brats21_amd.R2Unet implements --norm group|instance (got {norm_layer!r})")
        if act == "prelu":
            raise NotImplementedError("brats21_amd.R2Unet: --act prelu is not built for this network")
        if act not in ("relu", "leakyrelu", "elu", "swish", "mish"):
            raise NotImplementedError(f"brats21_amd.R2Unet implements --act relu|leakyrelu|elu|swish|mish (got {act!r})")
        if int(t) != t or t < 1:
            raise ValueError(f"brats21_amd.R2Unet: t must be an integer >= 1 (got {t!r})")
        self._check_shape_limits(img_ch, output_ch, features, 8)
        f = self.features = list(features)
        if len(f) != 4:
            raise ValueError(f"brats21_amd.R2Unet: features must hold four widths (got {f})")
        print(f"R2Unet features: {features}")
        self.deep_supervision = deep_supervision
        self.act, self.t = act, int(t)
        self._init_dropout(0)  # (the reference's class has no dropout)
        self._init_switches(pack_plan="0")
        # the network input is zero-padded to a channel vector in every storage type, as RRCNNblock pads a narrow input
        self._cpad = 8 if self.inplanes <= 8 else 16
        nl, kw = norm_layer, dict(norm_layer=norm_layer, act=act, t=self.t)
        self.RRCNN1 = RRCNNblock(img_ch, f[0], **kw)
        self.RRCNN2 = RRCNNblock(f[0], f[1], **kw)
        self.RRCNN3 = RRCNNblock(f[1], f[2], **kw)
        self.RRCNN4 = RRCNNblock(f[2], f[3], **kw)
        self.Up4 = UpConv(f[3], f[2], nl, act)
        self.Up_RRCNN4 = RRCNNblock(f[3], f[2], **kw)
        self.Up3 = UpConv(f[2], f[1], nl, act)
        self.Up_RRCNN3 = RRCNNblock(f[2], f[1], **kw)
        self.Up2 = UpConv(f[1], f[0], nl, act)
        self.Up_RRCNN2 = RRCNNblock(f[1], f[0], **kw)
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
            raise NotImplementedError("brats21_amd.R2Unet with the e4m3 convolution path (conv_fp8) is not implemented")
        if self.precision in ("x3", "fp16x3", "bf16x3", "x3fwd", "x3bwd"):
            raise NotImplementedError(f"brats21_amd.R2Unet: the split-precision modes are not built for the recurrent block "
                                      f"(precision = {self.precision!r}; auto | fp32 | bf16 | fp16 are)")
        res = self._run(_R2UnetFn, x)
        if not self.deep_supervision:
            return res
        out, deeps = res  # the reference returns the flat tuple (d1, d2, d3, d4)
        return (out, *deeps) if deeps else out
