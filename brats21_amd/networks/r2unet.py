"""R2Unet: the recurrent residual U-Net of the reference's networks/unet_family.py:220-308 on the HIP kernels -- same constructor,
same ``state_dict`` keys / shapes / order (``RRCNN1.RCNN.0.conv.0.weight`` ... ``Up4.up.1.bias`` ... ``outconv2.bias``), same
``forward(x) -> (d1, d2, d3, d4)`` flat tuple.

The program is the family's (networks/unet.py: _UnetFamily) with an RRCNNblock where Unet has a ConvBlock: the blocks are
ops.rrcnn_fwd / ops.rrcnn_bwd on the network's own NDHWC tensors -- the decoder blocks read the virtual concat [skip | up] from two
pointers --, an encoder block's last normalise pass writes the skip tensor AND its max-pooled form (ops.rrcnn_fwd(pool=True)), the
``UpConv`` units, the 1x1x1 heads with nearest up-sampling of the logits and the deep heads' gradients are the family's.  There is
no head fold: a block's last pass is a residual sum, not a plain normalise + act.

Built: ``--norm group | instance``, ``--act relu | leakyrelu | elu | swish | mish``, t >= 1, f32 / bf16 / fp16 storage.  ``batch``,
``bcn``, ``none``, ``prelu``, the split-precision modes and the e4m3 convolutions raise NotImplementedError.
"""
import torch

from .. import ops
from ._program import _heads_bwd
from .rrcnn import RRCNNblock
from .unet import _UnetFamily


class R2Unet(_UnetFamily):
    """Constructor signature of networks/unet_family.py:221."""
    name = "R2Unet"
    ENCODER, DECODER = ("RRCNN1", "RRCNN2", "RRCNN3", "RRCNN4"), ("Up_RRCNN4", "Up_RRCNN3", "Up_RRCNN2")

    def __init__(self, img_ch, output_ch, features, t=2, norm_layer="group", act="relu", deep_supervision=True):
        super().__init__(norm_layer, act)
        if int(t) != t or t < 1:
            raise ValueError(f"brats21_amd.R2Unet: t must be an integer >= 1 (got {t!r})")
        self.t = int(t)
        self._build(img_ch, output_ch, features, norm_layer, act, deep_supervision)
        # the network input is zero-padded to a channel vector in every storage type, as RRCNNblock pads a narrow input
        self._cpad = 8 if self.inplanes <= 8 else 16

    def _make_block(self, ch_in, ch_out, norm_layer, act):
        return RRCNNblock(ch_in, ch_out, norm_layer=norm_layer, act=act, t=self.t)

    def _run(self, x):
        if self.precision in ("x3", "fp16x3", "bf16x3", "x3fwd", "x3bwd"):
            raise NotImplementedError(f"brats21_amd.R2Unet: the split-precision modes are not built for the recurrent block "
                                      f"(precision = {self.precision!r}; auto | fp32 | bf16 | fp16 are)")
        return super()._run(x)

    def _block_fwd(self, cx, b, t, x2=None, pool=False):
        out, cx.recs[b] = ops.rrcnn_fwd(t, x2, tuple(b.parameters()), b.groups, cx.act, b.t, save=cx.will_bwd, pool=pool)
        return out

    def _block_bwd(self, cx, b, dout, need_dx=True):
        # every parameter gradient of the block is finished by rrcnn_bwd: one cx.put each
        dx, dx2, grads = ops.rrcnn_bwd(dout, cx.recs.pop(b), tuple(b.parameters()), need_dx=need_dx)
        for p, g in zip(b.parameters(), grads):
            cx.put(p, g)
        return dx, dx2

    def _level_bwd(self, cx, b, skip, d_pooled, d_skip, need_dx=True):
        # the level's output gradient: ONE tensor, read by the block's last norm backward and by the residual's sum
        return self._block_bwd(cx, b, ops.maxpool2_bwd(skip, d_pooled, dx_skip=d_skip), need_dx)[0]

    def _top_fwd(self, ctx, cx, b, x1, u):
        d2_up = self._block_fwd(cx, b, x1, x2=u)
        ctx.top_fused = False  # (the last pass is a residual sum: no head fold)
        logits = ops.head(d2_up, self.Conv_1x1.weight, self.Conv_1x1.bias, 1)
        ctx.out_shape = tuple(logits.shape)
        ctx.heads = [(self.Conv_1x1, d2_up, 1)]
        return logits

    def _top_bwd(self, ctx, cx, b, low):
        _, dsrc = _heads_bwd(ctx, cx, low, False)
        d2_up = ctx.heads[0][1]
        d = dsrc.get(d2_up.data_ptr())
        return self._block_bwd(cx, b, d if d is not None else torch.zeros_like(d2_up)), dsrc
