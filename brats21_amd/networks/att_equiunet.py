"""AttEquiUnet: EquiUnet with a CBAM gate behind every encoder block, the bottom block and bottom_2 (drop-in for
``networks.equiunet2020.AttEquiUnet`` of the reference, networks/equiunet2020.py:238-249,503-561: same constructor, same
``state_dict`` keys / shapes / order, ``Unet.forward`` :374-405).  The units, the decoder and the heads are EquiUnet's programs
(networks/equiunet.py); the gates are ops.cbam_fwd / ops.cbam_bwd on the program's own NDHWC tensors.

A gate sits between a level's last unit and its pooling, so EquiUnet's two folds on that edge (normalise + act + pool in one pass,
pooling backward inside the norm backward) move to the gate's side: its last forward pass also writes the pooled tensor
(brats_cbam_apply_pool), and its two gradient-reading backward passes compose d_skip + maxpool_bwd(d_pooled) on load
(brats_cbam_bwd_reduce_pool / _bwd_apply_pool).  ``model.fold_gate_pool = False`` runs the plain composition instead (same bits).

Built for the reference's default gate: ``--norm instance`` (with group / bcn the reference itself fails, constructing
norm_layer(1) of the spatial gate), f32 and bf16 storage.  ``definer.get_model`` does not name the network yet; import the class.
"""
import functools
import os

import torch
import torch.nn as nn

from .. import ops
from ._program import _PackedWeightsModule
from .cbam import CBAM, MAX_CHANNELS
from .equiunet import (ConvBnRelu, UBlock, _blk, _cgr_bwd, _cgr_fwd, _ConvParams, _decoder_bwd, _decoder_fwd, _head, _plus)


class UBlockCbam(nn.Module):
    """networks/equiunet2020.py:238-249: keys ``UBlock.*`` then ``CBAM.*``."""

    def __init__(self, inplanes, midplanes, outplanes, dilation=(1, 1), norm="instance", act="relu"):
        super().__init__()
        self.UBlock = UBlock(inplanes, midplanes, outplanes, dilation, norm=norm, act=act)
        self.CBAM = CBAM(outplanes, norm_layer=norm)


def _gate_fwd(cx, cbam, x, pool=False):
    """CBAM on a unit's output -> gated tensor, or (gated, max-pooled gated) for a level that is pooled; what the backward needs
    goes to cx.recs[cbam].  The no-grad path keeps nothing and writes no index planes."""
    save, pooled = cx.will_bwd, None
    if pool and cx.m.fold_gate_pool:
        out, pooled, saved = ops.cbam_fwd(x, *cbam._params(), save=save, pool=True)
    else:
        out, saved = ops.cbam_fwd(x, *cbam._params(), save=save)
        if pool:
            pooled = ops.maxpool2(out, want_argmax=save)
    if save:
        cx.recs[cbam] = (x, saved, out)
    return (out, pooled) if pool else out


def _gate_bwd(cx, cbam, dout, d_pooled=None):
    """Backward of _gate_fwd -> the gradient of the gate's input; the seven parameter gradients go to cx.put.  d_pooled: the level
    was pooled, dout is the skip gradient."""
    x, saved, out = cx.recs[cbam]
    params = cbam._params()
    if d_pooled is not None and saved.pidx is None:  # (fold_gate_pool off: the composition, through a stored gradient)
        dout, d_pooled = ops.maxpool2_bwd(out, d_pooled, dx_skip=dout), None
    grads = ops.cbam_bwd(dout, x, saved, *params, d_pooled=d_pooled)
    for p, g in zip(params, grads[1:]):
        cx.put(p, g)
    return grads[0]


class AttEquiUnet(_PackedWeightsModule):
    """Constructor signature of networks/equiunet2020.py:503-505."""
    name = "AttEquiUnet"
    _cpu_hint = "; move input/model to cuda"

    def __init__(self, inplanes, num_classes, features, norm_layer=None, act="relu", deep_supervision=False, dropout=0):
        super().__init__()
        if norm_layer in ("group", "bcn"):
            raise ValueError(f"brats21_amd.AttEquiUnet: --norm {norm_layer} cannot normalise the ONE channel of the spatial gate "
                             "(8 groups) -- the reference fails the same way, constructing norm_layer(1)")
        if norm_layer == "batch":
            raise NotImplementedError("brats21_amd.AttEquiUnet: --norm batch is not built for the CBAM gate; use 'instance'")
        if norm_layer != "instance":
            raise NotImplementedError(f"brats21_amd.AttEquiUnet implements --norm instance (got {norm_layer!r})")
        if act not in ("relu", "leakyrelu", "elu", "prelu", "swish", "mish"):
            raise NotImplementedError(f"brats21_amd.AttEquiUnet implements --act relu|leakyrelu|elu|prelu|swish|mish (got {act!r})")
        self._check_shape_limits(inplanes, num_classes, features, 8)
        f = self.features = list(features)
        if len(f) != 4 or f[0] % 16 or any(c > MAX_CHANNELS for c in f):
            raise NotImplementedError(f"brats21_amd.AttEquiUnet: features = {f}: the gates take C // 16 >= 1, C % 8 == 0 and "
                                      f"C <= {MAX_CHANNELS} (features[0] a multiple of 16, features[3] <= {MAX_CHANNELS})")
        print(f"AttEquiUnet features: {features}")
        self.deep_supervision = deep_supervision
        self.act = act
        self._init_dropout(dropout)  # (the units' streams, as in EquiUnet; the gate has no dropout)
        self._init_switches(pack_plan="0")
        # the pooling behind a gate inside the gate's own passes (brats_cbam_apply_pool, brats_cbam_bwd_reduce_pool / _bwd_apply_pool);
        # 0: cbam_fwd -> maxpool2, maxpool2_bwd -> cbam_bwd, for same-box A/B runs and the bit-identity tests
        self.fold_gate_pool = os.environ.get("BRATS_FOLD_GATE_POOL", "1") != "0"
        self.norm_on_load = os.environ.get("BRATS_NORM_ON_LOAD", "1") != "0"
        nl = norm_layer
        self.encoder1 = UBlockCbam(inplanes, f[0], f[0], norm=nl, act=act)
        self.encoder2 = UBlockCbam(f[0], f[1], f[1], norm=nl, act=act)
        self.encoder3 = UBlockCbam(f[1], f[2], f[2], norm=nl, act=act)
        self.encoder4 = UBlockCbam(f[2], f[3], f[3], norm=nl, act=act)
        self.bottom = UBlockCbam(f[3], f[3], f[3], (2, 2), norm=nl, act=act)
        self.bottom_2 = nn.ModuleList([ConvBnRelu(f[3] * 2, f[2], norm=nl, act=act), CBAM(f[2], norm_layer=nl)])  # keys "bottom_2.0.*", "bottom_2.1.*"
        self.decoder3 = UBlock(f[2] * 2, f[2], f[1], norm=nl, act=act)
        self.decoder2 = UBlock(f[1] * 2, f[1], f[0], norm=nl, act=act)
        self.decoder1 = UBlock(f[0] * 2, f[0], f[0], norm=nl, act=act)
        self.outconv = _ConvParams(f[0], num_classes, 1, bias=True)
        if deep_supervision:
            self.deep_bottom = _head(f[3], num_classes)
            self.deep_bottom2 = _head(f[2], num_classes)
            self.deep3 = _head(f[1], num_classes)
            self.deep2 = _head(f[0], num_classes)
        self._unit_ids = {u: i for i, u in enumerate(mod for mod in self.modules() if isinstance(mod, ConvBnRelu))}
        # init_weights(self, "kaiming"), networks/factory.py:203-224: kaiming-normal fan_out on the convolution and Linear weights
        # (the gates' own: CBAM.reset_parameters)
        print("initialize network with kaiming")
        for mod in self.modules():
            if isinstance(mod, _ConvParams):
                nn.init.kaiming_normal_(mod.weight.data, a=0.0, mode="fan_out")

    def forward(self, x):
        if self._dtype() == torch.float16:
            raise NotImplementedError("brats21_amd.AttEquiUnet: fp16 storage is not built for the CBAM gates (use bf16 autocast / "
                                      "precision='bf16', 'fp32' or an x3 mode)")
        if self.conv_fp8:
            raise NotImplementedError("brats21_amd.AttEquiUnet with the e4m3 convolution path (conv_fp8) is not implemented")
        return self._run(x)

    def _program_fwd(self, ctx, cx, x0):
        m = cx.m
        cgr = functools.partial(_cgr_fwd, cx)

        def level(enc, t, pool=False):
            # unit 1 runs lazy into unit 2; unit 2's output is materialised (the gate reads it three times), then the gate
            c1, c2 = _blk(enc.UBlock)
            return _gate_fwd(cx, enc.CBAM, cgr(c2, cgr(c1, t, lazy=True)), pool=pool)

        down1, p1 = level(m.encoder1, x0, pool=True)
        down2, p2 = level(m.encoder2, p1, pool=True)
        down3, p3 = level(m.encoder3, p2, pool=True)
        down4 = level(m.encoder4, p3)
        bottom = level(m.bottom, down4)
        bottom_2 = _gate_fwd(cx, m.bottom_2[1], cgr(m.bottom_2[0], down4, x2=bottom))
        # the decoder and the heads are EquiUnet's; the deep heads read the gated bottom / bottom_2
        return tuple(_decoder_fwd(ctx, cx, down1, down2, down3, down4, bottom, bottom_2))

    def _program_bwd(self, ctx, cx, *douts):
        m = cx.m
        cbw = functools.partial(_cgr_bwd, cx)
        gbw = functools.partial(_gate_bwd, cx)

        def level(enc, dout, d_pooled=None, need_dx=True):
            c1, c2 = _blk(enc.UBlock)
            return cbw(c1, cbw(c2, gbw(enc.CBAM, dout, d_pooled), bst=c1), need_dx=need_dx)

        d_skip1, d_skip2, d_skip3, d_b2, d_deep_bottom = _decoder_bwd(ctx, cx, douts)
        d_skip4, d_bot = cbw(m.bottom_2[0], gbw(m.bottom_2[1], d_b2))
        d_down4 = d_skip4 + level(m.bottom, _plus(d_bot, d_deep_bottom))
        d_p3 = level(m.encoder4, d_down4)
        d_p2 = level(m.encoder3, d_skip3, d_p3)
        d_p1 = level(m.encoder2, d_skip2, d_p2)
        level(m.encoder1, d_skip1, d_p1, need_dx=False)
        ctx.bufs = None
