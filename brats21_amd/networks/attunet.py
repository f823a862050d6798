"""AttUnet and R2AttUnet: the two gated members of the reference's U-Net family (networks/unet_family.py:311-402, :405-499) on the
HIP kernels -- same constructors, same ``state_dict`` keys / shapes / order (``Up4.up.1.weight`` ... ``Att4.W_g.0.weight`` ...
``Att4.psi.1.num_batches_tracked``, ``Up_conv4.conv.0.weight`` ...: 139 / 153 keys, 112 / 126 of them parameters), same
``forward(x) -> (d1, d2, d3, d4)`` flat tuple.

The program is the family's (networks/unet.py: _UnetFamily) with its two gate hooks filled in: in front of every decoder block the
skip tensor goes through the additive attention gate (ops.attgate_fwd on the program's own NDHWC tensors, g = the UpConv output
beside it), and the block reads the virtual concat [gated skip | up] from two pointers as before; behind the block's backward,
ops.attgate_bwd turns the gated skip's gradient into the skip's and adds its gradient of g to the UpConv output's.  The gates are
networks.AttentionBlock modules (``Att4``, ``Att3``, ``Att2``): BatchNorm3d whatever ``--norm`` says, so these networks carry
running buffers -- updated from device tensors in every training-mode forward (a captured step replays the update), read in eval
mode.

R2AttUnet defers the gate's last pass: the gradient of a skip tensor there is one tensor, gate's dx + un-pooled gradient of the level
below, and brats_attgate_dx_unpool writes it in one pass once that level's backward has run (ops.AttGatePending.finish).  AttUnet's
level backward folds the skip and pooled gradients into its norm backward (ops.gn_act_bwd_pool): nothing to defer.

Built: what Unet / R2Unet build, without the split-precision modes (the gate has none).  ``batch``, ``bcn``, ``none``, ``prelu``, the
split-precision modes and the e4m3 convolutions raise NotImplementedError; AttentionBlock's channel limits apply.
"""
from .. import ops
from .r2unet import R2Unet
from .unet import Unet


class _Gated:
    """The attention gates of a family member: _gate_fwd / _gate_bwd of _UnetFamily on the member's ``Att{level}`` blocks."""
    GATED = True
    DEFER_DX = False  # True: _gate_bwd hands an ops.AttGatePending on as d_skip, which the member's _level_bwd finishes

    def _run(self, x):
        if self.precision in ("x3", "fp16x3", "bf16x3", "x3fwd", "x3bwd"):
            raise NotImplementedError(f"brats21_amd.{self.name}: the split-precision modes are not built for the attention gate "
                                      f"(precision = {self.precision!r}; auto | fp32 | bf16 | fp16 are)")
        return super()._run(x)

    def _gate_fwd(self, cx, level, g, x):
        b = getattr(self, f"Att{level}")
        training = self.training
        out, cx.recs[b], stats = ops.attgate_fwd(g, x, tuple(b.parameters()), cx.act, training=training, save=cx.will_bwd,
                                                 running=None if training else b._running())
        if training:  # (no_grad included, as torch does; device tensors, no host read)
            b._update_running(stats, float(x.numel() // x.shape[-1]))
        return out

    def _gate_bwd(self, cx, level, d_skip, d_u):
        b = getattr(self, f"Att{level}")
        params = tuple(b.parameters())
        dg, dx, grads = ops.attgate_bwd(d_skip, cx.recs.pop(b), params, defer_dx=self.DEFER_DX)
        for p, gr in zip(params, grads):  # each a finished sum: one cx.put
            cx.put(p, gr)
        return dx, ops.grad_sum(d_u, dg)


class AttUnet(_Gated, Unet):
    """Constructor signature of networks/unet_family.py:312."""
    name = "AttUnet"


class R2AttUnet(_Gated, R2Unet):
    """Constructor signature of networks/unet_family.py:406."""
    name = "R2AttUnet"
    DEFER_DX = True

    def _level_bwd(self, cx, b, skip, d_pooled, d_skip, need_dx=True):
        # d_skip: the gate's pending dx.  The level's output gradient is written by ONE pass from dout, t and the pooled gradient
        return self._block_bwd(cx, b, d_skip.finish(skip, d_pooled), need_dx)[0]
