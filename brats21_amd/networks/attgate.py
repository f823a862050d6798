"""AttentionBlock, the additive attention gate of the reference's AttUnet / R2AttUnet (networks/unet_family.py:104-131), as a
stand-alone module on the HIP kernels of csrc/attgate.hip: two 1x1x1 convolutions to f_int channels, each behind a BatchNorm3d,
added, activated, projected to ONE channel, BatchNorm3d(1), sigmoid -- and the skip tensor x scaled by that plane.  The norms are
nn.BatchNorm3d whatever ``--norm`` says (the reference hard-codes them), so the module carries running buffers and train() /
eval() select batch or running statistics.  The state-dict names are the reference's 21 (its containers are nn.Sequentials:
``W_g.0.weight`` ... ``psi.1.num_batches_tracked``), so its checkpoints load with strict=True.

The network programs that place the gate into the decoders of AttUnet / R2AttUnet (networks/attunet.py) call ops.attgate_fwd /
ops.attgate_bwd on their own NDHWC tensors, with this module as the holder of the parameters and running buffers; its forward() is
the same pair behind the reference's NCDHW float32 interface.

Built: ``act`` relu | leakyrelu | elu | swish | mish, f_g and f_l multiples of 8, any f_int >= 1, f32 / bf16 / fp16 storage
(``.storage``).  ``prelu`` (it would add a state-dict key) and the split-precision modes raise NotImplementedError."""
import torch
import torch.nn as nn

from .. import ops
from .._lib import BratsHipError
from .equiunet import _ConvParams, _NormParams

MAX_CHANNELS = 1024  # f_g, f_l: the streaming passes' limit in f32 storage, 256 channel vectors of 4
MAX_INT = 512        # f_int after padding to a multiple of 8
MOMENTUM = 0.1       # nn.BatchNorm3d's default


class _AttGateFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, x, block, save, *params):
        # save comes from AttentionBlock.forward: ctx.needs_input_grad does not see torch.no_grad()
        storage, training = block.storage, block.training
        gs, xs = ops.ncdhw_to_ndhwc(g, storage), ops.ncdhw_to_ndhwc(x, storage)
        out, saved, stats = ops.attgate_fwd(gs, xs, params, block.act, training=training, save=save,
                                            running=None if training else block._running())
        if training:
            block._update_running(stats, float(x.numel() // x.shape[1]))
        if save:
            ctx.saved, ctx.storage = saved, storage
            ctx.save_for_backward(*params)
        return ops.ndhwc_to_ncdhw(out)

    @staticmethod
    def backward(ctx, dout):
        params = ctx.saved_tensors
        dg, dx, grads = ops.attgate_bwd(ops.ncdhw_to_ndhwc(dout, ctx.storage), ctx.saved, params, need_dg=ctx.needs_input_grad[0],
                                        need_dx=ctx.needs_input_grad[1])
        ctx.saved = None
        dg = ops.ndhwc_to_ncdhw(dg) if dg is not None else None
        dx = ops.ndhwc_to_ncdhw(dx) if dx is not None else None
        return (dg, dx, None, None) + tuple(gr.reshape(p.shape) for gr, p in zip(grads, params))


class AttentionBlock(nn.Module):
    """Constructor signature of networks/unet_family.py:105; ``act`` is the name string, as everywhere here."""

    def __init__(self, f_g, f_l, f_int, act="relu"):
        super().__init__()
        if act == "prelu":
            raise NotImplementedError("brats21_amd.AttentionBlock: --act prelu is not built for this block (it adds a state-dict key)")
        if act not in ("relu", "leakyrelu", "elu", "swish", "mish"):
            raise NotImplementedError(f"brats21_amd.AttentionBlock implements --act relu|leakyrelu|elu|swish|mish (got {act!r})")
        for name, c in (("f_g", f_g), ("f_l", f_l)):
            if int(c) != c or c < 8 or c % 8 or c > MAX_CHANNELS:
                raise NotImplementedError(f"brats21_amd.AttentionBlock: the kernels need {name} to be a multiple of 8, at most {MAX_CHANNELS} "
                                          f"(got {c!r})")
        if int(f_int) != f_int or f_int < 1 or (f_int + 7) // 8 * 8 > MAX_INT:
            raise NotImplementedError(f"brats21_amd.AttentionBlock: f_int must be an integer from 1 to {MAX_INT} (got {f_int!r})")
        self.f_g, self.f_l, self.f_int, self.act = int(f_g), int(f_l), int(f_int), act
        self.storage = torch.float32
        self.W_g = nn.ModuleDict({"0": _ConvParams(self.f_g, self.f_int, 1, bias=True), "1": _NormParams(self.f_int, batch=True)})
        self.W_x = nn.ModuleDict({"0": _ConvParams(self.f_l, self.f_int, 1, bias=True), "1": _NormParams(self.f_int, batch=True)})
        self.psi = nn.ModuleDict({"0": _ConvParams(self.f_int, 1, 1, bias=True), "1": _NormParams(1, batch=True)})
        # init_weights(self, "kaiming") of the enclosing networks, networks/factory.py:203-224: kaiming-normal fan_out on the convolution
        # weights (the biases keep nn.Conv3d's default), BatchNorm weights ~ N(1, 0.02), BatchNorm biases 0
        for mod in self.modules():
            if isinstance(mod, _ConvParams):
                nn.init.kaiming_normal_(mod.weight.data, a=0.0, mode="fan_out")
            elif isinstance(mod, _NormParams):
                nn.init.normal_(mod.weight.data, 1.0, 0.02)
                nn.init.constant_(mod.bias.data, 0.0)

    def _norms(self):
        return self.W_g["1"], self.W_x["1"], self.psi["1"]

    def _running(self):
        return [b for bn in self._norms() for b in (bn.running_mean, bn.running_var)]

    def _update_running(self, stats, count):
        """nn.BatchNorm3d's buffer update from the finalisers' device tensors (no host read: a captured step replays it): momentum 0.1,
        the UNBIASED variance."""
        with torch.no_grad():
            for bn, (mean, var) in zip(self._norms(), stats):
                bn.running_mean.mul_(1.0 - MOMENTUM).add_(mean, alpha=MOMENTUM)
                bn.running_var.mul_(1.0 - MOMENTUM).add_(var, alpha=MOMENTUM * count / (count - 1.0))
                bn.num_batches_tracked += 1

    def train(self, mode=True):
        if mode != self.training:
            ops.invalidate_packed_weights()
        return super().train(mode)

    def forward(self, g, x):
        if not g.is_cuda or not x.is_cuda:
            raise BratsHipError("brats21_amd.networks.AttentionBlock runs on the GPU only (no CPU fallback); move input/model to cuda")
        if (g.dim() != 5 or x.dim() != 5 or g.shape[1] != self.f_g or x.shape[1] != self.f_l or g.shape[0] != x.shape[0]
                or g.shape[2:] != x.shape[2:]):
            raise ValueError(f"expected g [N, {self.f_g}, D, H, W] and x [N, {self.f_l}, D, H, W] of one extent")
        if self.training and x.numel() // x.shape[1] == 1:
            raise ValueError("brats21_amd.AttentionBlock: batch statistics need more than one value per channel (training mode, "
                             "N * D * H * W = 1); nn.BatchNorm3d refuses that too")
        if self.storage not in (torch.float32, torch.bfloat16, torch.float16):
            raise NotImplementedError(f"brats21_amd.AttentionBlock: storage {self.storage} (torch.float32, torch.bfloat16 or torch.float16)")
        if ops.x3_active():
            raise NotImplementedError("brats21_amd.AttentionBlock: the split-precision modes are not built for this block")
        params = tuple(self.parameters())
        grad = torch.is_grad_enabled()
        if grad:
            ops.invalidate_packed_weights()  # (weights written through p.data carry no version bump: _PackedWeightsModule's rule)
        # the inference variant (no_grad, or nothing to differentiate) keeps nothing
        save = grad and (g.requires_grad or x.requires_grad or any(p.requires_grad for p in params))
        return _AttGateFn.apply(g.float(), x.float(), self, save, *params)

    def extra_repr(self):
        return f"f_g={self.f_g}, f_l={self.f_l}, f_int={self.f_int}, act={self.act!r}"
