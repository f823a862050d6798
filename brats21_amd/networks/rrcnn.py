"""RRCNNblock, the recurrent residual block of the reference's R2U-Net family (networks/unet_family.py:60-101), as a stand-alone
module on the HIP kernels: a 1x1x1 convolution with bias gives x0; two RecurrentBlocks follow, each applying ONE conv3x3x3 (bias)
-> norm -> act unit t + 1 times, to its input and then to input + previous result; the block returns x0 + their result.  The
state-dict names are the reference's (its containers are nn.Sequentials: ``RCNN.0.conv.0.weight`` ... ``Conv_1x1.bias``), so its
checkpoints load with strict=True.

The network program that will place the block into R2Unet calls ops.rrcnn_fwd / ops.rrcnn_bwd on its own NDHWC tensors (the decoder
blocks with the virtual concat [skip | up] as two sources); this module is the same pair behind the reference's NCDHW float32
interface.

Built: ``norm_layer`` "group" (8 groups) | "instance", ``act`` relu | leakyrelu | elu | swish | mish, t >= 1, f32 / bf16 / fp16
storage (``.storage``).  ``batch``, ``bcn``, ``none``, ``prelu`` and the split-precision modes raise NotImplementedError."""
import torch
import torch.nn as nn

from .. import ops
from .._lib import BratsHipError
from .equiunet import _ConvParams, _NormParams

MAX_CHANNELS = 1024  # affine_act's limit in f32 storage: 256 channel vectors of 4 (16-bit storage would take 2048)
MAX_NARROW = 16      # widest input that is zero-padded to a channel vector (8 or 16 channels)


class _RrcnnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, x2, block, save, *params):
        # save comes from RRCNNblock.forward: ctx.needs_input_grad does not see torch.no_grad()
        storage = block.storage
        cpad = block._cpad if x2 is None else None
        xs = ops.ncdhw_to_ndhwc(x, storage, cpad=cpad)
        xs2 = ops.ncdhw_to_ndhwc(x2, storage) if x2 is not None else None
        out, saved = ops.rrcnn_fwd(xs, xs2, params, block.groups, block.act, block.t, save=save)
        if save:
            ctx.saved, ctx.storage, ctx.cin = saved, storage, x.shape[1]
            ctx.need_dx = ctx.needs_input_grad[0] or (x2 is not None and ctx.needs_input_grad[1])
            ctx.save_for_backward(*params)
        return ops.ndhwc_to_ncdhw(out)

    @staticmethod
    def backward(ctx, dout):
        params = ctx.saved_tensors
        dx, dx2, grads = ops.rrcnn_bwd(ops.ncdhw_to_ndhwc(dout, ctx.storage), ctx.saved, params, need_dx=ctx.need_dx)
        ctx.saved = None
        if dx is not None:
            dx = ops.ndhwc_to_ncdhw(dx[..., :ctx.cin] if dx.shape[-1] != ctx.cin else dx)  # (a padded narrow input: its own channels)
            dx2 = ops.ndhwc_to_ncdhw(dx2) if dx2 is not None else None
        return (dx, dx2, None, None) + tuple(g.reshape(p.shape) for g, p in zip(grads, params))


class RecurrentBlock(nn.Module):
    """networks/unet_family.py:60-86: keys ``conv.0.*`` (convolution), ``conv.1.*`` (norm); entry 2, the activation, has none."""

    def __init__(self, ch_out):
        super().__init__()
        self.conv = nn.ModuleDict({"0": _ConvParams(ch_out, ch_out, 3, bias=True), "1": _NormParams(ch_out)})


class RRCNNblock(nn.Module):
    """Constructor signature of networks/unet_family.py:90, with ``norm_layer`` the name string the networks here take (the
    reference passes the callable it made from the same name)."""

    def __init__(self, ch_in, ch_out, norm_layer="group", act="relu", t=2):
        super().__init__()
        if norm_layer in ("batch", "bcn", "none"):
            raise NotImplementedError(f"brats21_amd.RRCNNblock: --norm {norm_layer} is not built for this block (group | instance are)")
        if norm_layer not in ("group", "instance"):
            raise NotImplementedError(f"brats21_amd.RRCNNblock implements --norm group|instance (got {norm_layer!r})")
        if act == "prelu":
            raise NotImplementedError("brats21_amd.RRCNNblock: --act prelu is not built for this block")
        if act not in ("relu", "leakyrelu", "elu", "swish", "mish"):
            raise NotImplementedError(f"brats21_amd.RRCNNblock implements --act relu|leakyrelu|elu|swish|mish (got {act!r})")
        if int(t) != t or t < 1:
            raise ValueError(f"brats21_amd.RRCNNblock: t must be an integer >= 1 (got {t!r}); the reference's block returns the integer 0 "
                             "from a RecurrentBlock with t = 0")
        if int(ch_in) != ch_in or int(ch_out) != ch_out or ch_in < 1 or ch_out < 1:
            raise ValueError(f"brats21_amd.RRCNNblock: ch_in and ch_out must be positive integers (got {ch_in!r}, {ch_out!r})")
        if ch_out % 8 or ch_out > MAX_CHANNELS:
            raise NotImplementedError(f"brats21_amd.RRCNNblock: the kernels need ch_out to be a multiple of 8, at most {MAX_CHANNELS} "
                                      f"(got {ch_out})")
        if ch_in > MAX_NARROW and ch_in % 8:
            raise NotImplementedError(f"brats21_amd.RRCNNblock: ch_in must be 1 .. {MAX_NARROW} or a multiple of 8 (got {ch_in})")
        self.ch_in, self.ch_out, self.t, self.act, self.norm_layer = int(ch_in), int(ch_out), int(t), act, norm_layer
        self.groups = 8 if norm_layer == "group" else self.ch_out
        # a narrow input is zero-padded to a channel vector by the layout conversion (the weight's columns alike, its gradient
        # sliced back)
        self._cpad = None if self.ch_in % 8 == 0 else (8 if self.ch_in < 8 else 16)
        self.storage = torch.float32
        self.RCNN = nn.ModuleDict({"0": RecurrentBlock(self.ch_out), "1": RecurrentBlock(self.ch_out)})
        self.Conv_1x1 = _ConvParams(self.ch_in, self.ch_out, 1, bias=True)
        # init_weights(self, "kaiming") of the enclosing networks, networks/factory.py:203-224: kaiming-normal fan_out on the convolution
        # weights; the biases keep nn.Conv3d's default
        for mod in self.modules():
            if isinstance(mod, _ConvParams):
                nn.init.kaiming_normal_(mod.weight.data, a=0.0, mode="fan_out")

    def train(self, mode=True):
        if mode != self.training:
            ops.invalidate_packed_weights()
        return super().train(mode)

    def forward(self, x, x2=None):
        if not x.is_cuda or (x2 is not None and not x2.is_cuda):
            raise BratsHipError("brats21_amd.networks.RRCNNblock runs on the GPU only (no CPU fallback); move input/model to cuda")
        cin = x.shape[1] + (x2.shape[1] if x2 is not None else 0) if x.dim() == 5 and (x2 is None or x2.dim() == 5) else -1
        if cin != self.ch_in or (x2 is not None and (x2.shape[0] != x.shape[0] or x2.shape[2:] != x.shape[2:])):
            raise ValueError(f"expected input [N, {self.ch_in}, D, H, W] (or two tensors whose channels add up to {self.ch_in})")
        if x2 is not None and (x.shape[1] % 8 or x2.shape[1] % 8):
            raise NotImplementedError("brats21_amd.RRCNNblock: each of two sources must have a multiple of 8 channels")
        if self.storage not in (torch.float32, torch.bfloat16, torch.float16):
            raise NotImplementedError(f"brats21_amd.RRCNNblock: storage {self.storage} (torch.float32, torch.bfloat16 or torch.float16)")
        if ops.x3_active():
            raise NotImplementedError("brats21_amd.RRCNNblock: the split-precision modes are not built for this block")
        params = tuple(self.parameters())
        grad = torch.is_grad_enabled()
        if grad:
            ops.invalidate_packed_weights()  # (weights written through p.data carry no version bump: _PackedWeightsModule's rule)
        # the inference variant (no_grad, or nothing to differentiate) keeps nothing and reuses four activation buffers
        save = grad and (x.requires_grad or (x2 is not None and x2.requires_grad) or any(p.requires_grad for p in params))
        return _RrcnnFn.apply(x.float(), None if x2 is None else x2.float(), self, save, *params)

    def extra_repr(self):
        return f"ch_in={self.ch_in}, ch_out={self.ch_out}, norm_layer={self.norm_layer!r}, act={self.act!r}, t={self.t}"
