"""CBAM attention block of the reference's AttEquiUnet (networks/equiunet2020.py:147-235) as a stand-alone module on the HIP
kernels of csrc/cbam.hip: channel gate (global avg + max pool, shared MLP, sigmoid), then spatial gate (7x7x7 convolution over the
per-voxel channel [max | mean], InstanceNorm3d(1, affine), ReLU, sigmoid).  The state-dict names are the reference's, so its
checkpoints load with strict=True.  The network program that places the block into EquiUnet calls ops.cbam_fwd / ops.cbam_bwd on its
own NDHWC tensors; this module is the same pair behind the reference's NCDHW float32 interface."""
import torch
import torch.nn as nn

from .. import ops
from .._lib import BratsHipError

MAX_CHANNELS = 512


class _Params(nn.Module):
    """A bare container: gives the parameters the reference's dotted names."""


class _CbamFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, storage, save, *params):
        # save comes from CBAM.forward: ctx.needs_input_grad does not see torch.no_grad()
        xs = ops.ncdhw_to_ndhwc(x, storage)
        out, saved = ops.cbam_fwd(xs, *params, save=save)
        if save:
            ctx.saved, ctx.storage = saved, storage
            ctx.save_for_backward(xs, *params)
        return ops.ndhwc_to_ncdhw(out)

    @staticmethod
    def backward(ctx, dout):
        xs, *params = ctx.saved_tensors
        grads = ops.cbam_bwd(ops.ncdhw_to_ndhwc(dout, ctx.storage), xs, ctx.saved, *params)
        return (ops.ndhwc_to_ncdhw(grads[0]), None, None) + tuple(grads[1:])


class CBAM(nn.Module):
    def __init__(self, gate_channels, reduction_ratio=16, pool_types=None, norm_layer="instance"):
        super().__init__()
        if pool_types is not None and list(pool_types) != ["avg", "max"]:
            raise NotImplementedError(f"CBAM: pool_types {pool_types!r} (only the reference's default ['avg', 'max'] is built)")
        if norm_layer == "group":
            raise ValueError("CBAM: the spatial gate normalises ONE channel; num_channels (1) must be divisible by num_groups (8) -- "
                             "the reference fails the same way with --norm group")
        if norm_layer == "bcn":
            raise ValueError("CBAM: the spatial gate normalises ONE channel, which BCNorm's 8 groups cannot take -- the reference raises "
                             "inside BCNorm with --norm bcn")
        if norm_layer == "batch":
            raise NotImplementedError("CBAM: norm_layer='batch' is not built yet (it comes with the pull request that wires the block "
                                      "into att_equiunet); use 'instance'")
        if norm_layer != "instance":
            raise ValueError(f"CBAM: unknown norm_layer {norm_layer!r}")
        c, r = int(gate_channels), int(reduction_ratio)
        if c % 8 or c > MAX_CHANNELS or r < 1 or c // r < 1:
            raise NotImplementedError(f"CBAM: gate_channels = {c}, reduction_ratio = {r}: the kernels take C % 8 == 0, C <= {MAX_CHANNELS} and "
                                      "C // reduction_ratio >= 1")
        self.gate_channels, self.reduction_ratio, self.storage = c, r, torch.float32
        ch = c // r
        mlp = _Params()
        lin1, lin3 = _Params(), _Params()
        lin1.weight, lin1.bias = nn.Parameter(torch.empty(ch, c)), nn.Parameter(torch.empty(ch))
        lin3.weight, lin3.bias = nn.Parameter(torch.empty(c, ch)), nn.Parameter(torch.empty(c))
        mlp.add_module("1", lin1)
        mlp.add_module("3", lin3)
        self.ChannelGate = _Params()
        self.ChannelGate.mlp = mlp
        spatial = _Params()
        spatial.conv, spatial.bn = _Params(), _Params()
        spatial.conv.weight = nn.Parameter(torch.empty(1, 2, 7, 7, 7))
        spatial.bn.weight, spatial.bn.bias = nn.Parameter(torch.ones(1)), nn.Parameter(torch.zeros(1))
        self.SpatialGate = _Params()
        self.SpatialGate.spatial = spatial
        self.reset_parameters()

    def reset_parameters(self):
        """init_weights(init_type='kaiming') of the reference on the Linear and Conv weights; nn.Linear's own bias init."""
        for lin in (self.ChannelGate.mlp._modules["1"], self.ChannelGate.mlp._modules["3"]):
            nn.init.kaiming_normal_(lin.weight, a=0.0, mode="fan_out")
            bound = 1.0 / lin.weight.shape[1] ** 0.5
            nn.init.uniform_(lin.bias, -bound, bound)
        nn.init.kaiming_normal_(self.SpatialGate.spatial.conv.weight, a=0.0, mode="fan_out")

    def _params(self):
        m, sp = self.ChannelGate.mlp._modules, self.SpatialGate.spatial
        return (m["1"].weight, m["1"].bias, m["3"].weight, m["3"].bias, sp.conv.weight, sp.bn.weight, sp.bn.bias)

    def forward(self, x):
        if not x.is_cuda:
            raise BratsHipError("brats21_amd.networks.CBAM runs on the GPU only (no CPU fallback)")
        if x.dim() != 5 or x.shape[1] != self.gate_channels:
            raise ValueError(f"expected input [N, {self.gate_channels}, D, H, W]")
        if self.storage not in (torch.float32, torch.bfloat16):
            raise NotImplementedError(f"CBAM: storage {self.storage} (torch.float32 or torch.bfloat16; fp16 storage is not built)")
        params = self._params()
        # the inference variant (no_grad, or nothing to differentiate) keeps nothing and does not write the channel-index plane
        save = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))
        return _CbamFn.apply(x.float(), self.storage, save, *params)

    def extra_repr(self):
        return f"gate_channels={self.gate_channels}, reduction_ratio={self.reduction_ratio}, norm_layer='instance'"
