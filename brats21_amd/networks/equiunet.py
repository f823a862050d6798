"""EquiUnet (GroupNorm + ReLU 3D U-Net) on the HIP kernels of libbrats_hip.so.

Drop-in for ``networks.equiunet2020.EquiUnet`` of the reference (networks/equiunet2020.py:407-500):
same constructor signature, same ``state_dict`` keys / shapes, same
``forward(x) -> (logits, [deep heads])`` contract on NCDHW float32 input, trainable through
``loss.backward()``.  Internally the whole network is ONE autograd node whose forward / backward are
explicit programs over NDHWC activations: torch.cat is replaced by producers writing into channel
slices of shared buffers, GroupNorm statistics come out of the convolution epilogue, and the skip /
pool gradient sum is fused into the pooling backward.

Precision follows the reference's switch (learning/engine.py:304 ``autocast(enabled=not no_amp)``):
under autocast the bf16-storage / f32-accumulate kernels run, otherwise the exact-f32 MFMA kernels
(the 1e-3 logit parity mode).  ``model.precision = "bf16" | "fp32"`` overrides it.
"""
import contextlib
import functools
import math
import os

import torch
import torch.nn as nn

from .. import ops
from .._lib import PACK_DGRAD, PACK_FWD, BratsHipError
from ._program import _PackedWeightsModule, _heads_bwd, _inherit_amax, input_cpad


# ------------------------------------------------------------------------------------------ parameter holders
class _ConvParams(nn.Module):
    """Parameter holder with nn.Conv3d's names, shapes and default init (weight [Co,Ci,k,k,k])."""

    def __init__(self, cin, cout, k, bias):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(cout, cin, k, k, k))
        self.bias = nn.Parameter(torch.empty(cout)) if bias else None
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if bias:
            bound = 1.0 / math.sqrt(cin * k * k * k)
            nn.init.uniform_(self.bias, -bound, bound)


class _NormParams(nn.Module):
    """weight / bias of the unit's norm layer; with ``batch`` also nn.BatchNorm3d's buffers (same state-dict names)."""

    def __init__(self, c, batch=False):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(c))
        self.bias = nn.Parameter(torch.zeros(c))
        if batch:
            self.register_buffer("running_mean", torch.zeros(c))
            self.register_buffer("running_var", torch.ones(c))
            self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))


class _EstBNParams(nn.Module):
    """EstBN's parameters and buffers under its state-dict names (networks/factory.py:150-160)."""

    def __init__(self, c):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(c))
        self.bias = nn.Parameter(torch.zeros(c))
        self.register_buffer("running_mean", torch.zeros(c))
        self.register_buffer("running_var", torch.ones(c))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))
        self.register_buffer("estbn_moving_speed", torch.zeros(1))


class _BCNormParams(nn.Module):
    """``--norm bcn`` = BCNorm(C, 8, estimate=True) (networks/factory.py:125-147,189-190): per-GROUP weight / bias [1, 8, 1]
    around a per-(sample, group) normalisation of EstBN's output.  How it runs here (no new kernel): EstBN is a per-channel
    affine map with constants -- u = a_c * y + b_c, a_c = weight_c / sqrt(running_var_c + 1e-5), b_c = bias_c - running_mean_c *
    a_c -- because nothing in the reference ever sets ``estbn_moving_speed`` away from 0, so its running buffers never move.  A
    per-output-channel affine map behind a convolution IS a convolution: the unit packs a_c * W_c and passes b_c as the
    bias, the implicit-GEMM kernel writes u directly, and what is left of BCNorm is GroupNorm(8) whose per-channel gamma /
    beta are the group's weight / bias -- the existing statistics, apply and backward kernels.  The chain rule back to W, EstBN's
    weight / bias and the group parameters is [C]- and weight-sized torch algebra (_bcn_param_grads)."""

    def __init__(self, c, groups=8):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(1, groups, 1))
        self.bias = nn.Parameter(torch.zeros(1, groups, 1))
        self.bn = _EstBNParams(c)
        self.num_groups = groups
        self._speed_checked = False

    def _load_from_state_dict(self, *args, **kwargs):
        self._speed_checked = False
        return super()._load_from_state_dict(*args, **kwargs)

    def tables(self):
        """(a_c, b_c, gamma_c, beta_c): EstBN as a per-channel affine map; the group weight / bias expanded per channel."""
        if not self._speed_checked:  # (the reference reads it with .item() in EVERY forward; once per load is enough here)
            if float(self.bn.estbn_moving_speed.reshape(-1)[0]) != 0.0:
                raise NotImplementedError("--norm bcn: EstBN with estbn_moving_speed != 0 is not implemented (the reference "
                                          "never sets it: networks/factory.py:160 is its only mention)")
            self._speed_checked = True
        c = self.bn.weight.numel()
        a = self.bn.weight.detach() * torch.rsqrt(self.bn.running_var + 1e-5)
        b = self.bn.bias.detach() - self.bn.running_mean * a
        cpg = c // self.num_groups
        gamma = self.weight.detach().reshape(-1).repeat_interleave(cpg)
        beta = self.bias.detach().reshape(-1).repeat_interleave(cpg)
        return a.float().contiguous(), b.float().contiguous(), gamma.float().contiguous(), beta.float().contiguous()


def _bcn_param_grads(unit, dw_eff, db_eff, dgamma_c, dbeta_c):
    """Chain rule of the BCNorm unit (see _BCNormParams): W' = a_c W, bias' = b_c, gamma_c = group weight, beta_c = group bias.
    Returns {parameter: gradient} for conv.weight, bn.weight, bn.bias, bn.bn.weight, bn.bn.bias."""
    bcn = unit.bn
    a, _, _, _ = bcn.tables()
    w = unit.conv.weight.detach()
    k = torch.rsqrt(bcn.bn.running_var + 1e-5)
    da = (dw_eff * w).sum((1, 2, 3, 4))
    g = bcn.num_groups
    return {unit.conv.weight: dw_eff * a.view(-1, 1, 1, 1, 1),
            bcn.weight: dgamma_c.view(g, -1).sum(1).view(1, g, 1),
            bcn.bias: dbeta_c.view(g, -1).sum(1).view(1, g, 1),
            bcn.bn.weight: k * (da - bcn.bn.running_mean * db_eff),
            bcn.bn.bias: db_eff}


class ConvBnRelu(nn.Module):
    """conv3x3x3 (no bias) -> norm -> act -> Dropout(p)   (networks/equiunet2020.py:51-75).  The norm is GroupNorm(8)
    (``--norm group``) or InstanceNorm3d(affine=True) (``--norm instance``, the CLI default; networks/factory.py:
    179-188): the same kernels with 8 or ``planes`` statistics groups.  ``--norm batch`` (nn.BatchNorm3d(affine=True),
    round 4) is the same kernels again: NDHWC is contiguous, so the batch [N, D, H, W, C] viewed as ONE sample
    [1, N*D, H, W, C] with ``planes`` groups gives exactly the batch statistics (biased variance) in training mode, forward
    and backward; the running buffers are updated from the finalised mean / rstd, and eval mode builds the per-channel
    scale / shift from them (_bn_forward_tables).  ``--act prelu``: MONAI's Act["prelu"] = nn.PReLU()
    -- one learnable slope per unit, state-dict key ``<unit>.prelu.weight`` like the reference's nn.Sequential entry."""

    def __init__(self, inplanes, planes, dilation=1, norm="group", act="relu"):
        super().__init__()
        self.conv = _ConvParams(inplanes, planes, 3, bias=False)
        self.batch_norm = norm == "batch"
        self.bcn = norm == "bcn"
        self.bn = _BCNormParams(planes, 8) if self.bcn else _NormParams(planes, batch=self.batch_norm)
        if act == "prelu":
            self.prelu = nn.PReLU()
        self.dilation = dilation
        self.groups = 8 if norm in ("group", "bcn") else planes


class UBlock(nn.Module):
    """networks/equiunet2020.py:105-123"""

    def __init__(self, inplanes, midplanes, outplanes, dilation=(1, 1), norm="group", act="relu"):
        super().__init__()
        self.ConvBnRelu1 = ConvBnRelu(inplanes, midplanes, dilation[0], norm, act)
        self.ConvBnRelu2 = ConvBnRelu(midplanes, outplanes, dilation[1], norm, act)


class RefUnet(nn.Module):
    """The refinement stage of ``--model equiunet_ref`` (networks/equiunet2020.py:252-310): a five-level U-Net of ConvBnRelu units
    at one width between a num_classes -> width convolution (bias, no norm) and a width -> num_classes convolution (bias) whose
    output is added onto the logits.  Parameter container only -- the programs are _ref_fwd / _ref_bwd below."""

    def __init__(self, in_ch, inc_ch, norm="group", act="relu"):
        super().__init__()
        self.conv0 = _ConvParams(in_ch, inc_ch, 3, bias=True)
        for name in ("hx1", "hx2", "hx3", "hx4", "hx5"):
            setattr(self, name, ConvBnRelu(inc_ch, inc_ch, 1, norm, act))
        for name in ("d4", "d3", "d2", "d1"):
            setattr(self, name, ConvBnRelu(inc_ch * 2, inc_ch, 1, norm, act))
        self.conv_d0 = _ConvParams(inc_ch, in_ch, 3, bias=True)


def _head(cin, k):
    return nn.ModuleList([_ConvParams(cin, k, 1, bias=True)])  # key "<name>.0.weight" like nn.Sequential


# ------------------------------------------------------------------------------------------ programs
def _f8_ok(fp8, dtype, x, x2=None):
    return (bool(fp8) and ops.is16(dtype) and not getattr(x, "_net_input", False) and x.shape[1] >= ops.F8_MIN_SIZE and
            ops.conv_f8_chunk(x.shape[-1], x2.shape[-1] if x2 is not None else 0) > 0)


def _unit_act(unit, act):
    """(kernel activation, device slope | None): PReLU = leakyrelu whose slope is the unit's learnable scalar."""
    if act == "prelu":
        return "leakyrelu", unit.prelu.weight.detach()
    return act, None


def _one_sample(t):
    """[N, D, H, W, C] (dense) as one sample [1, N*D, H, W, C]: what turns per-sample statistics into batch statistics."""
    n, d, h, w, c = t.shape
    if not t.is_contiguous():
        raise BratsHipError("--norm batch needs dense activations")
    return t.view(1, n * d, h, w, c)


def _blk(b):
    """(first, second) unit of a UBlock."""
    return b.ConvBnRelu1, b.ConvBnRelu2


def _bn_fwd_tail(cx, unit, x, x2, y, stats, pool):
    """BatchNorm3d + activation behind the convolution (see ConvBnRelu)."""
    n, d, h, wd, c = y.shape
    bn = unit.bn
    if cx.training:
        mean_rstd, scale_shift = ops.gn_finalize(stats.view(1, -1, c, 2), 1, c, c, n * d * h * wd, bn.weight.detach(), bn.bias.detach())
        with torch.no_grad():  # running buffers: momentum 0.1, UNBIASED variance (torch.nn.functional.batch_norm)
            cnt = float(n * d * h * wd)
            mean = mean_rstd[0, :, 0]
            var = (1.0 / mean_rstd[0, :, 1].double() ** 2 - 1e-5).clamp_min(0).float()
            bn.running_mean.mul_(0.9).add_(mean, alpha=0.1)
            bn.running_var.mul_(0.9).add_(var, alpha=0.1 * cnt / max(cnt - 1.0, 1.0))
            bn.num_batches_tracked += 1
    else:
        mean_rstd = None
        scale = bn.weight.detach() * torch.rsqrt(bn.running_var + 1e-5)
        scale_shift = torch.stack([scale, bn.bias.detach() - bn.running_mean * scale], -1).reshape(1, c, 2).contiguous().float()
    kact, slope_t = _unit_act(unit, cx.act)
    z = ops.affine_act(_one_sample(y), scale_shift, kact, slope_t=slope_t).view(n, d, h, wd, c)
    cx.dropped(z, cx.drop_of(unit), out=z)
    cx.recs[unit] = (unit, x, x2, y, mean_rstd, scale_shift)
    if pool:
        return z, ops.maxpool2(z, want_argmax=pool == "argmax")
    return z


def _cgr_fwd(cx, unit, x, x2=None, *, no_act=False, pool=False, lazy=False):
    """One ConvBnRelu: pack -> implicit-GEMM conv over the virtual concat [x | x2] (+ tile statistics)
    -> finalize -> normalise+act; what the backward needs goes to cx.recs[unit].  cx.fp8: the convolution runs on the e4m3
    kernel (scales from the |max| the producer of x recorded); the normalise+act pass records the |max| of its own output for
    the next layer.
    no_act: return the raw convolution output (the last layer under the fused output head, ops.gn_head: the activation is
    applied on load there).  pool: the layer ends an encoder level -> (z, max-pooled z).  lazy: z has one reader, the next
    convolution -> an ops.Pending where cx.lazy_ok."""
    dtype, fp8 = cx.dtype, cx.fp8
    # nn.Dropout(p) behind the activation (networks/equiunet2020.py:62; training mode only).  The activation is then always
    # materialised (no fused pooling / head / on-load forms) and dropped in place (ops.dropout).
    uid = cx.drop_of(unit)
    lazy = lazy and cx.lazy_ok and uid is None
    if pool:  # (training: the pooling pass also records the arg-max bytes its backward reads)
        pool = "argmax" if cx.will_bwd else True
    w = unit.conv.weight
    cbias, gamma_c, beta_c = None, unit.bn.weight.detach(), unit.bn.bias.detach()
    if unit.bcn:
        # BCNorm (see _BCNormParams): EstBN's per-channel affine map rides in the convolution (weights a_c * W, bias b_c), the
        # rest is GroupNorm(8) with the group's weight / bias as per-channel gamma / beta
        if torch.is_grad_enabled():
            a_c, cbias, gamma_c, beta_c = unit.bn.tables()
            w = w.detach() * a_c.view(-1, 1, 1, 1, 1)
        else:
            # inference (~144 forwards of the same weights per volume): fold ONCE per unit -- the folded tensor stays the same
            # object, so ops.pack_weights' cache hits and no dead entry piles up in it.  Valid while none of the
            # tensors it was made from changed: version counters, addresses and the pack generation (writes through p.data)
            srcs = (unit.conv.weight, unit.bn.weight, unit.bn.bias, unit.bn.bn.weight, unit.bn.bn.bias, unit.bn.bn.running_var,
                    unit.bn.bn.running_mean)
            key = (ops.pack_generation(),) + tuple((t._version, t.data_ptr()) for t in srcs)
            hit = getattr(unit, "_bcn_fold", None)
            if hit is None or hit[0] != key:
                a_c, cbias, gamma_c, beta_c = unit.bn.tables()
                hit = unit._bcn_fold = (key, (w.detach() * a_c.view(-1, 1, 1, 1, 1), cbias, gamma_c, beta_c))
            w, cbias, gamma_c, beta_c = hit[1]
        fp8, lazy = None, False
    elif unit.conv.bias is not None:
        # a learnable convolution bias (the units of networks/unet_family.py): it rides in the convolution like bcn's folded
        # shift; the e4m3 form is not built with one, so such a unit takes the 16-bit convolution
        cbias, fp8 = unit.conv.bias.detach(), None
    cout = w.shape[0]
    cin_pad = x.shape[-1] + (x2.shape[-1] if x2 is not None else 0)
    c1 = x.shape[-1] if x2 is not None else None
    if isinstance(x, ops.Pending) or isinstance(x2, ops.Pending):
        # inference: an input whose normalised activation was never stored -- applied on load where that form of the
        # convolution is built for this layer, materialised (the affine_act pass) otherwise
        if fp8 or not ops.conv_pre_ok(dtype, 3, unit.dilation, x.shape[-1], x2.shape[-1] if x2 is not None else 0, cout):
            x = x.materialize() if isinstance(x, ops.Pending) else x
            x2 = x2.materialize() if isinstance(x2, ops.Pending) else x2
    if _f8_ok(fp8, dtype, x, x2):
        wpk = ops.pack_weights_f8(w, PACK_FWD, cin_pad=cin_pad, c1=c1)
        y, stats = ops.conv3d_f8(x, wpk, cout, unit.dilation, want_stats=True, x2=x2, amax=getattr(x, "_amax", None),
                                 amax2=getattr(x2, "_amax", None) if x2 is not None else None)
    else:
        with ops.use_plan(None) if unit.bcn else contextlib.nullcontext():  # (a_c * W is a new tensor every step: not a plan entry)
            wpk = ops.pack_weights(w, dtype, PACK_FWD, cin_pad=cin_pad, dil=unit.dilation, c1=c1)
        # (_x3amax: the network input in split-precision mode -- the only conv input no normalisation has bounded; see _fn_forward)
        y, stats = ops.conv3d(x, wpk, cout, 3, unit.dilation, want_stats=True, x2=x2, amax=getattr(x, "_x3amax", None), bias=cbias)
    n, d, h, wd, _ = y.shape
    if unit.batch_norm:
        return _bn_fwd_tail(cx, unit, x, x2, y, stats, pool)
    mean_rstd, scale_shift = ops.gn_finalize(stats, n, cout, unit.groups, d * h * wd, gamma_c, beta_c)
    rec = (unit, x, x2, y, mean_rstd, scale_shift)
    if no_act:
        cx.recs[unit] = rec
        return y
    amax = cx.slot(y.device)
    kact, slope_t = _unit_act(unit, cx.act)
    if lazy and slope_t is None and kact in ("relu", "leakyrelu") and amax is None and not pool:
        return ops.Pending(y, scale_shift, kact)  # (no_grad only: nothing is taped)
    cx.recs[unit] = rec
    if pool and uid is None and kact in ("relu", "leakyrelu") and y.numel() * y.element_size() >= (256 << 20):
        # normalise + act and the 2x2x2 max pool of the result in one pass -- for tensors
        # beyond the Infinity Cache (the 128^3 level: 188 us against 148 + 85); smaller ones are re-read from the cache by
        # the pooling kernel at no HBM cost and the two plain kernels are as fast (measured: 70 against 63 us)
        z, pooled = ops.affine_act_pool(y, scale_shift, kact, amax=amax, slope_t=slope_t, want_argmax=pool == "argmax")
        if amax is not None:
            z._amax = pooled._amax = amax  # (max|pool(z)| <= max|z|: the pooled tensor inherits the scale source)
        return z, pooled
    z = ops.affine_act(y, scale_shift, kact, amax=amax, slope_t=slope_t)
    if amax is not None:
        z._amax = amax
    cx.dropped(z, uid, out=z)
    if pool:
        return z, _inherit_amax(ops.maxpool2(z, want_argmax=pool == "argmax"), z)
    return z


def _cgr_bwd(cx, unit, dz, *, need_dx=True, head=None, pool=None, bst=None):
    """Backward of one ConvBnRelu; the parameter gradients go to cx.put.  Returns dx, or (dx1, dx2) -- two dense tensors from
    one dgrad launch -- for a two-source unit.
    head = (head module, dlogits) instead of dz: the last layer, whose output feeds only the 1x1x1 head.
    pool = (d_skip, d_pooled, arg-max bytes) instead of dz: the layer ends an encoder level.
    bst: the unit that PRODUCED this unit's input (the first unit of the block).  Where the kernel form is built
    (model.fold_bwd_stats), the input-gradient launch also takes the first pass of that unit's GroupNorm backward
    (ops.conv3d_bstats) and dx is returned as (dx, tile_stats); handed on as `dz`, such a pair makes this function finish from
    the tile sums (ops.gn_act_bwd_tiles) instead of reading dz and y twice.
    cx.fp8 == "all": the input gradient (dgrad) and -- for the dilation-1 layers the all-taps kernel covers -- the weight
    gradient run on the e4m3 kernels too, scaled by the |max| of dy that the GroupNorm backward records (and the |max| of
    the layer input recorded in the forward pass)."""
    _, x, x2, y, mean_rstd, scale_shift = cx.recs[unit]
    dtype, fp8 = cx.dtype, cx.fp8
    if bst is not None:  # dropout: the folds that never materialise a unit's output gradient are off
        bst = cx.recs[bst] if (cx.m.fold_bwd_stats and cx.drop is None) else None
    cin = unit.conv.weight.shape[1]
    gamma_c = unit.bn.weight.detach()
    w_bwd = unit.conv.weight
    if unit.bcn:
        a_c, _, gamma_c, _ = unit.bn.tables()
        w_bwd = unit.conv.weight.detach() * a_c.view(-1, 1, 1, 1, 1)  # the weights the forward convolved with
        fp8 = None
    elif unit.conv.bias is not None:
        fp8 = None
    tiles = None
    if isinstance(dz, tuple):
        dz, tiles = dz
    dz = cx.dropped(dz, cx.drop_of(unit))  # the forward's mask, regenerated: d(dropout(z)) / dz = the same multiplier
    all8 = fp8 == "all" and ops.is16(dtype)
    f8 = all8 and need_dx and ops.conv_f8_chunk(y.shape[-1]) > 0
    # e4m3 weight gradient: where the all-taps kernel is built for the layer and the producers of x (x2) recorded |max|
    ax, ax2 = getattr(x, "_amax", None), (getattr(x2, "_amax", None) if x2 is not None else None)
    w8 = (all8 and unit.dilation == 1 and ax is not None and (x2 is None or ax2 is not None) and ops.is16(y.dtype)
          and ops.conv3d_wgrad_f8_ok(x, y, x2))
    # split precision on fp16 pairs: dy (values of 1e-6 and below) is scaled by a power of two taken from its recorded |max|
    x3s = cx.x3s
    amax = cx.slot(y.device, True) if (f8 or w8 or x3s) else None
    kact, slope_t = _unit_act(unit, cx.act)
    if slope_t is not None:
        cx.put(unit.prelu.weight, ops.prelu_slope_grad(dz, y, scale_shift))
    if unit.batch_norm:
        if mean_rstd is None:
            raise NotImplementedError("--norm batch: backward through an eval-mode forward (running statistics) is not implemented")
        n_, d_, h_, w_, c_ = y.shape
        dy, dgamma, dbeta = ops.gn_act_bwd(_one_sample(dz), _one_sample(y), scale_shift, mean_rstd, gamma_c, c_, kact,
                                           amax=amax, slope_t=slope_t)
        dy = dy.view(n_, d_, h_, w_, c_)
        if amax is not None:
            dy._amax = amax
    elif head is not None:
        # the head's backward is folded into the GroupNorm backward -- d(up1) is never written, the head's weight / bias
        # gradients come out of the same passes (ops.gn_act_bwd_head)
        hd, dout = head
        dy, dgamma, dbeta, dhw, dhb = ops.gn_act_bwd_head(dout, hd.weight, y, scale_shift, mean_rstd, gamma_c,
                                                          unit.groups, kact, amax=amax)
        cx.put(hd.weight, dhw)
        cx.put(hd.bias, dhb)
    elif pool is not None:
        # dz = skip gradient + max-pool backward, composed inside the GroupNorm backward -- the pooling backward's output
        # tensor is never written (ops.gn_act_bwd_pool)
        dy, dgamma, dbeta = ops.gn_act_bwd_pool(pool[0], pool[1], pool[2], y, scale_shift, mean_rstd, gamma_c,
                                                unit.groups, kact, amax=amax)
    elif tiles is not None:
        dy, dgamma, dbeta = ops.gn_act_bwd_tiles(tiles, dz, y, scale_shift, mean_rstd, gamma_c, unit.groups, kact,
                                                 amax=amax)
    else:
        dy, dgamma, dbeta = ops.gn_act_bwd(dz, y, scale_shift, mean_rstd, gamma_c, unit.groups, kact, amax=amax,
                                           slope_t=slope_t)
    wdst = cx.dest(unit.conv.weight)  # data-parallel: the weight gradient is written straight into its slice of the bucket
    if w8 and amax is not None:
        dw = ops.conv3d_wgrad_f8(x, dy, ax, amax, x2=x2, amax2=ax2, out=wdst)
    elif x2 is not None and x.shape[-1] % 16:  # narrow test widths only: the wgrad ci tile (16) would straddle x | x2
        dw, db = ops.conv3d_wgrad(torch.cat([x, x2], -1), dy, 3, unit.dilation, amax_dy=amax if x3s else None, want_dbias=unit.bcn)
    else:
        dw, db = ops.conv3d_wgrad(x, dy, 3, unit.dilation, x2=x2, out=None if unit.bcn else wdst, amax_dy=amax if x3s else None,
                                  want_dbias=unit.bcn)
    dw = dw[:, :cin].contiguous() if dw.shape[1] != cin else dw
    if unit.bcn:
        pg = _bcn_param_grads(unit, dw, db, dgamma, dbeta)  # dw / db are the gradients of a_c * W and b_c
    else:
        pg = {unit.conv.weight: dw, unit.bn.weight: dgamma, unit.bn.bias: dbeta}
        if unit.conv.bias is not None:
            # the channel sum of dy: ops.channel_dot streams the tensor once (the weight-gradient entry's own dbias pass is one
            # workgroup per channel, see _ref_bwd)
            pg[unit.conv.bias] = ops.channel_dot(dy).sum(0)
    for prm, g in pg.items():
        cx.put(prm, g)
    if not need_dx:
        return None
    if f8:
        wpk = ops.pack_weights_f8(unit.conv.weight, PACK_DGRAD)

        def dgrad(**kw):
            return ops.conv3d_f8(dy, wpk, cin, unit.dilation, amax=amax, **kw)
    else:
        with ops.use_plan(None) if unit.bcn else contextlib.nullcontext():
            wpk = ops.pack_weights(w_bwd, dtype, PACK_DGRAD, dil=unit.dilation)

        def dgrad(**kw):
            return ops.conv3d(dy, wpk, cin, 3, unit.dilation, amax=amax if x3s else None, **kw)
    if x2 is None:
        if bst is not None and not f8:
            u1, _, _, y1, mr1, ss1 = bst
            kact1, slope1 = _unit_act(u1, cx.act)
            if (not u1.batch_norm and not u1.bcn and not unit.bcn and mr1 is not None and y1.shape[-1] == cin and y1.dtype == dy.dtype
                    and ops.conv_bstats_ok(dtype, unit.dilation, dy.shape[-1], cin, kact1, slope1)):
                # (dx, tile sums of u1's GroupNorm backward)
                return ops.conv3d_bstats(dy, wpk, cin, unit.dilation, y1, ss1, kact1, amax=amax if x3s else None)
        dx, _ = dgrad()
        return dx
    c1 = x.shape[-1]
    if c1 % ops.split_granule(cin) == 0:
        dx, _ = dgrad(split=c1)  # (dx1, dx2): two dense tensors, one launch
        return dx
    dx, _ = dgrad()  # narrow test widths: slice views of one tensor
    return dx[..., :c1], dx[..., c1:]


def _level_bwd(cx, unit, down, d_pooled, d_skip, need_dx=True, bst=None):
    """Backward of the last layer of an encoder level: its output gradient = d_skip + max-pool backward(d_pooled)."""
    idx = getattr(down, "_pool_argmax", None)
    kact, slope_t = _unit_act(unit, cx.act)
    if (idx is not None and cx.m.fold_pool_bwd and cx.drop is None and not unit.batch_norm and slope_t is None
            and kact in ("relu", "leakyrelu")):
        return _cgr_bwd(cx, unit, None, need_dx=need_dx, pool=(d_skip, d_pooled, idx), bst=bst)
    return _cgr_bwd(cx, unit, ops.maxpool2_bwd(down, d_pooled, dx_skip=d_skip), need_dx=need_dx, bst=bst)


# ------------------------------------------------------------------------------------------ refinement stage (RefUnet)
def _ref_cpad(k):
    """Channels of the zero-padded NDHWC form of a [N, k, D, H, W] gradient that the weight-gradient / dgrad kernels take as dy."""
    return 8 if k <= 8 else 16


def _ref_amax(cx, t):
    """max|t| for the fp16-pair split of a gradient no producer kernel recorded it for (see _cgr_bwd's amax); None elsewhere."""
    return ops.absmax(t) if cx.x3s else None


def _ref_fwd(ctx, cx, out):
    """RefUnet.forward on the unrefined logits `out` [N, K, D, H, W] f32 -> refined logits, same shape (networks/equiunet2020.py:
    277-309).  The nine units are _cgr_fwd -- the up-sampled tensor comes FIRST in the concat, the skip second (:296-305, the
    opposite of the main decoder) -- conv0 is the first layer's route (class planes zero-padded to a channel vector), and the last
    convolution, the bias and the residual are one pass of ops.conv3d_narrow."""
    r, dtype = cx.m.refunet, cx.dtype
    cgr = functools.partial(_cgr_fwd, cx)
    k, f0 = out.shape[1], r.conv0.weight.shape[0]
    x0 = ops.ncdhw_to_ndhwc(out, dtype, cpad=input_cpad(k, dtype))
    x0._net_input = True
    amax0 = ops.absmax(x0) if ops.x3_mode() == ops.X3F else None  # (un-normalised, like the network input: _fn_forward)
    wpk = ops.pack_weights(r.conv0.weight, dtype, PACK_FWD, cin_pad=x0.shape[-1])
    hx, _ = ops.conv3d(x0, wpk, f0, 3, 1, bias=r.conv0.bias.detach(), amax=amax0)
    hx1, p = cgr(r.hx1, hx, pool=True)
    hx2, p = cgr(r.hx2, p, pool=True)
    hx3, p = cgr(r.hx3, p, pool=True)
    hx4, p = cgr(r.hx4, p, pool=True)
    d = cgr(r.hx5, p)
    for unit, skip in ((r.d4, hx4), (r.d3, hx3), (r.d2, hx2), (r.d1, hx1)):
        d = cgr(unit, ops.upsample(d, 2), x2=skip)
    ctx.ref = (x0, hx1, hx2, hx3, hx4, d)
    return ops.conv3d_narrow(d, ops.pack_weights_narrow(r.conv_d0.weight, PACK_FWD), k, bias=r.conv_d0.bias.detach(), add=out)


def _ref_bwd(ctx, cx, d_ref, d_out):
    """Backward of _ref_fwd: the stage's parameter gradients go to cx.put; returns the whole gradient of the unrefined logits,
    d_ref (through the residual) + d_out (the loss on the unrefined head) + conv0^T d(hx) -- the last two terms and the
    transposed convolution are one pass of ops.conv3d_narrow."""
    r, dtype = cx.m.refunet, cx.dtype
    cbw = functools.partial(_cgr_bwd, cx)
    x0, hx1, hx2, hx3, hx4, d1 = ctx.ref
    ctx.ref = None
    if d_ref is None:
        d_ref = torch.zeros(ctx.out_shape, dtype=torch.float32, device=d1.device)
    d_ref = d_ref.contiguous().float()
    k, f0 = d_ref.shape[1], d1.shape[-1]
    # conv_d0: dy = d_ref as NDHWC, class planes zero-padded to a channel vector (the weight rows are padded alike)
    dy = ops.ncdhw_to_ndhwc(d_ref, dtype, cpad=_ref_cpad(k))
    amax = _ref_amax(cx, dy)
    dw, _ = ops.conv3d_wgrad(d1, dy, 3, 1, amax_dy=amax)
    cx.put(r.conv_d0.weight, dw[:k].contiguous())
    # (the bias gradients are channel sums: ops.channel_dot streams the tensor once; the weight-gradient entry's own dbias pass is
    #  one workgroup per channel -- 6.8 ms at 2 x 128^3, measured)
    cx.put(r.conv_d0.bias, ops.channel_dot(dy).sum(0)[:k].contiguous())
    wpad = torch.zeros((dy.shape[-1],) + tuple(r.conv_d0.weight.shape[1:]), dtype=torch.float32, device=d1.device)
    wpad[:k] = r.conv_d0.weight.detach()
    with ops.use_plan(None):  # (a new tensor every step: not a plan entry)
        wpk = ops.pack_weights(wpad, dtype, PACK_DGRAD)
    g, _ = ops.conv3d(dy, wpk, f0, 3, 1, amax=amax)
    # d1 .. d4 (inputs [up-sampled | skip]), hx5, then the pooled levels
    skips = []
    for unit in (r.d1, r.d2, r.d3, r.d4):
        g_up, g_skip = cbw(unit, g)
        skips.append(g_skip)
        g = ops.upsample_bwd(g_up, 2)
    g = cbw(r.hx5, g)
    for unit, down in ((r.hx4, hx4), (r.hx3, hx3), (r.hx2, hx2), (r.hx1, hx1)):
        g = _level_bwd(cx, unit, down, g, skips.pop())
    # conv0: weight / bias gradients on the padded logits, input gradient + the two other terms of d(out)
    dw0, _ = ops.conv3d_wgrad(x0, g, 3, 1, amax_dy=_ref_amax(cx, g))
    cx.put(r.conv0.weight, dw0[:, :k].contiguous())
    cx.put(r.conv0.bias, ops.channel_dot(g).sum(0))
    rest = d_ref if d_out is None else d_ref + d_out.float()
    return ops.conv3d_narrow(g, ops.pack_weights_narrow(r.conv0.weight, PACK_DGRAD), k, add=rest)


def _deep_heads_on(m):
    return m.deep_supervision and not (m.skip_deep_heads_in_eval and not m.training)


def _plus(a, b):
    return a if b is None else a + b


def _top_head_fwd(ctx, cx, last, u1, head):
    """The last unit of the decoder on its input u1, and the output head on it -> (logits, the unit's stored activation or None);
    sets ctx.top_fused / ctx.out_shape / ctx.heads = [the output head's entry] for _top_head_bwd."""
    m = cx.m
    # the last layer's activation up1 feeds only the output head: where the kernels for it are built, the head reads
    # the raw convolution output and applies GroupNorm + act on load (ops.gn_head), the backward recomputes what it
    # needs (ops.gn_act_bwd_head) -- up1 (2 x 403 MB written + read at 2 x 48 x 128^3) is never stored
    kact, slope_t = _unit_act(last, cx.act)
    nk = head.weight.shape[0]
    fuse_top = (m.fold_head_fwd and cx.drop is None and not last.batch_norm and slope_t is None and kact in ("relu", "leakyrelu")
                and nk <= 4 and (not cx.will_bwd or (m.fold_head_bwd and ops.head_fold_ok(head.weight, kact, slope_t))))
    if fuse_top:
        y1 = _cgr_fwd(cx, last, u1, no_act=True)
        up1 = None
        logits = ops.gn_head(y1, cx.recs[last][5], head.weight, head.bias, kact)
    else:
        up1 = _cgr_fwd(cx, last, u1)
        logits = ops.head(up1, head.weight, head.bias, 1)
    ctx.top_fused = fuse_top
    ctx.out_shape = tuple(logits.shape)
    ctx.heads = [(head, up1, 1)]
    return logits, up1


def _top_head_bwd(ctx, cx, c1, c2, head, douts):
    """Backward of all heads (ctx.heads, _heads_bwd) and of the decoder's last block (c1, c2) under the output head
    (_top_head_fwd) -> (what the backward of c1 returns, dsrc)."""
    m = cx.m
    # the output head on up1: folded into the GroupNorm backward of the last layer where that is built
    top, dsrc = _heads_bwd(ctx, cx, douts, m.fold_head_bwd and cx.drop is None and not c2.batch_norm
                           and ops.head_fold_ok(head.weight, *_unit_act(c2, cx.act)))
    if top is not None:
        d_c1 = _cgr_bwd(cx, c2, None, head=top, bst=c1)
    else:
        up1 = ctx.heads[0][1]
        d_up1 = dsrc.get(up1.data_ptr())
        d_c1 = _cgr_bwd(cx, c2, d_up1 if d_up1 is not None else torch.zeros_like(up1), bst=c1)
    return _cgr_bwd(cx, c1, d_c1), dsrc


def _decoder_fwd(ctx, cx, down1, down2, down3, down4, bottom, bottom_2):
    """The decoder and the heads behind bottom_2 (networks/equiunet2020.py:481-498; AttEquiUnet's program hands in its gated
    tensors) -> [logits, deep heads...]; ctx.bufs / ctx.heads / ctx.top_fused are what _decoder_bwd reads."""
    m = cx.m
    cgr = functools.partial(_cgr_fwd, cx)

    def up(t):
        return _inherit_amax(ops.upsample(t, 2), t)

    up3 = cgr(m.decoder3.ConvBnRelu2, cgr(m.decoder3.ConvBnRelu1, down3, x2=up(bottom_2), lazy=True))
    up2 = cgr(m.decoder2.ConvBnRelu2, cgr(m.decoder2.ConvBnRelu1, down2, x2=up(up3), lazy=True))
    u1 = cgr(m.decoder1.ConvBnRelu1, down1, x2=up(up2), lazy=True)
    logits, up1 = _top_head_fwd(ctx, cx, m.decoder1.ConvBnRelu2, u1, m.outconv)
    outs = [logits]
    if _deep_heads_on(m):
        for hd, src, sc in ((m.deep_bottom[0], bottom, 8), (m.deep_bottom2[0], bottom_2, 8), (m.deep3[0], up3, 4),
                            (m.deep2[0], up2, 2)):
            outs.append(ops.head(src, hd.weight, hd.bias, sc))
            ctx.heads.append((hd, src, sc))
    ctx.bufs = (down1, down2, down3, down4, bottom, bottom_2, up3, up2, up1)
    return outs


def _decoder_bwd(ctx, cx, douts):
    """Backward of _decoder_fwd -> (d_skip1, d_skip2, d_skip3, the whole gradient of bottom_2, the deep head's gradient of bottom or
    None)."""
    m = cx.m
    _, _, _, _, bottom, bottom_2, up3, up2, _ = ctx.bufs
    cbw = functools.partial(_cgr_bwd, cx)
    (d_skip1, d_u1), dsrc = _top_head_bwd(ctx, cx, *_blk(m.decoder1), m.outconv, douts)

    def extra(t):
        return dsrc.get(t.data_ptr())

    # (the deep head's gradient of the same activation is added inside the adjoint's launch: the sum of the two stored tensors)
    d_up2 = ops.upsample_bwd(d_u1, 2, add=extra(up2))
    c1, c2 = _blk(m.decoder2)
    d_skip2, d_u2 = cbw(c1, cbw(c2, d_up2, bst=c1))
    d_up3 = ops.upsample_bwd(d_u2, 2, add=extra(up3))
    c1, c2 = _blk(m.decoder3)
    d_skip3, d_u3 = cbw(c1, cbw(c2, d_up3, bst=c1))
    return d_skip1, d_skip2, d_skip3, ops.upsample_bwd(d_u3, 2, add=extra(bottom_2)), extra(bottom)


# ------------------------------------------------------------------------------------------ module
class EquiUnet(_PackedWeightsModule):
    """Constructor signature of networks/equiunet2020.py:413-414."""
    name = "EquiUnet"
    _cpu_hint = "; move input/model to cuda"

    def __init__(self, inplanes, num_classes, features, norm_layer=None, act="relu", deep_supervision=False, dropout=0,
                 refinement=False):
        super().__init__()
        if norm_layer not in ("group", "instance", "batch", "bcn"):
            raise NotImplementedError(f"brats21_amd.EquiUnet implements --norm group|instance|batch|bcn (got {norm_layer!r})")
        if norm_layer == "batch" and act == "prelu":
            raise NotImplementedError("--norm batch with --act prelu is not implemented")
        if act not in ("relu", "leakyrelu", "elu", "prelu", "swish", "mish"):
            raise NotImplementedError(f"brats21_amd.EquiUnet implements --act relu|leakyrelu|elu|prelu|swish|mish (got {act!r})")
        self._check_shape_limits(inplanes, num_classes, features, 8)
        print(f"EquiUnet features: {features}")
        self.deep_supervision = deep_supervision
        self.refinement = bool(refinement)
        self.act = act
        self.features = list(features)
        # nn.Dropout(p) behind every ConvBnRelu's activation (networks/equiunet2020.py:62; --dropout, src/arguments_train.py:52)
        self._init_dropout(dropout)
        self._init_switches(pack_plan="0")
        # pack_plan is off by default here: this network's step is GPU-bound; the single launch (0.11 ms) saves 0.1 ms over the
        # 33 per-layer ones (6.6 us each), and the convolutions lose 0.10-0.18 ms per step on weights that were packed long before
        # their layer runs and have left L2 (same-box A/B); EquiUnetASSPEvo (host-bound eager) gains 10 %.
        # inference (no_grad, 16-bit): the activation between the two convolutions of a block is applied on load by the second
        # one and never stored (ops.Pending / brats_conv3d_fwd_pre); BRATS_NORM_ON_LOAD=0: the two-pass path, for A/B runs
        self.norm_on_load = os.environ.get("BRATS_NORM_ON_LOAD", "1") != "0"
        f = self.features
        nl = norm_layer
        self.encoder1 = UBlock(inplanes, f[0], f[0], norm=nl, act=act)
        self.encoder2 = UBlock(f[0], f[1], f[1], norm=nl, act=act)
        self.encoder3 = UBlock(f[1], f[2], f[2], norm=nl, act=act)
        self.encoder4 = UBlock(f[2], f[3], f[3], norm=nl, act=act)
        self.bottom = UBlock(f[3], f[3], f[3], (2, 2), norm=nl, act=act)
        self.bottom_2 = ConvBnRelu(f[3] * 2, f[2], norm=nl, act=act)
        self.decoder3 = UBlock(f[2] * 2, f[2], f[1], norm=nl, act=act)
        self.decoder2 = UBlock(f[1] * 2, f[1], f[0], norm=nl, act=act)
        self.decoder1 = UBlock(f[0] * 2, f[0], f[0], norm=nl, act=act)
        self.outconv = _ConvParams(f[0], num_classes, 1, bias=True)
        if deep_supervision:
            self.deep_bottom = _head(f[3], num_classes)
            self.deep_bottom2 = _head(f[2], num_classes)
            self.deep3 = _head(f[1], num_classes)
            self.deep2 = _head(f[0], num_classes)
        if self.refinement:
            # registered LAST (networks/equiunet2020.py:460-462): its keys end the state dict, and the dropout streams of the
            # units above (_unit_ids) are the same with and without it
            self.refunet = RefUnet(num_classes, f[0], norm=nl, act=act)
        self._unit_ids = {u: i for i, u in enumerate(mod for mod in self.modules() if isinstance(mod, ConvBnRelu))}
        # init_weights(self, "kaiming"), networks/factory.py:203-224: kaiming-normal fan_out on conv weights
        print("initialize network with kaiming")
        for mod in self.modules():
            if isinstance(mod, _ConvParams):
                nn.init.kaiming_normal_(mod.weight.data, a=0.0, mode="fan_out")
            elif isinstance(mod, _NormParams) and norm_layer == "batch":  # factory.py:219-221: BatchNorm3d weights ~ N(1, 0.02)
                nn.init.normal_(mod.weight.data, 1.0, 0.02)
                nn.init.constant_(mod.bias.data, 0.0)

    def forward(self, x):
        return self._run(x)

    def _program_fwd(self, ctx, cx, x0):
        m = cx.m
        cgr = functools.partial(_cgr_fwd, cx)
        # encoder (networks/equiunet2020.py:469-475); every tensor is dense NDHWC, the decoder convolutions
        # read the virtual concat [skip | up-sampled] from two pointers (no torch.cat, no strided slices)
        # (the last layer of a level writes its activation -- the skip connection -- and the max-pooled tensor in one pass;
        #  lazy: the activation between the two units of a block has ONE reader, the block's second convolution)
        down1, p1 = cgr(m.encoder1.ConvBnRelu2, cgr(m.encoder1.ConvBnRelu1, x0, lazy=True), pool=True)
        down2, p2 = cgr(m.encoder2.ConvBnRelu2, cgr(m.encoder2.ConvBnRelu1, p1, lazy=True), pool=True)
        down3, p3 = cgr(m.encoder3.ConvBnRelu2, cgr(m.encoder3.ConvBnRelu1, p2, lazy=True), pool=True)
        down4 = cgr(m.encoder4.ConvBnRelu2, cgr(m.encoder4.ConvBnRelu1, p3, lazy=True))
        # bottom (:477-478): dilated block, then conv over cat[down4, bottom]
        bottom = cgr(m.bottom.ConvBnRelu2, cgr(m.bottom.ConvBnRelu1, down4, lazy=True), lazy=not _deep_heads_on(m))
        bottom_2 = cgr(m.bottom_2, down4, x2=bottom)
        # decoder (:481-486)
        outs = _decoder_fwd(ctx, cx, down1, down2, down3, down4, bottom, bottom_2)
        if m.refinement:  # (networks/equiunet2020.py:490-491: out = [refunet(out), out])
            outs.insert(0, _ref_fwd(ctx, cx, outs[0]))
        return tuple(outs)

    def _program_bwd(self, ctx, cx, *douts):
        m = cx.m
        down1, down2, down3 = ctx.bufs[:3]
        cbw = functools.partial(_cgr_bwd, cx)

        level_bwd = functools.partial(_level_bwd, cx)
        if m.refinement:  # the stage runs first: (d_refined, d_out, deep...) -> (the whole gradient of out, deep...)
            douts = (_ref_bwd(ctx, cx, douts[0], douts[1]),) + tuple(douts[2:])

        d_skip1, d_skip2, d_skip3, d_b2, d_deep_bottom = _decoder_bwd(ctx, cx, douts)
        d_skip4, d_bot = cbw(m.bottom_2, d_b2)
        d_bottom = _plus(d_bot, d_deep_bottom)
        c1, c2 = _blk(m.bottom)
        d_down4 = d_skip4 + cbw(c1, cbw(c2, d_bottom, bst=c1))
        c1, c2 = _blk(m.encoder4)
        d_p3 = cbw(c1, cbw(c2, d_down4, bst=c1))
        c1, c2 = _blk(m.encoder3)
        d_p2 = cbw(c1, level_bwd(c2, down3, d_p3, d_skip3, bst=c1))
        c1, c2 = _blk(m.encoder2)
        d_p1 = cbw(c1, level_bwd(c2, down2, d_p2, d_skip2, bst=c1))
        c1, c2 = _blk(m.encoder1)
        cbw(c1, level_bwd(c2, down1, d_p1, d_skip1, bst=c1), need_dx=False)
        ctx.bufs = None
