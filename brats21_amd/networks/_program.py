"""What the network programs (equiunet.py, equiunet_assp.py, att_equiunet.py and the U-Net family of unet.py / r2unet.py) share: the
module base with the precision / fold switches and the forward() body, the per-pass context their unit programs take as first
argument, the one autograd Function that runs a network's forward / backward program methods inside the plan + split-precision
scoping, and the backward of the 1x1x1 heads."""
import os

import torch
import torch.nn as nn

from .. import ops
from .._lib import BratsHipError


class _PackedWeightsModule(nn.Module):
    """Base of every network.  A network supplies its programs as two methods, _program_fwd(ctx, cx, x0) -> tuple of logits and
    _program_bwd(ctx, cx, *douts), which leaves the parameter gradients in cx.grads (_ProgramFn).  Keeps ops' no_grad packed-weight cache honest: the cache is dropped on every train() /
    eval() transition and on every grad-enabled forward, so weights changed without a version bump (``p.data.copy_`` of the
    reference's Ranger2020, learning/optimizer.py:243,253) are never served stale to a later evaluation."""

    PRECISIONS = ("auto", "bf16", "fp16", "fp32", "x3", "fp16x3", "bf16x3", "x3fwd", "x3bwd")
    _cpu_hint = ""  # tail of the "GPU only" message
    _cpad = None    # channels the network input is zero-padded to; None: input_cpad decides (R2Unet sets its own)

    @property
    def precision(self):
        return self._precision

    @precision.setter
    def precision(self, value):
        # a typo ("X3", "x3 ") must not fall through to autocast / exact f32 under a parity-mode label
        if value not in self.PRECISIONS:
            raise ValueError(f"model.precision / BRATS_PRECISION must be one of {self.PRECISIONS}, got {value!r}")
        self._precision = value

    def train(self, mode=True):
        if mode != self.training:
            ops.invalidate_packed_weights()
        return super().train(mode)

    def _init_switches(self, pack_plan):
        """The run-time switches both networks read.  pack_plan: the default of BRATS_PACK_PLAN ("0" | "1")."""
        # "auto" = follow torch.autocast; BRATS_PRECISION=x3 makes the split-precision parity mode the default of an unmodified
        # training script run with --no_amp
        self.precision = os.environ.get("BRATS_PRECISION", "auto")
        # None | "fwd" | "all": run the 3x3x3 convolutions (forward / forward + input gradients) on the e4m3 MFMA kernel
        # when the activations are 16-bit (BASELINE.json configs[4]); the weight gradients stay 16-bit where no e4m3 form is built
        self.conv_fp8 = None
        self.skip_deep_heads_in_eval = False
        self._grad_sink = None  # set by brats21_amd.ddp.GradientBuckets
        self._grad_dest = None  # (ditto: parameter index -> its slice of an all-reduce bucket, or None)
        # training: one multi-tensor weight-packing launch per step (ops.PackPlan)
        self.pack_plan = os.environ.get("BRATS_PACK_PLAN", pack_plan) != "0"
        # the output head's backward inside the norm backward of the last layer / block (brats_gn_act_bwd_head,
        # brats_evonorm_se_bwd with dlogits); 0: the separate brats_head_bwd pass, for same-box A/B runs
        self.fold_head_bwd = os.environ.get("BRATS_FOLD_HEAD", "1") != "0"
        # the pooling backward + skip add inside the norm backward of the level's last layer / block (brats_gn_act_bwd_pool,
        # brats_evonorm_se_bwd_pool)
        self.fold_pool_bwd = os.environ.get("BRATS_FOLD_POOL", "1") != "0"
        # the norm backward's first pass of a block's first unit inside the input-gradient launch of its second convolution
        # (ops.conv3d_bstats + ops.gn_act_bwd_tiles / ops.evonorm_bwd_tiles): dz and y are read once instead of twice
        self.fold_bwd_stats = os.environ.get("BRATS_FOLD_BWD_STATS", "1") != "0"
        # ... and the head's forward on the last layer's raw convolution output (brats_gn_head_fwd, brats_evonorm_head_fwd):
        # up1 is never stored
        self.fold_head_fwd = os.environ.get("BRATS_FOLD_HEAD_FWD", os.environ.get("BRATS_FOLD_HEAD", "1")) != "0"

    def _init_dropout(self, p):
        """--dropout p (src/arguments_train.py:52).  The masks come from this library's Philox stream (csrc/dropout.hip), seeded
        from torch's CPU generator at construction (torch.manual_seed makes a run repeatable); the (seed, step counter) pair is a
        non-persistent buffer: not part of the state dict, like torch's own RNG state."""
        if not 0.0 <= float(p) < 1.0:
            raise ValueError(f"dropout probability has to be in [0, 1), got {p}")
        self.dropout_p = float(p)
        # The seed comes from a PRIVATE generator seeded with torch.initial_seed(): constructing a model never advances the global
        # CPU generator (the initial weights under a given torch.manual_seed do not depend on --dropout), and p = 0 draws
        # nothing.  Data-parallel ranks build identical replicas under one torch seed: the rank is mixed in at the first forward
        # (RANK of the launcher, else torch.distributed's rank) so that they draw different masks.
        seed = 0
        if self.dropout_p > 0.0:
            seed = int(torch.randint(0, 2 ** 62, (1,), generator=torch.Generator().manual_seed(torch.initial_seed())))
        self._dropout_seed_base, self._dropout_rank_mixed = seed, self.dropout_p == 0.0
        self.register_buffer("_dropout_state", torch.tensor([seed, 0], dtype=torch.int64), persistent=False)

    def _advance_dropout(self, device):
        """Next step's dropout state: the counter moves ON THE DEVICE (a captured step draws fresh masks at every replay); the
        returned copy belongs to this forward / backward pair."""
        if self._dropout_state.device != device:
            raise BratsHipError("brats21_amd: module and input are on different devices")
        if not self._dropout_rank_mixed:
            rank = os.environ.get("RANK")
            if rank is None:
                import torch.distributed as dist
                rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
            self._dropout_state[0] = (self._dropout_seed_base + 0x9E3779B97F4A7C15 * int(rank)) % (2 ** 63)
            self._dropout_rank_mixed = True
        self._dropout_state[1] += 1
        return self._dropout_state.clone()

    def _weights_may_have_changed(self):
        if torch.is_grad_enabled():
            ops.invalidate_packed_weights()

    def _dtype(self):
        if self.precision == "bf16":
            return torch.bfloat16
        if self.precision == "fp16":
            return torch.float16
        if self.precision in ("fp32", "x3", "fp16x3", "bf16x3", "x3fwd", "x3bwd"):
            return torch.float32
        if torch.is_autocast_enabled():  # the reference's switch (learning/engine.py:304): its autocast dtype is fp16
            return torch.float16 if torch.get_autocast_dtype("cuda") == torch.float16 else torch.bfloat16
        return torch.float32

    def _x3_modes(self):
        """(forward, backward) split of the 3x3x3 convolutions when the activations are f32 (ops.split_precision):
        precision "x3" (= "fp16x3") = fp16 pairs (f32-class: 2^-22 per product) forward AND backward -- dY, whose values lie far
        below fp16's range, is scaled by a power of two from the |max| its producer kernel records (brats_conv3d_x3_fwd /
        _x3_wgrad; the reference needs a GradScaler for the same reason); "bf16x3" = bf16 pairs everywhere (2^-16 per product:
        logits ~5e-4, gradients ~5e-3 from f64 -- measured, tests/test_x3_gpu.py); anything else = the exact-f32 MFMA kernels."""
        if self.precision in ("x3", "fp16x3"):
            return ops.X3F, ops.X3F
        if self.precision == "bf16x3":
            return ops.X3B, ops.X3B
        if self.precision in ("x3fwd", "x3bwd"):  # (diagnostic: one pass split, the other exact f32)
            return (ops.X3F, None) if self.precision == "x3fwd" else (None, ops.X3F)
        return None, None

    MAX_INPLANES = MAX_CLASSES = 16

    def _check_shape_limits(self, inplanes, num_classes, features, width_multiple):
        """What the kernels cover of the reference's constructor arguments: the layout conversion pads the input to at most 16
        channels, brats_head_fwd / brats_head_bwd take at most 16 classes, the convolutions whole channel vectors."""
        if int(inplanes) != inplanes or int(num_classes) != num_classes or inplanes < 1 or num_classes < 1:
            raise ValueError(f"{self.name}: inplanes and num_classes must be positive integers (got {inplanes!r}, {num_classes!r})")
        if inplanes > self.MAX_INPLANES:
            raise NotImplementedError(f"{self.name}: the input layer is built for inplanes <= {self.MAX_INPLANES} (got {inplanes})")
        if num_classes > self.MAX_CLASSES:
            raise NotImplementedError(f"{self.name}: the head kernels are built for num_classes <= {self.MAX_CLASSES} (got {num_classes})")
        if any(c % width_multiple for c in features):
            raise NotImplementedError(f"{self.name}: the convolution kernels need widths that are multiples of {width_multiple} "
                                      f"(got {list(features)})")
        self.inplanes = int(inplanes)

    def _run(self, x):
        """forward(x) of every network."""
        if not x.is_cuda:
            raise BratsHipError(f"brats21_amd.{self.name} runs on the GPU only (no CPU fallback){self._cpu_hint}")
        if x.dim() != 5 or x.shape[1] != self.inplanes or any(s % 8 for s in x.shape[2:]):
            raise ValueError(f"expected input [N, {self.inplanes}, D, H, W] with D, H, W divisible by 8")
        refinement = getattr(self, "refinement", False)
        if refinement and any(s % 16 for s in x.shape[2:]):  # (four pooled levels; the reference fails in torch.cat there)
            raise ValueError(f"refinement=True: expected input [N, {self.inplanes}, D, H, W] with D, H, W divisible by 16")
        if refinement and self.conv_fp8:
            raise NotImplementedError("refinement=True with the e4m3 convolution path (conv_fp8) is not implemented")
        self._fwd_grad = torch.is_grad_enabled()  # (inside autograd.Function.forward grad mode is always off)
        self._weights_may_have_changed()
        if self.training and self.pack_plan and torch.is_grad_enabled():
            ops.plan_for(self, x.device)  # all layers' weights (forward + dgrad layouts) packed by one launch
        outs = _ProgramFn.apply(self, x.float(), self._dtype(), *self.parameters())
        if refinement:  # networks/equiunet2020.py:490-498: the first element is the list [refined, out]
            return ([outs[0], outs[1]], list(outs[2:])) if self.deep_supervision else [outs[0], outs[1]]
        if self.deep_supervision:
            return outs[0], list(outs[1:])
        return outs[0]


# ------------------------------------------------------------------------------------------ per-pass context
class _AmaxSlots:
    """Zero-initialised device scalars for the |max| side outputs of the producer kernels (one fill per pass)."""

    def __init__(self, n, device):
        self.buf = torch.zeros(n, dtype=torch.float32, device=device)
        self.i = 0

    def take(self):
        s = self.buf[self.i:self.i + 1]
        self.i += 1
        return s


def _inherit_amax(dst, src):
    """max-pooling / trilinear interpolation never exceed the |max| of their input."""
    a = getattr(src, "_amax", None)
    if a is not None:
        dst._amax = a
    return dst


def douts_device(douts):
    return next(d.device for d in douts if d is not None)


class _Ctx:
    """State of one forward (and its backward) shared by the unit programs of a network."""

    def __init__(self, model, dtype, will_bwd=False):
        self.m, self.dtype = model, dtype
        # e4m3 convolutions (model.conv_fp8): the norm / SE kernels record the |max| of what they write into slots taken
        # here; a tensor without a recorded |max| falls back to ops.absmax inside ops.conv3d_f8
        self.fp8 = getattr(model, "conv_fp8", None) if ops.is16(dtype) else None
        # split precision on fp16 pairs (backward): dy is scaled by a power of two from its recorded |max| (_x3_modes)
        self.x3s = ops.x3_mode() == ops.X3F and dtype == torch.float32
        self.slots = None
        self._names = None
        self.grads = {}
        self.recs = {}  # unit -> what its backward needs
        # nn.Dropout(p), training mode only: (p, state) with state = (seed, step counter) on the device; None = off
        self.drop = None
        self.act, self.training = getattr(model, "act", None), model.training
        self.will_bwd = will_bwd
        # inference (no_grad, 16-bit): an activation with ONE reader, the next convolution, is never stored (ops.Pending:
        # normalise + act applied on load, model.norm_on_load)
        self.lazy_ok = (not will_bwd and not torch.is_grad_enabled() and getattr(model, "norm_on_load", False)
                        and ops.is16(dtype))

    @property
    def names(self):
        if self._names is None:
            self._names = {p: i for i, p in enumerate(self.m.parameters())}
        return self._names

    def start_dropout(self, device):
        """The state (seed, step counter) is advanced on the device and a copy travels to the backward, which regenerates the
        masks from it."""
        m = self.m
        if m.training and m.dropout_p > 0.0:
            if self.fp8:
                raise NotImplementedError("--dropout > 0 with the e4m3 convolution path is not implemented")
            self.drop = (m.dropout_p, m._advance_dropout(device))

    def drop_of(self, unit):
        """The unit's dropout stream; None: dropout is off."""
        return self.m._unit_ids[unit] if self.drop is not None else None

    def dropped(self, t, uid, out=None):
        """t * keep / (1 - p) with unit uid's mask of this step (forward: in place on the activation; backward: on the gradient)."""
        if self.drop is None or uid is None:
            return t
        return ops.dropout(t, self.drop[0], self.drop[1], uid, out=out)

    def slot(self, device, force=False):
        if not self.fp8 and not force:
            return None
        if self.slots is None or self.slots.i >= self.slots.buf.numel():
            self.slots = _AmaxSlots(64, device)
        return self.slots.take()

    def identity_ss(self, n, c, device):
        """{scale, shift} = {1, 0} per (sample, channel): ops.conv3d_bstats' activation argument when there is no activation."""
        key = (n, c)
        if getattr(self, "_ss", None) is None:
            self._ss = {}
        if key not in self._ss:
            ss = torch.zeros((n, c, 2), dtype=torch.float32, device=device)
            ss[..., 0] = 1.0
            self._ss[key] = ss
        return self._ss[key]

    def dest(self, param):
        """The parameter's slice of a DDP all-reduce bucket (ddp.GradientBuckets.dest) for kernels that can write there."""
        d = getattr(self.m, "_grad_dest", None)
        return d(self.names[param]) if d is not None else None

    def put(self, param, grad):
        """A finished gradient; data-parallel: handed to the bucketed all-reduce right away."""
        i = self.names[param]
        self.grads[i] = grad.reshape(param.shape)
        if self.m._grad_sink is not None:
            self.m._grad_sink(i, self.grads[i])


# ------------------------------------------------------------------------------------------ autograd Function scoping
def input_cpad(inplanes, dtype):
    """Channels of the NDHWC network input: inplanes zero-padded to what the first convolution has a channel chunk for -- 8 or 16
    in the 16-bit and split-precision modes, 4, 8 or 16 in exact f32.  (4 modalities: 8 / 4, one 16-byte vector per voxel.)"""
    cands = (8, 16) if (ops.is16(dtype) or ops.x3_active()) else (4, 8, 16)
    return next(c for c in cands if c >= inplanes)


def _fn_forward(program, ctx, model, x, dtype, params, cpad=None):
    """_ProgramFn.forward around the network's forward program(ctx, cx, x0) -> tuple of logits.  cpad: the channels the network
    input is zero-padded to where the network wants other than input_cpad's."""
    # training: the module packed all layers' weights up front (ops.plan_for); pack_weights() then returns views
    ctx.plan = ops._PLANS.get(model) if (model.training and model.pack_plan) else None
    ctx.x3 = model._x3_modes() if dtype == torch.float32 else (None, None)
    ctx.nparams = len(params)
    with ops.use_plan(ctx.plan), ops.split_precision(ctx.x3[0]):
        ctx.cx = cx = _Ctx(model, dtype, will_bwd=any(ctx.needs_input_grad) and model._fwd_grad)  # (needs_input_grad ignores no_grad)
        cx.start_dropout(x.device)
        x0 = ops.ncdhw_to_ndhwc(x, dtype, cpad=cpad or input_cpad(x.shape[1], dtype))
        x0._net_input = True  # (un-normalised: never an e4m3 operand, whatever its padded width)
        if ops.x3_mode() == ops.X3F:
            # fp16 pairs overflow at |x| >= 65504 (hi = inf, lo = NaN: silently NaN logits).  Every other convolution
            # input is a normalised activation; the network INPUT is whatever the caller passes (un-normalised volumes reach
            # 3e4 and more), so its |max| is recorded (one 134 MB pass at 2 x 128^3) and the first layer's forward scales by the
            # matching power of two (brats_conv3d_x3_fwd's xamax: exact).  The first layer's WEIGHT gradient still splits the
            # unscaled input: split-precision training expects z-scored inputs like the reference's pipeline produces
            # (utils/transforms.py:364-385), inference does not.
            x0._x3amax = ops.absmax(x0)
        return program(ctx, cx, x0)


def _fn_backward(program, ctx, douts):
    """_ProgramFn.backward around the network's backward program(ctx, cx, *douts), which leaves the parameter gradients in
    cx.grads."""
    cx = ctx.cx
    with ops.use_plan(ctx.plan), ops.split_precision(ctx.x3[1]):
        cx.x3s = ops.x3_mode() == ops.X3F and cx.dtype == torch.float32  # (the BACKWARD split decides about the dy scales)
        program(ctx, cx, *douts)
    ctx.cx = None
    return (None, None, None) + tuple(cx.grads.get(i) for i in range(ctx.nparams))


class _ProgramFn(torch.autograd.Function):
    """The autograd Function of every network: model's own programs."""

    @staticmethod
    def forward(ctx, model, x, dtype, *params):
        return _fn_forward(model._program_fwd, ctx, model, x, dtype, params, cpad=model._cpad)

    @staticmethod
    def backward(ctx, *douts):
        return _fn_backward(ctx.cx.m._program_bwd, ctx, douts)


def _heads_bwd(ctx, cx, douts, fold):
    """Backward of the 1x1x1 heads, ctx.heads = [(head, source tensor, scale)] with the output head first: d(logits) -> gradient
    w.r.t. their NDHWC source tensors.  fold: the output head's backward rides in the backward of the last layer (always when
    its forward was fused: ctx.top_fused).  Returns (top, dsrc): top = (output head, dlogits) when folded, else None; dsrc =
    {source data_ptr: gradient}."""
    dsrc, top, out_head = {}, None, ctx.heads[0][0]
    for (hd, src, sc), dout in zip(ctx.heads, douts):
        if dout is None and hd is out_head and ctx.top_fused:
            # a loss built from the deep heads only: the fused top has no stored up1 to fall back on -- zero logit gradients
            dout = torch.zeros((ctx.out_shape), dtype=torch.float32, device=douts_device(douts))
        if dout is None:
            continue
        if hd is out_head and (ctx.top_fused or fold):
            top = (hd, dout)
            continue
        dx, dw, db = ops.head_bwd(src, hd.weight, dout, sc)
        cx.put(hd.weight, dw)
        cx.put(hd.bias, db)
        key = src.data_ptr()
        dsrc[key] = dx if key not in dsrc else dsrc[key] + dx
    return top, dsrc
