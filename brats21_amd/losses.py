"""Loss that "stays in PyTorch-ROCm" (BASELINE.json north_star): the Dice / Jaccard criterion the
reference configures at src/definer.py:184-203 (monai.losses.DiceLoss(include_background=True,
sigmoid=True, squared_pred=True, batch=True, reduction='mean', smooth 1e-5)) and the
deep-supervision averaging of learning/engine.py:312-333; and the distance-map criteria of learning/losses.py:59-467
(HausdorffLoss, DiceHDLoss, SurfaceLoss = BoundaryLoss, DiceBoundaryLoss) as src/definer.py:246-282 configures them, on
csrc/edt.hip + csrc/dist_loss.hip: no host round trip, so a step with them captures into a hipGraph like the Dice step; and, for
K exclusive classes, SoftmaxDiceCELoss = learning/losses.py DiceCELoss(softmax=True, to_onehot_y=True) on csrc/softmax_loss.hip;
and the multi-label criteria src/definer.py:204-245 configures as dice_ce, dice_focal, focal and tversky (DiceCELoss, DiceFocalLoss,
FocalLoss, TverskyLoss) on csrc/sigmoid_loss.hip."""
import ctypes
from collections.abc import Sequence

import torch
import torch.nn as nn

from ._tensors import _vec


class DiceLoss(nn.Module):
    def __init__(self, jaccard=False, smooth_nr=1e-5, smooth_dr=1e-5):
        super().__init__()
        self.jaccard, self.smooth_nr, self.smooth_dr = jaccard, smooth_nr, smooth_dr

    def forward(self, logits, target):
        p = torch.sigmoid(logits.float())
        t = target.float()
        axes = (0, 2, 3, 4)  # batch=True: the batch dimension is reduced too
        inter = (t * p).sum(axes)
        denom = (t * t).sum(axes) + (p * p).sum(axes)
        if self.jaccard:
            denom = 2.0 * (denom - inter)
        return (1.0 - (2.0 * inter + self.smooth_nr) / (denom + self.smooth_dr)).mean()


def flatten_heads(outputs):
    """Every tensor of a network output in order, as the reference's ``flatten`` does (learning/engine.py:322-330):
    (out, [deep...]) -> [out, deep...]; with the refinement stage ([refined, out], [deep...]) -> [refined, out, deep...]."""
    if isinstance(outputs, (tuple, list)):
        return [h for o in outputs for h in flatten_heads(o)]
    return [outputs]


def deep_supervision_loss(criterion, outputs, target):
    """mean over [main] + deep heads of criterion(head, label) (learning/engine.py:322-330); returns (loss, first head) -- the
    refined logits where the network has the refinement stage."""
    if isinstance(outputs, (tuple, list)):
        heads = flatten_heads(outputs)
        return torch.stack([criterion(h, target) for h in heads]).mean(), heads[0]
    return criterion(outputs, target), outputs


MAX_FUSED_HEADS, MAX_FUSED_CLASSES = 8, 16  # brats_dice_stats_multi / brats_dice_finish


def _pointer_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[x.data_ptr() for x in tensors])


class _FusedDiceFn(torch.autograd.Function):
    """loss = mean over heads and classes of (1 - (2I+eps)/(D+eps)), no host sync.  Heads of the target's shape (the training
    step: every deep head is up-sampled to full size): three launches for all of them -- brats_dice_stats_multi,
    brats_dice_finish (the ordered sums, the [heads, classes] algebra, the loss) and brats_dice_grad_multi -- with the target
    read once per pass.  Heads in any other form (a strided view, another dtype, more than 8 of them): two HBM passes per head
    (brats_dice_stats / brats_dice_grad), the algebra in torch.  Both paths give the same bits; the loss value could differ in
    its last place where the kernel's order of the final mean is not torch's (csrc/dice.hip, dice_mean)."""

    @staticmethod
    def forward(ctx, target, jaccard, eps, *heads):
        from . import _lib
        lib = _lib.lib()
        st = torch.cuda.current_stream().cuda_stream
        t = target.contiguous().float()
        n, k = t.shape[:2]
        vox = t[0, 0].numel()
        ctx.multi = (len(heads) <= MAX_FUSED_HEADS and k <= MAX_FUSED_CLASSES and n * k <= 65535 and t.is_cuda
                     and all(h.shape == t.shape and h.dtype == torch.float32 and h.is_contiguous() and h.device == t.device for h in heads))
        if ctx.multi:
            nh = len(heads)
            with torch.cuda.device(t.device):
                ws = torch.empty(lib.brats_dice_multi_ws_floats(nh, n, k), dtype=torch.float32, device=t.device)
                sums = torch.empty((nh, k, 3), dtype=torch.float32, device=t.device)
                coef = torch.empty((nh, k, 2), dtype=torch.float32, device=t.device)
                loss = torch.empty((), dtype=torch.float32, device=t.device)
                _lib.check(lib.brats_dice_stats_multi(_pointer_array(heads), nh, t.data_ptr(), ws.data_ptr(), n, k, vox, st), "dice_stats_multi")
                _lib.check(lib.brats_dice_finish(ws.data_ptr(), nh, n, k, vox, eps, int(bool(jaccard)), sums.data_ptr(), coef.data_ptr(),
                                                 loss.data_ptr(), st), "dice_finish")
            ctx.save_for_backward(t, coef, *heads)
            return loss
        hs = [h.contiguous().float() for h in heads]
        for h in hs:  # (the fused path compared every head with the target above; this one indexes them by the target's sizes too)
            _vec(h, t.numel(), "fused Dice: head", t)
        sums = torch.empty((len(hs), k, 3), dtype=torch.float32, device=t.device)
        ws = torch.empty(lib.brats_dice_ws_floats(n, k), dtype=torch.float32, device=t.device)  # per-block partials
        for i, h in enumerate(hs):
            _lib.check(lib.brats_dice_stats(h.data_ptr(), t.data_ptr(), sums[i].data_ptr(), ws.data_ptr(), n, k, vox, st), "dice_stats")
        inter, p2, t2 = sums[..., 0], sums[..., 1], sums[..., 2]
        hk = float(len(hs) * k)
        if jaccard:
            den = 2.0 * (t2 + p2 - inter)
            f = 1.0 - (2.0 * inter + eps) / (den + eps)
            dden = (2.0 * inter + eps) / (den + eps) ** 2
            coef = torch.stack([(-2.0 / (den + eps) - 2.0 * dden) / hk, 2.0 * dden / hk], -1)
        else:
            den = t2 + p2
            f = 1.0 - (2.0 * inter + eps) / (den + eps)
            coef = torch.stack([-2.0 / (den + eps) / hk, (2.0 * inter + eps) / (den + eps) ** 2 / hk], -1)
        ctx.save_for_backward(t, coef.contiguous(), *hs)
        return f.mean()

    @staticmethod
    def backward(ctx, g):
        from . import _lib
        lib = _lib.lib()
        st = torch.cuda.current_stream().cuda_stream
        t, coef, *hs = ctx.saved_tensors
        n, k = t.shape[:2]
        vox = t[0, 0].numel()
        if ctx.multi:  # coef * g is formed inside the kernel from the device scalar g
            g = g.to(device=t.device, dtype=torch.float32)
            with torch.cuda.device(t.device):
                outs = [torch.empty_like(h) for h in hs]
                _lib.check(lib.brats_dice_grad_multi(_pointer_array(hs), len(hs), t.data_ptr(), coef.data_ptr(), g.data_ptr(),
                                                     _pointer_array(outs), n, k, vox, st), "dice_grad_multi")
            return (None, None, None) + tuple(outs)
        coef = (coef * g).contiguous()
        outs = []
        for i, h in enumerate(hs):
            d = torch.empty_like(h)
            _lib.check(lib.brats_dice_grad(h.data_ptr(), t.data_ptr(), coef[i].data_ptr(), d.data_ptr(), n, k, vox, st), "dice_grad")
            outs.append(d)
        return (None, None, None) + tuple(outs)


def fused_deep_supervision_dice(outputs, target, jaccard=False, eps=1e-5):
    """Same value and gradients as deep_supervision_loss(DiceLoss(jaccard), outputs, target), fused."""
    heads = flatten_heads(outputs)
    return _FusedDiceFn.apply(target, jaccard, eps, *heads)


# ------------------------------------------------------------------------------------------ distance-map criteria
def _check_reference_options(name, sigmoid, softmax, to_onehot_y, other_act, reduction):
    """The option set src/definer.py:246-282 uses; everything else the reference's classes accept is not built."""
    if not sigmoid:
        raise NotImplementedError(f"{name}: only sigmoid=True is built (the kernels fuse the sigmoid, src/definer.py:246-282)")
    if softmax or to_onehot_y or other_act is not None:
        raise NotImplementedError(f"{name}: softmax / to_onehot_y / other_act are not built (the reference factory never sets them)")
    if getattr(reduction, "value", reduction) != "mean":
        raise NotImplementedError(f"{name}: only reduction='mean' is built")


def _select(t, idc):
    """t[:, idc] as contiguous f32; the full channel range (the factory's case) costs no copy."""
    t = t.float()
    if list(idc) != list(range(t.shape[1])):
        t = t[:, list(idc)]
    return t.contiguous()


def _need_cuda(t, what):
    if not t.is_cuda:
        from . import _lib
        raise _lib.BratsHipError(f"brats21_amd.losses.{what} runs on the GPU only (no CPU fallback)")


class PreparedTarget:
    """What a distance-map criterion derives from the target alone (criterion.prepare(target)): computed once per step and
    shared by every deep-supervision head instead of once per head (learning/engine.py:326-329 recomputes it)."""

    def __init__(self, owner, target, **fields):
        self.owner, self.target = owner, target
        self.__dict__.update(fields)


def sigmoid_one_hot(logits):
    """probs2one_hot(sigmoid(logits)) (learning/losses.py:43-56) as uint8 [N, K, ...]: 1 on the arg-max channel of every voxel,
    ties to the lowest channel (csrc/dist_loss.hip)."""
    from . import _lib
    _need_cuda(logits, "sigmoid_one_hot")
    x = logits.detach().contiguous().float()
    n, k = x.shape[:2]
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().brats_sigmoid_argmax_onehot(x.data_ptr(), out.data_ptr(), n, k, x[0, 0].numel(),
                                                          torch.cuda.current_stream().cuda_stream), "sigmoid_argmax_onehot")
    return out


def _loss_ws(lib, device):
    return torch.empty(lib.brats_dist_loss_ws_floats(), dtype=torch.float32, device=device)


class _HausdorffFn(torch.autograd.Function):
    """mean of (p - t)^2 (tdm^alpha + pdm^alpha); the fields carry no gradient.  One statistics pass and one gradient pass
    (brats_hd_loss_stats / brats_hd_loss_grad), the weight recomputed from the two fields in the backward."""

    @staticmethod
    def forward(ctx, logits, t, tdm, pdm, alpha):
        from . import _lib
        lib = _lib.lib()
        x = logits.contiguous().float()
        total = x.numel()
        s = torch.empty(1, dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(lib.brats_hd_loss_stats(_vec(x, None, "HausdorffLoss: logits", None), _vec(t, total, "HausdorffLoss: target", x),
                                               _vec(tdm, total, "HausdorffLoss: target field", x),
                                               _vec(pdm, total, "HausdorffLoss: predicted field", x), alpha, s.data_ptr(),
                                               _loss_ws(lib, x.device).data_ptr(), total,
                                               torch.cuda.current_stream().cuda_stream), "hd_loss_stats")
        ctx.save_for_backward(x, t, tdm, pdm)
        ctx.alpha = alpha
        return s[0] / total

    @staticmethod
    def backward(ctx, g):
        from . import _lib
        x, t, tdm, pdm = ctx.saved_tensors
        total = x.numel()
        scale = (g.float() / total).reshape(1).contiguous()
        dx = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().brats_hd_loss_grad(x.data_ptr(), t.data_ptr(), tdm.data_ptr(), pdm.data_ptr(), ctx.alpha,
                                                     scale.data_ptr(), dx.data_ptr(), total,
                                                     torch.cuda.current_stream().cuda_stream), "hd_loss_grad")
        return dx, None, None, None, None


class _BoundaryFn(torch.autograd.Function):
    """mean of p * dist (brats_boundary_loss_stats / brats_boundary_loss_grad)."""

    @staticmethod
    def forward(ctx, logits, dist):
        from . import _lib
        lib = _lib.lib()
        x = logits.contiguous().float()
        total = x.numel()
        s = torch.empty(1, dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(lib.brats_boundary_loss_stats(_vec(x, None, "BoundaryLoss: logits", None),
                                                     _vec(dist, total, "BoundaryLoss: distance map", x), s.data_ptr(),
                                                     _loss_ws(lib, x.device).data_ptr(),
                                                     total, torch.cuda.current_stream().cuda_stream), "boundary_loss_stats")
        ctx.save_for_backward(x, dist)
        return s[0] / total

    @staticmethod
    def backward(ctx, g):
        from . import _lib
        x, dist = ctx.saved_tensors
        total = x.numel()
        scale = (g.float() / total).reshape(1).contiguous()
        dx = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().brats_boundary_loss_grad(x.data_ptr(), dist.data_ptr(), scale.data_ptr(), dx.data_ptr(), total,
                                                           torch.cuda.current_stream().cuda_stream), "boundary_loss_grad")
        return dx, None


class _DiceFn(torch.autograd.Function):
    """monai DiceLoss(sigmoid, squared_pred, reduction mean) on the kernels of the fused Dice (brats_dice_stats /
    brats_dice_grad): batch=False -- one value per (n, k), one call per sample on its contiguous slice -- or batch=True."""

    @staticmethod
    def forward(ctx, logits, t, jaccard, smooth_nr, smooth_dr, batch):
        from . import _lib
        lib = _lib.lib()
        st = torch.cuda.current_stream().cuda_stream
        x = logits.contiguous().float()
        n, k = x.shape[:2]
        vox = x[0, 0].numel()
        _vec(x, None, "Dice: logits", None)
        _vec(t, x.numel(), "Dice: target", x)
        groups = [(x, t, n)] if batch else [(x[i], t[i], 1) for i in range(n)]
        sums = torch.empty((len(groups), k, 3), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            ws = torch.empty(lib.brats_dice_ws_floats(n, k), dtype=torch.float32, device=x.device)
            for i, (xs, ts, ns) in enumerate(groups):
                _lib.check(lib.brats_dice_stats(xs.data_ptr(), ts.data_ptr(), sums[i].data_ptr(), ws.data_ptr(), ns, k, vox, st), "dice_stats")
        inter, p2, t2 = sums[..., 0], sums[..., 1], sums[..., 2]
        cnt = float(len(groups) * k)
        num = 2.0 * inter + smooth_nr
        if jaccard:
            den = 2.0 * (t2 + p2 - inter) + smooth_dr
            coef = torch.stack([(-2.0 / den - 2.0 * num / den ** 2) / cnt, 2.0 * num / den ** 2 / cnt], -1)
        else:
            den = t2 + p2 + smooth_dr
            coef = torch.stack([-2.0 / den / cnt, num / den ** 2 / cnt], -1)
        ctx.save_for_backward(x, t, coef.contiguous())
        ctx.batch = batch
        return (1.0 - num / den).mean()

    @staticmethod
    def backward(ctx, g):
        from . import _lib
        lib = _lib.lib()
        st = torch.cuda.current_stream().cuda_stream
        x, t, coef = ctx.saved_tensors
        n, k = x.shape[:2]
        vox = x[0, 0].numel()
        coef = (coef * g).contiguous()
        dx = torch.empty_like(x)
        groups = [(x, t, dx, n)] if ctx.batch else [(x[i], t[i], dx[i], 1) for i in range(n)]
        with torch.cuda.device(x.device):
            for i, (xs, ts, ds, ns) in enumerate(groups):
                _lib.check(lib.brats_dice_grad(xs.data_ptr(), ts.data_ptr(), coef[i].data_ptr(), ds.data_ptr(), ns, k, vox, st), "dice_grad")
        return dx, None, None, None, None, None


class _PreparedCriterion(nn.Module):
    """criterion(logits, target): target is what the reference passes (a tensor, or the pair [target, distance_map] of the
    boundary criteria, learning/engine.py:93-94) or the PreparedTarget of this criterion's prepare(target)."""

    def _prepared(self, target):
        if isinstance(target, PreparedTarget):
            if target.owner is not self:
                raise ValueError("the PreparedTarget was made by another criterion")
            return target
        return self.prepare(target)

    def forward(self, logits, target):
        _need_cuda(logits, type(self).__name__)
        return self._loss(logits, self._prepared(target))


class HausdorffLoss(_PreparedCriterion):
    """learning/losses.py:98-179 with sigmoid=True, reduction mean: mean over N x len(idc) x voxels of
    (p - t)^2 (tdm^alpha + pdm^alpha), tdm the distance transform of the target, pdm that of the arg-max one-hot of p
    truncated to integers (the reference computes it into an int32 array, learning/losses.py:37,88,158-162)."""

    def __init__(self, idc, alpha=2.0, to_onehot_y=False, sigmoid=False, softmax=False, other_act=None, reduction="mean"):
        super().__init__()
        _check_reference_options("HausdorffLoss", sigmoid, softmax, to_onehot_y, other_act, reduction)
        self.idc, self.alpha = list(idc), float(alpha)

    def prepare(self, target):
        from .ops import distance_transform_edt
        _need_cuda(target, "HausdorffLoss")
        t = _select(target, self.idc)
        return PreparedTarget(self, target, t=t, tdm=distance_transform_edt(t))

    def _loss(self, logits, prep):
        from .ops import distance_transform_edt
        if logits.shape[0] != prep.t.shape[0] or logits.shape[2:] != prep.t.shape[2:] or logits.shape[1] != prep.target.shape[1]:
            raise AssertionError(f"ground truth has different shape ({tuple(prep.target.shape)}) from input ({tuple(logits.shape)})")
        onehot = sigmoid_one_hot(logits)  # the arg-max runs over ALL channels, idc selects afterwards (learning/losses.py:158-159)
        x = logits
        if self.idc != list(range(logits.shape[1])):
            x, onehot = logits[:, self.idc], onehot[:, self.idc].contiguous()
        # mode 2: the reference's predicted field is truncated (its one-hot is int32 and one_hot2hd_dist fills zeros_like of it)
        return _HausdorffFn.apply(x, prep.t, prep.tdm, distance_transform_edt(onehot, mode=2), self.alpha)


class SurfaceLoss(_PreparedCriterion):
    """learning/losses.py:296-355 with sigmoid=True, reduction mean: mean of p * dist over N x len(idc) x voxels; `dist` is
    the precomputed map (transforms.one_hot_to_dist) -- element 1 when the target is the pair [target, distance_map]."""

    def __init__(self, idc, to_onehot_y=False, sigmoid=False, softmax=False, other_act=None, reduction="mean"):
        super().__init__()
        _check_reference_options(type(self).__name__, sigmoid, softmax, to_onehot_y, other_act, reduction)
        self.idc = list(idc)

    def prepare(self, target):
        dist = target[1] if isinstance(target, Sequence) else target
        _need_cuda(dist, "SurfaceLoss")
        return PreparedTarget(self, target, full_shape=tuple(dist.shape), dist=_select(dist, self.idc))

    def _loss(self, logits, prep):
        if tuple(logits.shape) != prep.full_shape:
            raise AssertionError(f"distance map has different shape ({prep.full_shape}) from input ({tuple(logits.shape)})")
        x = logits if self.idc == list(range(logits.shape[1])) else logits[:, self.idc]
        return _BoundaryFn.apply(x, prep.dist)


BoundaryLoss = SurfaceLoss


class _SigmoidDice(nn.Module):
    """The monai DiceLoss inside the two hybrid criteria: sigmoid, squared_pred, include_background, reduction mean."""

    def __init__(self, name, include_background, squared_pred, jaccard, smooth_nr, smooth_dr, batch):
        super().__init__()
        if not include_background or not squared_pred:
            raise NotImplementedError(f"{name}: the Dice part is built for include_background=True, squared_pred=True "
                                      "(src/definer.py:254-282)")
        self.jaccard, self.smooth_nr, self.smooth_dr, self.batch = bool(jaccard), float(smooth_nr), float(smooth_dr), bool(batch)

    def forward(self, logits, t):
        if logits.shape != t.shape:
            raise AssertionError(f"ground truth has different shape ({tuple(t.shape)}) from input ({tuple(logits.shape)})")
        return _DiceFn.apply(logits, t, self.jaccard, self.smooth_nr, self.smooth_dr, self.batch)


class DiceHDLoss(_PreparedCriterion):
    """learning/losses.py:182-293: Dice + Hausdorff loss (hybrid=True: weight_dice * Dice + weight_hd * hd).  batch=False,
    the reference factory's setting, is one Dice value per (sample, class)."""

    def __init__(self, idc_hd, alpha_hd=2, hybrid=False, weight_hd=0.5, weight_dice=0.5, include_background=True, to_onehot_y=False,
                 sigmoid=False, softmax=False, other_act=None, squared_pred=False, jaccard=False, reduction="mean", smooth_nr=1e-5,
                 smooth_dr=1e-5, batch=False):
        super().__init__()
        self.hd = HausdorffLoss(idc=idc_hd, alpha=alpha_hd, to_onehot_y=to_onehot_y, sigmoid=sigmoid, softmax=softmax,
                                other_act=other_act, reduction=reduction)
        self.dice = _SigmoidDice("DiceHDLoss", include_background, squared_pred, jaccard, smooth_nr, smooth_dr, batch)
        self.hybrid, self.weight_hd, self.weight_dice = bool(hybrid), float(weight_hd), float(weight_dice)

    def prepare(self, target):
        hd = self.hd.prepare(target)
        full = hd.t if hd.t.shape == target.shape else target.contiguous().float()
        return PreparedTarget(self, target, hd=hd, t=full)

    def _loss(self, logits, prep):
        if logits.dim() != prep.t.dim():
            raise ValueError("the number of dimensions for input and target should be the same.")
        dice, hd = self.dice(logits, prep.t), self.hd(logits, prep.hd)
        return self.weight_dice * dice + self.weight_hd * hd if self.hybrid else dice + hd


class DiceBoundaryLoss(_PreparedCriterion):
    """learning/losses.py:361-467: lambda_dice * Dice(input, target[0]) + lambda_boundary * SurfaceLoss(input, target[1]);
    the target is the pair [target, distance_map]."""

    def __init__(self, idc_boundary, include_background=True, to_onehot_y=False, sigmoid=False, softmax=False, other_act=None,
                 squared_pred=False, jaccard=False, reduction="mean", smooth_nr=1e-5, smooth_dr=1e-5, batch=False, lambda_dice=1.0,
                 lambda_boundary=1.0):
        super().__init__()
        self.boundary = BoundaryLoss(idc=idc_boundary, to_onehot_y=to_onehot_y, sigmoid=sigmoid, softmax=softmax, other_act=other_act,
                                     reduction=reduction)
        self.dice = _SigmoidDice("DiceBoundaryLoss", include_background, squared_pred, jaccard, smooth_nr, smooth_dr, batch)
        if lambda_dice < 0.0:
            raise ValueError("lambda_dice should be no less than 0.0.")
        if lambda_boundary < 0.0:
            raise ValueError("lambda_boundary should be no less than 0.0.")
        self.lambda_dice, self.lambda_boundary = float(lambda_dice), float(lambda_boundary)

    def prepare(self, target):
        if not isinstance(target, Sequence) or len(target) != 2:
            raise ValueError("DiceBoundaryLoss: the target is the pair [target, distance_map]")
        _need_cuda(target[0], "DiceBoundaryLoss")
        return PreparedTarget(self, target, boundary=self.boundary.prepare(target[1]), t=target[0].contiguous().float())

    def _loss(self, logits, prep):
        return self.lambda_dice * self.dice(logits, prep.t) + self.lambda_boundary * self.boundary(logits, prep.boundary)


# ------------------------------------------------------------------------------------------ exclusive classes
MAX_CLASSES = 16


def label_map_u8(target):
    """The target of an exclusive-class criterion as a contiguous uint8 label map [N, D, H, W]: an integer or float label map
    [N, 1, D, H, W] / [N, D, H, W] (values outside 0..255 become 255, which every class count ignores), or a one-hot
    [N, K, D, H, W], arg-maxed as DiceCELoss.ce does (brats_argmax_labels, ties to the lowest class)."""
    _need_cuda(target, "label_map_u8")
    if target.dim() == 5 and target.shape[1] != 1:
        from .ops import argmax_labels
        return argmax_labels(target)[:, 0]
    if target.dim() == 5:
        target = target[:, 0]
    if target.dim() != 4:
        raise AssertionError(f"ground truth must be a label map [N, 1, D, H, W] / [N, D, H, W] or a one-hot [N, K, D, H, W], "
                             f"got {tuple(target.shape)}")
    if target.dtype == torch.uint8:
        return target.contiguous()
    return torch.where((target >= 0) & (target <= 255), target, 255).to(torch.uint8).contiguous()


class _LabelTarget(PreparedTarget):
    """PreparedTarget of SoftmaxDiceCELoss: the uint8 label map, and per class count K (the heads of one step all have the
    same) the per-sample class counts G [N, K] and valid-voxel counts [N] (brats_label_stats), made on first use and kept."""

    def stats(self, k):
        if k not in self.counts:
            from . import _lib
            lib = _lib.lib()
            y = self.labels
            n = y.shape[0]
            out = torch.empty((n, k + 1), dtype=torch.float32, device=y.device)
            with torch.cuda.device(y.device):
                ws = torch.empty(lib.brats_label_stats_ws_floats(n), dtype=torch.float32, device=y.device)
                _lib.check(lib.brats_label_stats(y.data_ptr(), out.data_ptr(), ws.data_ptr(), n, k, y[0].numel(),
                                                 torch.cuda.current_stream().cuda_stream), "label_stats")
            self.counts[k] = (out[:, :k], out[:, k])
        return self.counts[k]


class _SoftmaxDiceCEFn(torch.autograd.Function):
    """lambda_dice * monai DiceLoss(softmax, to_onehot_y) + lambda_ce * CrossEntropyLoss(mean, ignore_index): one statistics
    pass and one gradient pass over the logits (brats_softmax_stats / brats_softmax_grad), the [N][K] algebra in torch, the
    valid-voxel count a device scalar: no host sync."""

    @staticmethod
    def forward(ctx, logits, y, g, valid, opt):
        from . import _lib
        lib = _lib.lib()
        x = logits.contiguous().float()
        n, k = x.shape[:2]
        vox = x[0, 0].numel()
        sums = torch.empty((n, 3 * k + 1), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            ws = torch.empty(lib.brats_softmax_ws_floats(n, k), dtype=torch.float32, device=x.device)
            _lib.check(lib.brats_softmax_stats(x.data_ptr(), _vec(y, n * vox, "SoftmaxDiceCELoss: labels", x, torch.uint8),
                                               sums.data_ptr(), ws.data_ptr(), n, k, vox,
                                               torch.cuda.current_stream().cuda_stream), "softmax_stats")
        s = sums[:, :3 * k].reshape(n, k, 3)
        if opt.batch:  # the batch dimension is reduced too: one Dice value per class
            s, g = s.sum(0, keepdim=True), g.sum(0, keepdim=True)
        inter, pred = s[..., 0], s[..., 1 if opt.squared_pred else 2]
        num = 2.0 * inter + opt.smooth_nr
        if opt.jaccard:
            den = 2.0 * (g + pred - inter) + opt.smooth_dr
            a, b = -2.0 / den - 2.0 * num / den ** 2, 2.0 * num / den ** 2
        else:
            den = g + pred + opt.smooth_dr
            a, b = -2.0 / den, num / den ** 2
        k0 = 0 if opt.include_background else 1
        f = (1.0 - num / den)[:, k0:]
        scale = opt.lambda_dice / f.numel()
        ab = torch.stack([a, b], -1) * scale
        ab[:, :k0] = 0.0
        count = valid.sum()
        coef = torch.cat([ab.expand(n, k, 2).reshape(n, 2 * k), (opt.lambda_ce / count).expand(n, 1)], 1)
        ctx.save_for_backward(x, y, coef.contiguous())
        ctx.squared_pred = opt.squared_pred
        return opt.lambda_dice * f.mean() + opt.lambda_ce * (sums[:, 3 * k].sum() / count)

    @staticmethod
    def backward(ctx, grad):
        from . import _lib
        x, y, coef = ctx.saved_tensors
        n, k = x.shape[:2]
        coef = (coef * grad).contiguous()
        dx = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().brats_softmax_grad(x.data_ptr(), y.data_ptr(), coef.data_ptr(), dx.data_ptr(), n, k, x[0, 0].numel(),
                                                     int(ctx.squared_pred), torch.cuda.current_stream().cuda_stream), "softmax_grad")
        return dx, None, None, None, None


class SoftmaxDiceCELoss(_PreparedCriterion):
    """learning/losses.py DiceCELoss(softmax=True, to_onehot_y=True, reduction="mean") for K exclusive classes (2 <= K <= 16):
    lambda_dice * monai DiceLoss(softmax, to_onehot_y, include_background, squared_pred, jaccard, batch, smooth_nr, smooth_dr)
    + lambda_ce * torch.nn.CrossEntropyLoss(reduction="mean", ignore_index).  The target is an integer label map [N, 1, D, H, W]
    or [N, D, H, W] of any integer or float dtype, or a one-hot [N, K, D, H, W].  A voxel whose label is not one of 0 .. K-1
    (255 = unlabelled) is ignored by BOTH parts: it enters no sum, no count and no gradient."""

    def __init__(self, include_background=True, squared_pred=True, jaccard=False, batch=True, smooth_nr=1e-5, smooth_dr=1e-5,
                 lambda_dice=1.0, lambda_ce=1.0):
        super().__init__()
        if lambda_dice < 0.0:
            raise ValueError("lambda_dice should be no less than 0.0.")
        if lambda_ce < 0.0:
            raise ValueError("lambda_ce should be no less than 0.0.")
        self.include_background, self.squared_pred, self.jaccard, self.batch = bool(include_background), bool(squared_pred), bool(jaccard), bool(batch)
        self.smooth_nr, self.smooth_dr, self.lambda_dice, self.lambda_ce = float(smooth_nr), float(smooth_dr), float(lambda_dice), float(lambda_ce)

    def prepare(self, target):
        return _LabelTarget(self, target, labels=label_map_u8(target), counts={})

    def forward(self, logits, target):
        raw = target.target if isinstance(target, PreparedTarget) else target
        k = logits.shape[1] if logits.dim() == 5 else 0
        if not 2 <= k <= MAX_CLASSES:
            raise NotImplementedError(f"SoftmaxDiceCELoss: logits {tuple(logits.shape)}: [N, K, D, H, W] with 2 <= K <= {MAX_CLASSES} is built")
        label_shape = (raw.shape[0],) + tuple(raw.shape[2 if raw.dim() == 5 else 1:])
        if raw.dim() not in (4, 5) or label_shape != (logits.shape[0],) + tuple(logits.shape[2:]) or (raw.dim() == 5 and raw.shape[1] not in (1, k)):
            raise AssertionError(f"ground truth has different shape ({tuple(raw.shape)}) from input ({tuple(logits.shape)})")
        return super().forward(logits, target)

    def _loss(self, logits, prep):
        g, valid = prep.stats(logits.shape[1])
        return _SoftmaxDiceCEFn.apply(logits, prep.labels, g, valid, self)


# ------------------------------------------------------------------------------------------ multi-label criteria: dice_ce, dice_focal, focal, tversky
SIG_FOCAL, SIG_CE = 1, 2  # BRATS_SIG_FOCAL, BRATS_SIG_CE of include/brats_hip.h


def _dice_algebra(inter, p2, t2, d):
    """monai DiceLoss(sigmoid, squared_pred, reduction mean) from the per-(sample, class) sums [N, K], `d` a _SigmoidDice:
    (value, d value / d I, d value / d P2), the derivatives [N, K]."""
    n = inter.shape[0]
    if d.batch:  # the batch dimension is reduced too: one Dice value per class
        inter, p2, t2 = inter.sum(0, keepdim=True), p2.sum(0, keepdim=True), t2.sum(0, keepdim=True)
    num = 2.0 * inter + d.smooth_nr
    if d.jaccard:
        den = 2.0 * (t2 + p2 - inter) + d.smooth_dr
        a, b = -2.0 / den - 2.0 * num / den ** 2, 2.0 * num / den ** 2
    else:
        den = t2 + p2 + d.smooth_dr
        a, b = -2.0 / den, num / den ** 2
    f = 1.0 - num / den
    return f.mean(), (a / f.numel()).expand(n, -1), (b / f.numel()).expand(n, -1)


class _SigmoidLossFn(torch.autograd.Function):
    """One of the four multi-label criteria: one statistics pass and one gradient pass over the logits (brats_sigmoid_loss_stats /
    brats_sigmoid_loss_grad, csrc/sigmoid_loss.hip); the criterion's `_algebra` turns the [N, K] sums into the value and the
    coefficient table in torch on the device, and the upstream gradient is multiplied into the table there: no host sync."""

    @staticmethod
    def forward(ctx, logits, prep, crit):
        from . import _lib
        lib = _lib.lib()
        x = logits.contiguous().float()
        n, k = x.shape[:2]
        vox = x[0, 0].numel()
        classmap = prep.classmap if crit.terms & SIG_CE else None
        sums = torch.empty((n, 4 * k + 1), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            ws = torch.empty(lib.brats_sigmoid_loss_ws_floats(n, k), dtype=torch.float32, device=x.device)
            _lib.check(lib.brats_sigmoid_loss_stats(x.data_ptr(), _vec(prep.t, x.numel(), "criterion: target", x),
                                                    _vec(classmap, n * vox, "criterion: class map", x, torch.uint8, null=True),
                                                    sums.data_ptr(), ws.data_ptr(), n, k, vox, crit.terms, crit.gamma,
                                                    torch.cuda.current_stream().cuda_stream), "sigmoid_loss_stats")
        inter, p2, p1, focal = sums[:, :4 * k].reshape(n, k, 4).unbind(-1)
        value, (a, b, c, fc), cce = crit._algebra(inter, p2, p1, focal, sums[:, 4 * k], prep.tsums[..., 0], prep.tsums[..., 1], vox)
        zero = torch.zeros((n, k), dtype=torch.float32, device=x.device)
        table = torch.stack([zero if v is None else v.expand(n, k) for v in (a, b, c, fc)], -1).reshape(n, 4 * k)
        coef = torch.cat([table, torch.full((n, 1), cce, dtype=torch.float32, device=x.device)], 1)
        ctx.save_for_backward(x, prep.t, classmap, coef)
        ctx.terms, ctx.gamma = crit.terms, crit.gamma
        return value

    @staticmethod
    def backward(ctx, grad):
        from . import _lib
        x, t, classmap, coef = ctx.saved_tensors
        n, k = x.shape[:2]
        coef = (coef * grad).contiguous()
        dx = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().brats_sigmoid_loss_grad(x.data_ptr(), t.data_ptr(), classmap.data_ptr() if classmap is not None else None,
                                                          coef.data_ptr(), dx.data_ptr(), n, k, x[0, 0].numel(), ctx.terms, ctx.gamma,
                                                          torch.cuda.current_stream().cuda_stream), "sigmoid_loss_grad")
        return dx, None, None


class _SigmoidCriterion(_PreparedCriterion):
    """Base of the four: `terms` (SIG_FOCAL | SIG_CE) says what the passes compute beside the Dice sums, `gamma` is the focal
    exponent.  prepare(target) is the one pass over the target of a step (brats_sigmoid_target_prepare): the upcast target, its
    per-(sample, class) sums T1 and T2 and, for the CE term, the class map -- shared by every deep-supervision head."""
    terms, gamma = 0, 0.0

    def prepare(self, target):
        from . import _lib
        lib = _lib.lib()
        _need_cuda(target, type(self).__name__)
        if target.dim() < 3 or target.shape[1] > MAX_CLASSES:
            raise NotImplementedError(f"{type(self).__name__}: target {tuple(target.shape)}: [N, K, ...] with K <= {MAX_CLASSES} is built")
        t = target.contiguous().float()
        n, k = t.shape[:2]
        tsums = torch.empty((n, k, 2), dtype=torch.float32, device=t.device)
        classmap = torch.empty((n,) + tuple(t.shape[2:]), dtype=torch.uint8, device=t.device) if self.terms & SIG_CE else None
        with torch.cuda.device(t.device):
            ws = torch.empty(lib.brats_sigmoid_loss_ws_floats(n, k), dtype=torch.float32, device=t.device)
            _lib.check(lib.brats_sigmoid_target_prepare(t.data_ptr(), tsums.data_ptr(), classmap.data_ptr() if classmap is not None else None,
                                                        ws.data_ptr(), n, k, t[0, 0].numel(),
                                                        torch.cuda.current_stream().cuda_stream), "sigmoid_target_prepare")
        return PreparedTarget(self, target, t=t, tsums=tsums, classmap=classmap)

    def forward(self, logits, target):
        raw = target.target if isinstance(target, PreparedTarget) else target
        if logits.dim() != raw.dim():
            raise ValueError("the number of dimensions for input and target should be the same.")
        if logits.shape != raw.shape:
            raise AssertionError(f"ground truth has different shape ({tuple(raw.shape)}) from input ({tuple(logits.shape)})")
        if logits.dim() < 3 or logits.shape[1] > MAX_CLASSES:
            raise NotImplementedError(f"{type(self).__name__}: logits {tuple(logits.shape)}: [N, K, ...] with K <= {MAX_CLASSES} is built")
        return super().forward(logits, target)

    def _loss(self, logits, prep):
        return _SigmoidLossFn.apply(logits, prep, self)


def _nonnegative(**lambdas):
    for name, v in lambdas.items():
        if v < 0.0:
            raise ValueError(f"{name} should be no less than 0.0.")
    return [float(v) for v in lambdas.values()]


class DiceCELoss(_SigmoidCriterion):
    """learning/losses.py:470-595 as src/definer.py:204-212 configures it (sigmoid=True, squared_pred=True, batch=True):
    lambda_dice * monai DiceLoss(sigmoid) + lambda_ce * torch.nn.CrossEntropyLoss(mean) on the raw logits against
    y = argmax_k target (DiceCELoss.ce: ties to the lowest channel, so a background voxel and an all-ones voxel are class 0 --
    the reference's behaviour, kept).  For one class out of K per voxel see SoftmaxDiceCELoss."""
    terms = SIG_CE

    def __init__(self, include_background=True, to_onehot_y=False, sigmoid=False, softmax=False, other_act=None, squared_pred=False,
                 jaccard=False, reduction="mean", smooth_nr=1e-5, smooth_dr=1e-5, batch=False, ce_weight=None, lambda_dice=1.0,
                 lambda_ce=1.0):
        super().__init__()
        if softmax and to_onehot_y:
            raise NotImplementedError("DiceCELoss(softmax=True, to_onehot_y=True) is losses.SoftmaxDiceCELoss")
        _check_reference_options("DiceCELoss", sigmoid, softmax, to_onehot_y, other_act, reduction)
        if ce_weight is not None:
            raise NotImplementedError("DiceCELoss: ce_weight is not built (the reference factory never sets it)")
        self.dice = _SigmoidDice("DiceCELoss", include_background, squared_pred, jaccard, smooth_nr, smooth_dr, batch)
        self.lambda_dice, self.lambda_ce = _nonnegative(lambda_dice=lambda_dice, lambda_ce=lambda_ce)

    def _algebra(self, inter, p2, p1, focal, ce, t1, t2, vox):
        dice, a, b = _dice_algebra(inter, p2, t2, self.dice)
        voxels = float(inter.shape[0] * vox)
        value = self.lambda_dice * dice + self.lambda_ce * (ce.sum() / voxels)
        return value, (self.lambda_dice * a, self.lambda_dice * b, None, None), self.lambda_ce / voxels


class DiceFocalLoss(_SigmoidCriterion):
    """monai 0.6.0 DiceFocalLoss as src/definer.py:213-221 configures it (sigmoid=True, squared_pred=True, batch=False):
    lambda_dice * DiceLoss(sigmoid) + lambda_focal * FocalLoss(gamma) on the raw logits."""
    terms = SIG_FOCAL

    def __init__(self, include_background=True, to_onehot_y=False, sigmoid=False, softmax=False, other_act=None, squared_pred=False,
                 jaccard=False, reduction="mean", smooth_nr=1e-5, smooth_dr=1e-5, batch=False, gamma=2.0, focal_weight=None,
                 lambda_dice=1.0, lambda_focal=1.0):
        super().__init__()
        _check_reference_options("DiceFocalLoss", sigmoid, softmax, to_onehot_y, other_act, reduction)
        if focal_weight is not None:
            raise NotImplementedError("DiceFocalLoss: focal_weight is not built (the reference factory never sets it)")
        self.dice = _SigmoidDice("DiceFocalLoss", include_background, squared_pred, jaccard, smooth_nr, smooth_dr, batch)
        self.gamma = float(gamma)
        self.lambda_dice, self.lambda_focal = _nonnegative(lambda_dice=lambda_dice, lambda_focal=lambda_focal)

    def _algebra(self, inter, p2, p1, focal, ce, t1, t2, vox):
        dice, a, b = _dice_algebra(inter, p2, t2, self.dice)
        elements = float(focal.numel() * vox)
        value = self.lambda_dice * dice + self.lambda_focal * (focal.sum() / elements)
        return value, (self.lambda_dice * a, self.lambda_dice * b, None, torch.full_like(focal, self.lambda_focal / elements)), 0.0


class FocalLoss(_SigmoidCriterion):
    """monai 0.6.0 FocalLoss(gamma, reduction mean) (src/definer.py:232-236): the mean over N x K x voxels of
    exp(gamma logsigmoid(-x (2t - 1))) bce(x, t) on the raw logits -- (1 - p_t)^gamma BCE for a binary target."""
    terms = SIG_FOCAL

    def __init__(self, include_background=True, to_onehot_y=False, gamma=2.0, weight=None, reduction="mean"):
        super().__init__()
        _check_reference_options("FocalLoss", True, False, to_onehot_y, None, reduction)
        if not include_background or weight is not None:
            raise NotImplementedError("FocalLoss: include_background=False and class weights are not built (src/definer.py:232-236)")
        self.gamma = float(gamma)

    def _algebra(self, inter, p2, p1, focal, ce, t1, t2, vox):
        elements = float(focal.numel() * vox)
        return focal.sum() / elements, (None, None, None, torch.full_like(focal, 1.0 / elements)), 0.0


class TverskyLoss(_SigmoidCriterion):
    """monai TverskyLoss(sigmoid, alpha, beta, reduction mean) (src/definer.py:237-245): per (sample, class) -- per class with
    batch=True -- 1 - (tp + smooth_nr) / (tp + alpha fp + beta fn + smooth_dr), tp = sum p t, fp = sum p (1 - t),
    fn = sum (1 - p) t."""

    def __init__(self, include_background=True, to_onehot_y=False, sigmoid=False, softmax=False, other_act=None, alpha=0.5, beta=0.5,
                 reduction="mean", smooth_nr=1e-5, smooth_dr=1e-5, batch=False):
        super().__init__()
        _check_reference_options("TverskyLoss", sigmoid, softmax, to_onehot_y, other_act, reduction)
        if not include_background:
            raise NotImplementedError("TverskyLoss: include_background=False is not built (src/definer.py:237-245)")
        self.alpha, self.beta, self.smooth_nr, self.smooth_dr, self.batch = float(alpha), float(beta), float(smooth_nr), float(smooth_dr), bool(batch)

    def _algebra(self, inter, p2, p1, focal, ce, t1, t2, vox):
        n = inter.shape[0]
        if self.batch:
            inter, p1, t1 = inter.sum(0, keepdim=True), p1.sum(0, keepdim=True), t1.sum(0, keepdim=True)
        num = inter + self.smooth_nr
        den = inter + self.alpha * (p1 - inter) + self.beta * (t1 - inter) + self.smooth_dr
        f = 1.0 - num / den
        a = (-1.0 / den + num / den ** 2 * (1.0 - self.alpha - self.beta)) / f.numel()
        c = num / den ** 2 * self.alpha / f.numel()
        return f.mean(), (a.expand(n, -1), None, c.expand(n, -1), None), 0.0


def deep_supervision_prepared_loss(criterion, outputs, target):
    """deep_supervision_loss for a criterion with a prepare(target) step: what depends on the target alone (its distance
    field, the selected and upcast tensors) is computed once and shared by the main and the deep heads.  Same value and
    gradients as deep_supervision_loss(criterion, outputs, target), bit for bit."""
    prepared = criterion.prepare(target)
    if isinstance(outputs, (tuple, list)):
        heads = flatten_heads(outputs)
        return torch.stack([criterion(h, prepared) for h in heads]).mean(), heads[0]
    return criterion(outputs, prepared), outputs
