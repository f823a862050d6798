"""The four multi-label criteria of src/definer.py:204-245 restated in plain torch -- dice_ce (the reference's DiceCELoss with
sigmoid=True), dice_focal, focal and tversky (monai 0.6.0 DiceFocalLoss, FocalLoss, TverskyLoss) -- and deep supervision as the
mean over the heads, with values and gradients from autograd.  Runs on the CPU in the dtype it is given (float64: the reference
value; float32: the reference's own error, which sets the tests' bar).

x: logits [N, K, D, H, W]; t: target of the same shape (binary and overlapping in BraTS use); p = sigmoid(x)."""
import torch
import torch.nn.functional as F

SPATIAL = (2, 3, 4)


def dice(x, t, jaccard=False, batch=False, smooth_nr=1e-5, smooth_dr=1e-5):
    """monai DiceLoss(sigmoid=True, squared_pred=True, include_background=True, reduction="mean")"""
    p = torch.sigmoid(x)
    axes = (0,) + SPATIAL if batch else SPATIAL
    inter = (p * t).sum(axes)
    den = (t * t).sum(axes) + (p * p).sum(axes)
    if jaccard:
        den = 2.0 * (den - inter)
    return (1.0 - (2.0 * inter + smooth_nr) / (den + smooth_dr)).mean()


def bce_with_logits(x, t):
    """the max-subtracted form monai 0.6.0 FocalLoss writes out"""
    m = (-x).clamp(min=0)
    return x - x * t + m + ((-m).exp() + (-x - m).exp()).log()


def focal_elements(x, t, gamma=2.0):
    return (F.logsigmoid(-x * (t * 2 - 1)) * gamma).exp() * bce_with_logits(x, t)


def focal(x, t, gamma=2.0):
    """monai 0.6.0 FocalLoss(gamma, reduction="mean"): the mean over all N K V elements"""
    return focal_elements(x, t, gamma).mean()


def tversky(x, t, alpha=0.5, beta=0.5, batch=False, smooth_nr=1e-5, smooth_dr=1e-5):
    """monai TverskyLoss(sigmoid=True, include_background=True, reduction="mean")"""
    p = torch.sigmoid(x)
    axes = (0,) + SPATIAL if batch else SPATIAL
    tp = (p * t).sum(axes)
    fp = alpha * (p * (1 - t)).sum(axes)
    fn = beta * ((1 - p) * t).sum(axes)
    return (1.0 - (tp + smooth_nr) / (tp + fp + fn + smooth_dr)).mean()


def class_map(t):
    """DiceCELoss.ce (learning/losses.py:571): torch.argmax over the channels, ties to the lowest one"""
    return torch.argmax(t, dim=1)


def dice_ce(x, t, jaccard=False, batch=True, smooth_nr=1e-5, smooth_dr=1e-5, lambda_dice=1.0, lambda_ce=1.0):
    """learning/losses.py:470-595 with sigmoid=True, squared_pred=True: the cross-entropy is on the raw logits"""
    ce = F.cross_entropy(x, class_map(t), reduction="mean")
    return lambda_dice * dice(x, t, jaccard, batch, smooth_nr, smooth_dr) + lambda_ce * ce


def dice_focal(x, t, jaccard=False, batch=False, smooth_nr=1e-5, smooth_dr=1e-5, gamma=2.0, lambda_dice=1.0, lambda_focal=1.0):
    """monai 0.6.0 DiceFocalLoss(sigmoid=True, squared_pred=True)"""
    return lambda_dice * dice(x, t, jaccard, batch, smooth_nr, smooth_dr) + lambda_focal * focal(x, t, gamma)


CRITERIA = {"dice_ce": dice_ce, "dice_focal": dice_focal, "focal": focal, "tversky": tversky}


def deep_loss_and_grads(name, heads, target, dtype, **options):
    """mean over the heads of criterion `name` (learning/engine.py:322-330) in `dtype` -> (value as float, [gradient per head])."""
    xs = [h.detach().to(dtype).requires_grad_(True) for h in heads]
    t = target.to(dtype)
    loss = torch.stack([CRITERIA[name](x, t, **options) for x in xs]).mean()
    loss.backward()
    return float(loss.detach().double()), [x.grad.detach() for x in xs]
