"""The exclusive-class criterion restated in plain torch: DiceCELoss(softmax=True, to_onehot_y=True, reduction="mean") of the
reference's learning/losses.py -- monai DiceLoss over softmax probabilities and the one-hot of the label map, plus
F.cross_entropy(ignore_index=255) -- with values and gradients from autograd.  Runs on the CPU in the dtype it is given
(float64: the reference value; float32: the reference's own error, which sets the tests' bar).

Voxels whose label is not one of 0 .. K-1 must be 255 here; they are left out of BOTH parts (the Dice sums are masked), which
is what brats21_amd.losses.SoftmaxDiceCELoss documents."""
import torch
import torch.nn.functional as F

IGNORE = 255
OPTIONS = dict(include_background=True, squared_pred=True, jaccard=False, batch=True, smooth_nr=1e-5, smooth_dr=1e-5, lambda_dice=1.0,
               lambda_ce=1.0)


def softmax_dice_ce(logits, labels, **options):
    """logits [N, K, D, H, W] (any float dtype, CPU), labels [N, D, H, W] integer with values in 0 .. K-1 or 255."""
    o = dict(OPTIONS, **options)
    k = logits.shape[1]
    y = labels.long()
    valid = (y != IGNORE)
    assert bool(((y < k) | ~valid).all()), "labels outside 0 .. K-1 must be 255 in the restatement"
    m = valid.unsqueeze(1).to(logits.dtype)
    p = torch.softmax(logits, 1) * m
    t = F.one_hot(torch.where(valid, y, 0), k).movedim(-1, 1).to(logits.dtype) * m
    if not o["include_background"]:
        p, t = p[:, 1:], t[:, 1:]
    axes = (0, 2, 3, 4) if o["batch"] else (2, 3, 4)
    inter = (p * t).sum(axes)
    pred = (p * p if o["squared_pred"] else p).sum(axes)
    den = t.sum(axes) + pred
    if o["jaccard"]:
        den = 2.0 * (den - inter)
    dice = (1.0 - (2.0 * inter + o["smooth_nr"]) / (den + o["smooth_dr"])).mean()
    ce = F.cross_entropy(logits, y, ignore_index=IGNORE, reduction="mean")
    return o["lambda_dice"] * dice + o["lambda_ce"] * ce


def deep_loss_and_grads(heads, labels, dtype, **options):
    """mean over the heads of the criterion (learning/engine.py:322-330) in `dtype` -> (value as float, [gradient per head])."""
    xs = [h.detach().to(dtype).requires_grad_(True) for h in heads]
    loss = torch.stack([softmax_dice_ce(x, labels, **options) for x in xs]).mean()
    loss.backward()
    return float(loss.detach().double()), [x.grad.detach() for x in xs]


def ignore_above(labels, k):
    """the label map with every value >= k replaced by 255"""
    return torch.where(labels.long() < k, labels.long(), IGNORE).to(torch.uint8)
