"""Validation metrics of the reference (utils/metrics.py) on the GPU: hard Dice, Hausdorff distance 95, sensitivity and
specificity of 0/1 masks [N, K, D, H, W], with the reference's conventions for empty labels.

The Hausdorff distance is a HIP pipeline (csrc/metrics.hip): union box, edge masks, an exact separable squared
Euclidean distance transform to the other map's edges, a histogram of the squared distances at the source edges and an
exact percentile.  Sensitivity and specificity come from the exact counts of csrc/post.hip (|P & T|, |P|, |T|).
``get_metric_callable`` / ``compute_metric_tensor`` / ``set_labels`` take the reference's arguments and return what it
returns, so learning/engine.py:27 can import them from here.

Semantics are MONAI 0.6.0's (requirements.txt:17) as the reference calls it (include_background=True,
learning/engine.py:52-54):
  * A channel exists when it has a non-zero voxel.  Neither mask exists: Dice = 1, HD = 0, sensitivity = specificity = 1.
    Exactly one exists: Dice = 0, sensitivity = specificity = 0 and HD = sqrt(240^2 + 240^2 + 155^2) in float32 -- the
    reference hard-codes the BraTS volume (utils/metrics.py:74-79) whatever the input shape, and so does this module.
  * Edges (get_mask_edges(crop=True)): voxels equal to 1 are foreground; both masks are cropped to the bounding box of
    their union and np.squeeze()d; edges = fg ^ binary_erosion(fg) with the 6-neighbour cross and the outside as 0.
    Because of the squeeze an axis along which the box is one voxel thick is not eroded along.
  * HD = max(p(d(pred -> target)), p(d(target -> pred))) with np.percentile's linear method (numpy's _lerp, its t >= 0.5
    branch included); percentile None (or 0, MONAI's `if not percentile`) is the maximum; directed=True keeps the first
    term.  The raw function returns what MONAI does where a side has no edge: both -> NaN; exactly one -> inf for the
    maximum, NaN for a percentile (np.percentile of an all-inf array).

Where results can differ from the reference:
  1. Degenerate edge cases follow the published get_mask_edges bit for bit, as restated over scipy's own binary_erosion
     in tests/golden/make_golden_metrics.py: a one-voxel-thick slab has only its 2-D rim as edges, a one-voxel-wide line
     only its run ends, and a union of a single voxel squeezes to a 0-d array without edges, so its HD is NaN (not
     replaced, since both masks exist).
  2. The confusion counts are exact integers rounded once to float32; MONAI sums float32 values, which agrees exactly
     while a volume has fewer than 2^24 voxels (a BraTS volume has 9.2 million).
  3. Not provided: roc_auc and surface_distance (NotImplementedError; neither is a command-line choice, and the reference
     raises for surface_distance itself), and confusion-matrix metrics other than sensitivity and specificity.
  4. With include_background=False the conventions apply to the kept channels (the reference's own masks keep the
     background channel and would not broadcast); the reference only ever passes True.
  5. The masks must be 0/1: existence counts non-zero voxels where the reference takes amax != 0.
"""
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from .evaluate import _need_cuda, _stream, hard_dice_metric, overlap_counts

# utils/metrics.py:74-79: sqrt(sum((0 - (240, 240, 155))^2)) computed in float32 by torch
WORST_HAUSDORFF = float(torch.sqrt(torch.tensor(240.0 ** 2 + 240.0 ** 2 + 155.0 ** 2, dtype=torch.float32)))

METRICS = ("dice", "hausdorff_distance95", "sensitivity", "specificity")

# monai.metrics.confusion_matrix.check_confusion_matrix_metric_name (0.6.0), for the two metrics built here
_CONFUSION_NAMES = {
    "sensitivity": "tpr", "recall": "tpr", "hit_rate": "tpr", "true_positive_rate": "tpr", "tpr": "tpr",
    "specificity": "tnr", "selectivity": "tnr", "true_negative_rate": "tnr", "tnr": "tnr",
}
# the other names MONAI accepts there: the reference would route them to the confusion matrix, this module does not
_CONFUSION_OTHER = {
    "precision", "positive_predictive_value", "ppv", "negative_predictive_value", "npv", "miss_rate",
    "false_negative_rate", "fnr", "fall_out", "false_positive_rate", "fpr", "false_discovery_rate", "fdr",
    "false_omission_rate", "for", "prevalence_threshold", "pt", "threat_score", "critical_success_index", "ts", "csi",
    "accuracy", "acc", "balanced_accuracy", "ba", "f1_score", "f1", "matthews_correlation_coefficient", "mcc",
    "fowlkes_mallows_index", "fm", "informedness", "bookmaker_informedness", "bm", "markedness", "deltap", "mk",
}


def _pair(y_pred, y, what):
    _need_cuda(y_pred, what)
    _need_cuda(y, what)
    if y_pred.shape != y.shape or y_pred.device != y.device:
        raise ValueError(f"y_pred {tuple(y_pred.shape)} on {y_pred.device} and y {tuple(y.shape)} on {y.device} differ")
    if y_pred.dim() != 5:
        raise ValueError(f"expected [N, K, D, H, W] masks, got {tuple(y_pred.shape)}")
    return y_pred.contiguous().float(), y.contiguous().float()


def _drop_background(y_pred, y, include_background):
    return (y_pred, y) if include_background else (y_pred[:, 1:], y[:, 1:])


def _percentile_arg(percentile):
    if not percentile:  # MONAI: `if not percentile: return surface_distance.max()`
        return -1.0
    p = float(percentile)
    if not 0 <= p <= 100:
        raise ValueError(f"percentile should be a value between 0 and 100, get {percentile}.")
    return p


def hausdorff_distance(y_pred, y, percentile=95, directed=False, include_background=True):
    """MONAI 0.6.0 compute_hausdorff_distance(distance_metric="euclidean") on the GPU: device float32 [N, K] with MONAI's
    raw values (NaN / inf where a side has no edge; module docstring).  CUDA tensors only."""
    p, t = _pair(y_pred, y, "hausdorff_distance")
    pct = _percentile_arg(percentile)
    p, t = _drop_background(p, t, include_background)
    p, t = p.contiguous(), t.contiguous()
    n, k = p.shape[:2]
    out = torch.empty((n, k), dtype=torch.float32, device=p.device)
    if n * k == 0:
        return out
    d, h, w = (int(s) for s in p.shape[2:])
    with torch.cuda.device(p.device):
        ws = torch.empty(max(1, _lib.lib().brats_hausdorff_ws_bytes(n * k, d, h, w)), dtype=torch.uint8, device=p.device)
        _lib.check(_lib.lib().brats_hausdorff(p.data_ptr(), t.data_ptr(), n * k, d, h, w, pct, 1 if directed else 0,
                                              out.data_ptr(), ws.data_ptr(), _stream()), "hausdorff")
    return out


def confusion_matrix(y_pred, y, include_background=True):
    """MONAI 0.6.0 get_confusion_matrix: float32 [N, K, 4] = (tp, fp, tn, fn) per (n, k), from exact counts."""
    p, t = _pair(y_pred, y, "confusion_matrix")
    p, t = _drop_background(p, t, include_background)
    vox = p[0, 0].numel() if p.numel() else 0
    c = overlap_counts(p, t)
    tp, ps, ts = c[..., 0], c[..., 1], c[..., 2]
    fp, fn = ps - tp, ts - tp
    tn = vox - ps - ts + tp
    return torch.stack([tp, fp, tn, fn], dim=-1).float()


def _confusion_metric(cm, name):
    """monai.metrics.compute_confusion_matrix_metric (0.6.0) for tpr / tnr: float32, NaN where the denominator is 0."""
    tp, fp, tn, fn = cm[..., 0], cm[..., 1], cm[..., 2], cm[..., 3]
    num, den = (tp, tp + fn) if _CONFUSION_NAMES[name] == "tpr" else (tn, fp + tn)
    return (num / den).masked_fill(den == 0, float("nan"))


def _existence(y_pred, y):
    c = overlap_counts(y_pred, y)
    return c[..., 1] > 0, c[..., 2] > 0


def _conventions(value, ep, et, best, worst):
    """utils/metrics.py:47-79,96-101: both absent -> best, exactly one absent -> worst (no host copies: capturable)."""
    return value.masked_fill(~ep & ~et, best).masked_fill(ep ^ et, worst)


def _check_names(metrics):
    if isinstance(metrics, str):
        metrics = (metrics,)
    metrics = tuple(metrics)
    bad = [m for m in metrics if m not in METRICS]
    if bad:
        raise ValueError(f"unknown metric(s) {bad}; choose from {METRICS}")
    return metrics


def brats_metrics(y_pred, y, metrics=METRICS):
    """{name: device float32 [N, K]} for the chosen names of METRICS, with the reference's best / worst conventions
    (utils/metrics.py:35-104, include_background=True).  CUDA tensors only."""
    metrics = _check_names(metrics)
    p, t = _pair(y_pred, y, "brats_metrics")
    out = {}
    if not metrics:
        return out
    ep, et = _existence(p, t)
    cm = None
    for m in metrics:
        if m == "dice":
            out[m] = hard_dice_metric(p, t)
        elif m == "hausdorff_distance95":
            out[m] = _conventions(hausdorff_distance(p, t, 95), ep, et, 0.0, WORST_HAUSDORFF)
        else:
            cm = confusion_matrix(p, t) if cm is None else cm
            out[m] = _conventions(_confusion_metric(cm, m), ep, et, 1.0, 0.0)
    return out


# ---- drop-ins for utils/metrics.py (imported by learning/engine.py:27) -------------------------------------------------
def set_labels(labels):
    """utils/metrics.py:21-32."""
    if isinstance(labels, int):
        labels = [labels]
    if isinstance(labels, (list, tuple)):
        labels = OrderedDict({str(k): k for k in labels})
    elif isinstance(labels, dict):
        labels = OrderedDict({str(k): v for k, v in labels.items()})
    return OrderedDict({k: v for k, v in sorted(labels.items(), key=lambda item: item[1])})


class DiceMetric:
    """Stands for monai.metrics.DiceMetric in get_metric_callable's dictionary."""

    def __init__(self, include_background=True, reduction="none"):
        self.include_background, self.reduction = include_background, reduction


class HausdorffDistanceMetric:
    """Stands for monai.metrics.HausdorffDistanceMetric(distance_metric="euclidean", percentile=95)."""

    def __init__(self, include_background=True, percentile=95, directed=False, reduction="none"):
        self.include_background, self.percentile, self.directed = include_background, percentile, directed
        self.reduction = reduction

    def __call__(self, y_pred, y):
        return hausdorff_distance(y_pred, y, self.percentile, self.directed, self.include_background)


class ConfusionMatrixMetric:
    """Stands for monai.metrics.ConfusionMatrixMetric(metric_name=..., compute_sample=False)."""

    def __init__(self, metric_name, include_background=True, reduction="none"):
        self.metric_name, self.include_background, self.reduction = list(metric_name), include_background, reduction

    def __call__(self, y_pred, y):
        return confusion_matrix(y_pred, y, self.include_background)


def get_metric_callable(metrics_type, include_background=True, reduction="none"):
    """utils/metrics.py:137-167: {callable: [title-cased names]}; the callables are this module's stand-ins, to be passed
    to compute_metric_tensor.  Raises NotImplementedError for roc_auc, surface_distance and unknown names."""
    if isinstance(metrics_type, str):
        raise TypeError("metrics_type must be a sequence of metric names, not a string")
    names = list(metrics_type)
    for m in names:
        if not isinstance(m, str):
            raise TypeError(f"metric names must be strings, got {m!r}")
    conf = [m for m in names if m.lower() in _CONFUSION_NAMES]
    for m in names:
        low = m.lower()
        if low in _CONFUSION_OTHER:
            raise NotImplementedError(f"the confusion-matrix metric {m} is not provided on the GPU (only sensitivity and "
                                      "specificity are)")
        if low == "roc_auc":
            raise NotImplementedError("roc_auc is not provided on the GPU (it is not a command-line choice of the reference)")
        if low == "surface_distance":
            raise NotImplementedError("surface_distance is not provided (the reference raises for it too)")
    kw = {"include_background": include_background, "reduction": reduction}
    out = OrderedDict()
    seen = set()
    for m in names:
        if m in conf or m in seen:
            continue
        seen.add(m)
        low = m.lower()
        if low == "hausdorff_distance95":
            fn = HausdorffDistanceMetric(percentile=95, **kw)
        elif low == "dice":
            fn = DiceMetric(**kw)
        else:
            raise NotImplementedError(f"the metric {m} is not implemented.")
        out[fn] = [m.title()]
    if conf:
        conf = list(OrderedDict.fromkeys(conf))
        out[ConfusionMatrixMetric(metric_name=conf, **kw)] = [m.title() for m in conf]
    return out


def compute_metric_tensor(y_pred, y, callable_metric_dict, y_probs=None):
    """utils/metrics.py:35-134 -> (OrderedDict {name: float32 numpy [N, K]}, confusion matrix [[tp, fp], [fn, tn]] of
    the last confusion-matrix callable (numpy, squeezed as the reference does) or None).  The work runs on the GPU; CPU
    tensors are copied there."""
    if not (torch.is_tensor(y_pred) and torch.is_tensor(y)):
        raise TypeError("y_pred and y must be torch tensors")
    if y_pred.shape != y.shape:
        raise ValueError(f"y_pred {tuple(y_pred.shape)} and y {tuple(y.shape)} differ")
    if y_pred.dim() != 5:
        raise ValueError(f"expected [N, K, D, H, W] masks, got {tuple(y_pred.shape)}")
    for fn in callable_metric_dict:
        if not isinstance(fn, (DiceMetric, HausdorffDistanceMetric, ConfusionMatrixMetric)):
            raise NotImplementedError(f"{type(fn).__name__} is not a metric of brats21_amd.metrics.get_metric_callable")
    dev = y_pred.device if y_pred.is_cuda else (y.device if y.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    results = OrderedDict()
    confusion = None
    with torch.cuda.device(dev):
        p, t = y_pred.to(dev).contiguous().float(), y.to(dev).contiguous().float()
        cache = {}

        def exist(include_background):
            if include_background not in cache:
                cache[include_background] = _existence(*_drop_background(p, t, include_background))
            return cache[include_background]

        for fn, names in callable_metric_dict.items():
            ep, et = exist(fn.include_background)
            if isinstance(fn, DiceMetric):
                value = hard_dice_metric(*_drop_background(p, t, fn.include_background))
                results[names[0]] = value.cpu().numpy()
            elif isinstance(fn, HausdorffDistanceMetric):
                value = _conventions(fn(p, t), ep, et, 0.0, WORST_HAUSDORFF)
                results[names[0]] = value.cpu().numpy()
            else:
                cm = fn(p, t)
                for name in names:
                    results[name] = _conventions(_confusion_metric(cm, name.lower()), ep, et, 1.0, 0.0).cpu().numpy()
                tp, fp, tn, fn_ = (cm[..., i].squeeze().cpu().numpy() for i in range(4))
                confusion = np.array([[tp, fp], [fn_, tn]])
    return results, confusion
