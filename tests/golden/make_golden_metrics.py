"""Generates tests/golden/metrics.npz from the REFERENCE's own utils/metrics.py (get_metric_callable,
compute_metric_tensor) imported under oracle/refshim.py, the way make_golden_postproc.py does.

Run here only (the GPU box has no reference checkout):  python tests/golden/make_golden_metrics.py
MONAI 0.6.0 is not installed: the stub modules below restate the pieces utils/metrics.py touches -- DiceMetric
(compute_meandice), HausdorffDistanceMetric (compute_hausdorff_distance, compute_percent_hausdorff_distance,
get_mask_edges(crop=True) with generate_spatial_bounding_box + SpatialCrop + np.squeeze, get_surface_distance),
ConfusionMatrixMetric (get_confusion_matrix), compute_confusion_matrix_metric, check_confusion_matrix_metric_name,
do_metric_reduction and MetricReduction -- as published, over scipy's real binary_erosion / distance_transform_edt.
Whatever this restatement gives in the degenerate cases (a union of one voxel squeezed to a 0-d array, one-voxel-thick
slabs and lines) is the contract.  Masks are stored as packed bits; the archive holds arrays only.
"""
import enum
import itertools
import os
import sys
import warnings

import numpy as np
import torch
from scipy.ndimage import binary_erosion, distance_transform_edt

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import refshim  # noqa: E402

refshim.install()
OUT = os.path.dirname(os.path.abspath(__file__))


# ---- MONAI 0.6.0 restatements ---------------------------------------------------------------------------------------
class MetricReduction(enum.Enum):
    NONE = "none"
    MEAN = "mean"
    SUM = "sum"
    MEAN_BATCH = "mean_batch"
    SUM_BATCH = "sum_batch"
    MEAN_CHANNEL = "mean_channel"
    SUM_CHANNEL = "sum_channel"


def do_metric_reduction(f, reduction=MetricReduction.MEAN):
    nans = torch.isnan(f)
    not_nans = (~nans).float()
    if MetricReduction(reduction) != MetricReduction.NONE:
        raise NotImplementedError("only MetricReduction.NONE is restated (the reference uses nothing else)")
    return f, not_nans


def ignore_background(y_pred, y):
    y = y[:, 1:] if y.shape[1] > 1 else y
    y_pred = y_pred[:, 1:] if y_pred.shape[1] > 1 else y_pred
    return y_pred, y


def compute_meandice(y_pred, y, include_background=True):
    if not include_background:
        y_pred, y = ignore_background(y_pred=y_pred, y=y)
    y = y.float()
    y_pred = y_pred.float()
    if y.shape != y_pred.shape:
        raise ValueError("y_pred and y should have same shapes.")
    reduce_axis = list(range(2, len(y_pred.shape)))
    intersection = torch.sum(y * y_pred, dim=reduce_axis)
    y_o = torch.sum(y, reduce_axis)
    y_pred_o = torch.sum(y_pred, dim=reduce_axis)
    denominator = y_o + y_pred_o
    return torch.where(y_o > 0, (2.0 * intersection) / denominator, torch.tensor(float("nan"), device=y_o.device))


def generate_spatial_bounding_box(img, select_fn=lambda x: x > 0, channel_indices=None, margin=0):
    data = img[list(channel_indices)] if channel_indices is not None else img
    data = np.any(select_fn(data), axis=0)
    ndim = len(data.shape)
    margin = (margin,) * ndim
    box_start, box_end = [0] * ndim, [0] * ndim
    for di, ax in enumerate(itertools.combinations(reversed(range(ndim)), ndim - 1)):
        dt = data.any(axis=ax)
        if not np.any(dt):
            return [0] * ndim, [0] * ndim
        min_d = max(np.argmax(dt) - margin[di], 0)
        max_d = max(data.shape[di] - max(np.argmax(dt[::-1]) - margin[di], 0), min_d + 1)
        box_start[di], box_end[di] = min_d, max_d
    return box_start, box_end


def spatial_crop(img, roi_start, roi_end):  # SpatialCrop(roi_start, roi_end)(img) on a channel-first array
    return img[(slice(None),) + tuple(slice(s, e) for s, e in zip(roi_start, roi_end))]


def get_mask_edges(seg_pred, seg_gt, label_idx=1, crop=True):
    if isinstance(seg_pred, torch.Tensor):
        seg_pred = seg_pred.detach().cpu().numpy()
    if isinstance(seg_gt, torch.Tensor):
        seg_gt = seg_gt.detach().cpu().numpy()
    if seg_pred.shape != seg_gt.shape:
        raise ValueError("seg_pred and seg_gt should have same shapes.")
    if seg_pred.dtype != bool:
        seg_pred = seg_pred == label_idx
    if seg_gt.dtype != bool:
        seg_gt = seg_gt == label_idx
    if crop:
        if not np.any(seg_pred | seg_gt):
            return np.zeros_like(seg_pred), np.zeros_like(seg_gt)
        seg_pred, seg_gt = np.expand_dims(seg_pred, 0), np.expand_dims(seg_gt, 0)
        box_start, box_end = generate_spatial_bounding_box(np.asarray(seg_pred | seg_gt))
        seg_pred = np.squeeze(spatial_crop(seg_pred, box_start, box_end))
        seg_gt = np.squeeze(spatial_crop(seg_gt, box_start, box_end))
    edges_pred = binary_erosion(seg_pred) ^ seg_pred
    edges_gt = binary_erosion(seg_gt) ^ seg_gt
    return edges_pred, edges_gt


def get_surface_distance(seg_pred, seg_gt, distance_metric="euclidean"):
    if not np.any(seg_gt):
        dis = np.inf * np.ones_like(seg_gt)
    else:
        if not np.any(seg_pred):
            dis = np.inf * np.ones_like(seg_gt)
            return np.asarray(dis[seg_gt])
        if distance_metric != "euclidean":
            raise NotImplementedError("only the euclidean distance is restated (the reference uses nothing else)")
        dis = distance_transform_edt(~seg_gt)
    return np.asarray(dis[seg_pred])


def compute_percent_hausdorff_distance(edges_pred, edges_gt, distance_metric="euclidean", percentile=None):
    surface_distance = get_surface_distance(edges_pred, edges_gt, distance_metric=distance_metric)
    if surface_distance.shape == (0,):
        return np.nan
    if not percentile:
        return surface_distance.max()
    if 0 <= percentile <= 100:
        return np.percentile(surface_distance, percentile)
    raise ValueError(f"percentile should be a value between 0 and 100, get {percentile}.")


def compute_hausdorff_distance(y_pred, y, include_background=False, distance_metric="euclidean", percentile=None,
                               directed=False):
    if not include_background:
        y_pred, y = ignore_background(y_pred=y_pred, y=y)
    y, y_pred = y.float(), y_pred.float()
    if y.shape != y_pred.shape:
        raise ValueError("y_pred and y should have same shapes.")
    batch_size, n_class = y_pred.shape[:2]
    hd = np.empty((batch_size, n_class))
    for b, c in np.ndindex(batch_size, n_class):
        edges_pred, edges_gt = get_mask_edges(y_pred[b, c], y[b, c])
        distance_1 = compute_percent_hausdorff_distance(edges_pred, edges_gt, distance_metric, percentile)
        if directed:
            hd[b, c] = distance_1
        else:
            distance_2 = compute_percent_hausdorff_distance(edges_gt, edges_pred, distance_metric, percentile)
            hd[b, c] = max(distance_1, distance_2)
    return torch.from_numpy(hd)


def get_confusion_matrix(y_pred, y, include_background=True):
    if not include_background:
        y_pred, y = ignore_background(y_pred=y_pred, y=y)
    y, y_pred = y.float(), y_pred.float()
    if y.shape != y_pred.shape:
        raise ValueError("y_pred and y should have same shapes.")
    batch_size, n_class = y_pred.shape[:2]
    y_pred = y_pred.view(batch_size, n_class, -1)
    y = y.view(batch_size, n_class, -1)
    tp = ((y_pred + y) == 2).float()
    tn = ((y_pred + y) == 0).float()
    tp = tp.sum(dim=[2])
    tn = tn.sum(dim=[2])
    p = y.sum(dim=[2])
    n = y.shape[-1] - p
    fn = p - tp
    fp = n - tn
    return torch.stack([tp, fp, tn, fn], dim=-1)


_NAMES = {
    "sensitivity": "tpr", "recall": "tpr", "hit_rate": "tpr", "true_positive_rate": "tpr", "tpr": "tpr",
    "specificity": "tnr", "selectivity": "tnr", "true_negative_rate": "tnr", "tnr": "tnr",
    "precision": "ppv", "positive_predictive_value": "ppv", "ppv": "ppv",
    "negative_predictive_value": "npv", "npv": "npv",
    "miss_rate": "fnr", "false_negative_rate": "fnr", "fnr": "fnr",
    "fall_out": "fpr", "false_positive_rate": "fpr", "fpr": "fpr",
    "false_discovery_rate": "fdr", "fdr": "fdr", "false_omission_rate": "for", "for": "for",
    "prevalence_threshold": "pt", "pt": "pt", "threat_score": "ts", "critical_success_index": "ts", "ts": "ts", "csi": "ts",
    "accuracy": "acc", "acc": "acc", "balanced_accuracy": "ba", "ba": "ba", "f1_score": "f1", "f1": "f1",
    "matthews_correlation_coefficient": "mcc", "mcc": "mcc", "fowlkes_mallows_index": "fm", "fm": "fm",
    "informedness": "bm", "bookmaker_informedness": "bm", "bm": "bm", "markedness": "mk", "deltap": "mk", "mk": "mk",
}


def check_confusion_matrix_metric_name(metric_name):
    metric_name = metric_name.replace(" ", "_").lower()
    if metric_name not in _NAMES:
        raise NotImplementedError("the metric is not implemented.")
    return _NAMES[metric_name]


def compute_confusion_matrix_metric(metric_name, confusion_matrix):
    metric = check_confusion_matrix_metric_name(metric_name)
    if confusion_matrix.ndimension() == 1:
        confusion_matrix = confusion_matrix.unsqueeze(dim=0)
    if confusion_matrix.shape[-1] != 4:
        raise ValueError("the size of the last dimension of confusion_matrix should be 4.")
    tp, fp, tn, fn = (confusion_matrix[..., i] for i in range(4))
    p, n = tp + fn, fp + tn
    nan_tensor = torch.tensor(float("nan"), device=confusion_matrix.device)
    if metric == "tpr":
        numerator, denominator = tp, p
    elif metric == "tnr":
        numerator, denominator = tn, n
    else:
        raise NotImplementedError("only tpr / tnr are restated (the metrics the goldens use)")
    return torch.where(denominator != 0, numerator / denominator, nan_tensor)


class DiceMetric:
    def __init__(self, include_background=True, reduction=MetricReduction.MEAN, get_not_nans=False):
        self.include_background, self.reduction = include_background, reduction

    def __call__(self, y_pred, y):
        return compute_meandice(y_pred, y, self.include_background)


class HausdorffDistanceMetric:
    def __init__(self, include_background=False, distance_metric="euclidean", percentile=None, directed=False,
                 reduction=MetricReduction.MEAN, get_not_nans=False):
        self.include_background, self.distance_metric = include_background, distance_metric
        self.percentile, self.directed = percentile, directed

    def __call__(self, y_pred, y):
        if y_pred.ndimension() < 3:
            raise ValueError("y_pred should have at least three dimensions.")
        return compute_hausdorff_distance(y_pred, y, self.include_background, self.distance_metric, self.percentile,
                                          self.directed)


class ConfusionMatrixMetric:
    def __init__(self, include_background=True, metric_name="hit_rate", compute_sample=False,
                 reduction=MetricReduction.MEAN, get_not_nans=False):
        self.include_background = include_background

    def __call__(self, y_pred, y):
        return get_confusion_matrix(y_pred, y, self.include_background)


class SurfaceDistanceMetric:
    def __init__(self, *a, **k):
        raise NotImplementedError("not restated")


def compute_roc_auc(*a, **k):
    raise NotImplementedError("not restated")


refshim._mod("monai.metrics", DiceMetric=DiceMetric, HausdorffDistanceMetric=HausdorffDistanceMetric,
             ConfusionMatrixMetric=ConfusionMatrixMetric, SurfaceDistanceMetric=SurfaceDistanceMetric,
             compute_roc_auc=compute_roc_auc)
refshim._mod("monai.metrics.confusion_matrix", compute_confusion_matrix_metric=compute_confusion_matrix_metric,
             check_confusion_matrix_metric_name=check_confusion_matrix_metric_name)
refshim._mod("monai.metrics.utils", do_metric_reduction=do_metric_reduction, get_mask_edges=get_mask_edges,
             get_surface_distance=get_surface_distance)
sys.modules["monai.utils"].MetricReduction = MetricReduction
from utils.metrics import get_metric_callable, compute_metric_tensor  # noqa: E402

METRICS = ["dice", "hausdorff_distance95", "sensitivity", "specificity"]


# ---- cases ------------------------------------------------------------------------------------------------------------
def blobs(rng, shape, count, rmax):
    z, y, x = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    m = np.zeros(shape, bool)
    for _ in range(count):
        c = [rng.uniform(0, s) for s in shape]
        r = rng.uniform(1.0, rmax)
        m |= (z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2 <= r * r
    return m


def cases():
    rng = np.random.default_rng(20211016)
    S = (18, 20, 24)
    out = {}
    for n in (1, 2):
        p = np.stack([np.stack([blobs(rng, S, 3, 5) for _ in range(3)]) for _ in range(n)])
        t = np.stack([np.stack([blobs(rng, S, 3, 5) for _ in range(3)]) for _ in range(n)])
        out[f"blobs_n{n}"] = (p, t)
    a = np.stack([blobs(rng, S, 4, 6) for _ in range(3)])[None]
    out["identical"] = (a, a.copy())
    e = np.zeros((1, 3) + S, bool)
    p, t = e.copy(), e.copy()
    t[0, 0] = blobs(rng, S, 2, 5)          # empty prediction
    p[0, 1] = blobs(rng, S, 2, 5)          # empty target; channel 2: both empty
    out["empty"] = (p, t)
    p, t = e.copy(), e.copy()
    p[0, 0, 3, 4, 5] = True; t[0, 0, 10, 15, 2] = True      # one voxel each
    p[0, 1, 7, 7, 7] = True; t[0, 1, 7, 7, 7] = True        # union of a single voxel: 0-d after the squeeze
    p[0, 2, 0, 0, 0] = True; t[0, 2, 0, 0, 1] = True        # two adjacent voxels: a 1-D box of length 2
    out["voxels"] = (p, t)
    p, t = e.copy(), e.copy()
    p[0, 0, 5, 2:15, 3:20] = True; t[0, 0, 5, 4:18, 1:12] = True        # slab one voxel thick along D
    p[0, 1, 2:16, 9, 3:20] = True; t[0, 1, 6:12, 9, 8:10] = True        # ... along H
    p[0, 2, 1:17, 2:19, 23] = True; p[0, 2, 6:9, 8:12, 23] = False; t[0, 2, 4:10, 5:7, 23] = True  # along W, at the border
    out["slabs"] = (p, t)
    p, t = e.copy(), e.copy()
    p[0, 0, 2:17, 4, 6] = True; t[0, 0, 5:9, 4, 6] = True; t[0, 0, 12, 4, 6] = True   # lines along D with a gap
    p[0, 1, 3, 1:19, 0] = True; t[0, 1, 3, 8:11, 0] = True                              # along H at a border
    p[0, 2, 17, 19, 0:24] = True; t[0, 2, 17, 19, 5] = True                             # along W in the far corner
    out["lines"] = (p, t)
    p, t = e.copy(), e.copy()
    p[0, 0, :6, :, :] = True; t[0, 0, :9, :, :] = True                   # slabs filling whole planes
    p[0, 1, :, :, :] = True; t[0, 1, 4:14, 5:15, 6:18] = True            # the full volume
    p[0, 2] = blobs(rng, S, 5, 7); t[0, 2, :, :3, :] = True; t[0, 2, -2:, :, -4:] = True
    out["border"] = (p, t)
    p, t = e.copy(), e.copy()
    p[0, 0, 3:15, 3:15, 3:15] = True; t[0, 0, 5:13, 5:13, 5:13] = True   # nested cubes: many equal distances
    p[0, 1, 2:16, 2:18, 2:22] = True; t[0, 1, 2:16, 2:18, 2:22] = True
    t[0, 1, 8, 9, 10] = False                                           # a one-voxel hole
    g = (np.indices(S).sum(0) % 4 == 0)
    p[0, 2] = g; t[0, 2] = np.roll(g, 1, axis=2)                        # lattice: all distances 1
    out["ties"] = (p, t)
    sp = rng.random((2, 3) + S) < 0.01
    p, t = np.stack([np.stack([blobs(rng, S, 2, 6) for _ in range(3)]) for _ in range(2)]), sp
    p = p | (rng.random(p.shape) < 0.005)
    out["speckle_n2"] = (p, t)
    return out


def raw_variants(p, t):
    fp, ft = torch.from_numpy(p.astype(np.float32)), torch.from_numpy(t.astype(np.float32))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return {
            "raw_p95": compute_hausdorff_distance(fp, ft, True, percentile=95).numpy(),
            "raw_max": compute_hausdorff_distance(fp, ft, True, percentile=None).numpy(),
            "raw_p95_directed": compute_hausdorff_distance(fp, ft, True, percentile=95, directed=True).numpy(),
            "raw_max_directed_nobg": compute_hausdorff_distance(fp, ft, False, percentile=None, directed=True).numpy(),
            "raw_p50_nobg": compute_hausdorff_distance(fp, ft, False, percentile=50).numpy(),
        }


def main():
    arrays = {}
    names = []
    callables = get_metric_callable(METRICS, include_background=True)
    for name, (p, t) in cases().items():
        names.append(name)
        arrays[f"{name}__shape"] = np.array(p.shape, np.int64)
        arrays[f"{name}__pred"] = np.packbits(p.astype(bool).ravel())
        arrays[f"{name}__target"] = np.packbits(t.astype(bool).ravel())
        fp, ft = torch.from_numpy(p.astype(np.float32)), torch.from_numpy(t.astype(np.float32))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            res, cm = compute_metric_tensor(fp, ft, callables)
        for k, v in res.items():
            arrays[f"{name}__{k}"] = np.asarray(v)
        arrays[f"{name}__confusion"] = np.asarray(cm)
        for k, v in raw_variants(p, t).items():
            arrays[f"{name}__{k}"] = v
        print(name, {k: np.round(np.asarray(v), 3).tolist() for k, v in res.items()})
    arrays["cases"] = np.array(names)
    path = os.path.join(OUT, "metrics.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
