"""Post-forward chain of the reference's ``Engine.evaluate`` (learning/engine.py:205-285) kept on the GPU.

The reference pads the volume to a multiple of 8, runs every model x TTA pass, copies each output to the CPU,
averages sigmoid outputs there, thresholds, copies back, removes background voxels, converts to BraTS labels
and crops.  Here every step is a HIP kernel on device buffers (csrc/post.hip, csrc/infer.hip); only the final
label map / metric scalars leave the GPU.

Function names and argument meaning follow utils/transforms.py (shape_to_divisible :482, shape_to_original :515,
remove_background_voxels :536) so Engine.evaluate can import them unchanged.

The reference's optional label post-processing (--cleaning_areas / --replace_value, src/definer.py:679-694) is here too:
KeepLargestConnectedComponent and ReplaceWithClosestValue (utils/transforms.py:209-268) run as HIP kernels
(csrc/postproc.hip), and get_post_transforms / Evaluator(cleaning_areas_threshold=, replace_value_threshold=) chain them
like the reference does.  Where the GPU form differs from the reference:
  1. ReplaceWithClosestValue: of several pixels of DIFFERENT values at the same nearest distance, the reference's pick
     depends on scipy's KD-tree; here the one first in the slice's row-major order wins (deterministic).
  2. KeepLargestConnectedComponent(None) on a map without foreground returns it unchanged (the reference raises ValueError).
  3. Both always return a float32 tensor on the input's device (the reference returns a uint8 numpy array when it replaced
     something).
  4. A volume without a single background voxel is outside the contract (the reference assumes label 0 exists).

The reference's ensemble fusion by STAPLE (--perform_staple / --staple_threshold, learning/engine.py:244-247) is here as well:
perform_staple_on_brats_multi_channel (utils/transforms.py:650-687) and Evaluator(perform_staple=True, staple_threshold=) run
ops.staple (csrc/staple.hip) on bit-packed rater decisions.  The reference calls SimpleITK's STAPLEImageFilter; SimpleITK is not
available to this project's tests, so the kernels implement ITK's STAPLEImageFilter::GenerateData as RESTATED in DESIGN.md
section 6 and are tested against a numpy restatement of the same text (tests/_staple_ref.py): nothing executable pins the ITK
boundary.  The fused maps are float32 0 / 1 on the input's device (the reference returns a bool tensor on the CPU), and any
batch size works (the reference: batch 1).
"""
import numbers

import numpy as np
import torch

from . import _lib, ops
from ._tensors import _vec
from .inferers import GraphedPredictor, _first, sliding_window_inference
from .transforms import convert_to_multichannel


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _need_cuda(t, what):
    if not t.is_cuda:
        raise _lib.BratsHipError(f"brats21_amd.evaluate.{what} runs on the GPU only (no CPU fallback)")


def _pad_crop(data, out_spatial, offset, fill=0.0):
    x = data.contiguous().float()
    lead = tuple(x.shape[:-3])
    planes = int(np.prod(lead)) if lead else 1
    out = torch.empty(lead + tuple(int(v) for v in out_spatial), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().brats_pad_crop(x.data_ptr(), out.data_ptr(), planes, *x.shape[-3:], *out.shape[-3:],
                                         *[int(o) for o in offset], float(fill), _stream()), "pad_crop")
    return out


def shape_to_divisible(data, k=16, min_shape=None):
    """utils/transforms.py:482-512 -> (padded, p_b, p_a); the odd voxel of an odd padding goes in front."""
    assert k > 0, "k need to positive"
    if data.dim() not in (4, 5):
        raise ValueError("Tensor dimension is incorrect")
    _need_cuda(data, "shape_to_divisible")
    shape = np.array(data.shape[-3:])
    tgt = np.ceil(shape / k).astype(int) * k
    if min_shape is not None:
        tgt[tgt < min_shape] = min_shape
    p = tgt - shape
    p_b, p_a = np.ceil(p / 2).astype(int), np.floor(p / 2).astype(int)
    return _pad_crop(data, tgt, p_b), p_b, p_a


def shape_to_original(data, p_b, p_a):
    """utils/transforms.py:515-533."""
    if data.dim() not in (4, 5):
        raise ValueError("Tensor dimension is incorrect")
    _need_cuda(data, "shape_to_original")
    shape = np.array(data.shape[-3:])
    return _pad_crop(data, shape - np.asarray(p_a) - np.asarray(p_b), -np.asarray(p_b))


def finalize_segmentation(prob_sum, passes=1, img=None, thresh=0.5, want_labels=False):
    """mean over passes (learning/engine.py:249) + AsDiscrete(threshold) (src/definer.py:700-703) +
    remove_background_voxels (utils/transforms.py:536-550) [+ BraTS labels, utils/transforms.py:169-206] in
    one pass.  prob_sum: [N, K, D, H, W] sum of probabilities; img: [N, C, D, H, W] or None.
    -> seg f32 0/1 [N, K, D, H, W] (and uint8 labels [N, 1, D, H, W] when want_labels)."""
    _need_cuda(prob_sum, "finalize_segmentation")
    p = prob_sum.contiguous().float()
    n, k = p.shape[:2]
    vox = p[0, 0].numel()
    im = None
    if img is not None:
        im = img.contiguous().float()
        if im.shape[0] != n or tuple(im.shape[2:]) != tuple(p.shape[2:]):
            raise ValueError(f"image {tuple(im.shape)} does not match predictions {tuple(p.shape)}")
    seg = torch.empty_like(p)
    labels = torch.empty((n, 1) + tuple(p.shape[2:]), dtype=torch.uint8, device=p.device) if want_labels else None
    _lib.check(_lib.lib().brats_post_threshold(p.data_ptr(), _vec(im, None, "finalize_segmentation: image", p, null=True),
                                               seg.data_ptr(),
                                               labels.data_ptr() if labels is not None else None, n, k,
                                               im.shape[1] if im is not None else 0, vox, 1.0 / passes, float(thresh),
                                               _stream()), "post_threshold")
    return (seg, labels) if want_labels else seg


def remove_background_voxels(img, outputs):
    """utils/transforms.py:536-550 (outputs are the thresholded 0/1 maps, as in Engine.evaluate)."""
    return finalize_segmentation(outputs, 1, img, thresh=0.5)


def to_brats_labels(seg):
    """ConvertToBratsClassesBasedOnMultiChannel + ChangeLabel3To4 (utils/transforms.py:169-206), batched."""
    return finalize_segmentation(seg, 1, None, thresh=0.5, want_labels=True)[1]


def overlap_counts(pred, target):
    """uint64-exact {|P&T|, |P|, |T|} per (n, k) -> int64 tensor [N, K, 3] (device)."""
    _need_cuda(pred, "overlap_counts")
    p, t = pred.contiguous().float(), target.contiguous().float()
    if p.shape != t.shape:
        raise ValueError(f"prediction {tuple(p.shape)} and target {tuple(t.shape)} differ")
    n, k = p.shape[:2]
    counts = torch.empty((n, k, 3), dtype=torch.int64, device=p.device)
    _lib.check(_lib.lib().brats_overlap_counts(p.data_ptr(), _vec(t, p.numel(), "overlap_counts: target", p), counts.data_ptr(),
                                               n * k, p[0, 0].numel(),
                                               _stream()), "overlap_counts")
    return counts


def hard_dice_metric(pred, target):
    """Dice per (n, k) with the empty-label conventions of utils/metrics.py:47-67 (both empty -> 1, exactly
    one empty -> 0)."""
    c = overlap_counts(pred, target).double()
    inter, ps, ts = c[..., 0], c[..., 1], c[..., 2]
    dice = 2 * inter / (ps + ts).clamp_min(1)
    dice = torch.where((ps == 0) & (ts == 0), torch.ones_like(dice), dice)
    return dice.float()


_INT_MAX = 2 ** 31 - 1


def _check_int(value, what, allow_none=False):
    if value is None and allow_none:
        return
    if isinstance(value, bool) or not isinstance(value, numbers.Integral):
        raise TypeError(f"{what} must be an int{' or None' if allow_none else ''}, got {value!r}")


def _clean_labels_(lab, threshold):
    """In place on uint8 [N, D, H, W] (cuda, contiguous): keep the 26-connected components of more than `threshold`
    voxels, or only the largest one when threshold is None."""
    n, d, h, w = lab.shape
    ws = torch.empty(_lib.lib().brats_cc_ws_bytes(n, d, h, w), dtype=torch.uint8, device=lab.device)
    min_size = -1 if threshold is None else min(max(int(threshold), 0), _INT_MAX)
    _lib.check(_lib.lib().brats_cc_filter(lab.data_ptr(), n, d, h, w, min_size, ws.data_ptr(), _stream()), "cc_filter")


def _replace_rare_labels_(lab, threshold, axis):
    """In place on uint8 [N, D, H, W] (cuda, contiguous): values with at most `threshold` voxels take the nearest
    non-rare value of their slice along `axis`."""
    n, d, h, w = lab.shape
    ws = torch.empty(_lib.lib().brats_rare_fill_ws_bytes(n, d, h, w), dtype=torch.uint8, device=lab.device)
    max_count = min(max(int(threshold), -1), _INT_MAX)
    _lib.check(_lib.lib().brats_rare_fill(lab.data_ptr(), n, d, h, w, int(axis), max_count, ws.data_ptr(), _stream()),
               "rare_fill")


def _on_label_map(data, fn):
    """[1, 1, D, H, W] / [N, 1, D, H, W] / [D, H, W] label map (float or uint8, CPU or CUDA) -> fn(uint8 [N, D, H, W] copy
    on the GPU) -> float32 in the input's shape on the input's device."""
    if not torch.is_tensor(data):
        raise TypeError(f"expected a torch.Tensor label map, got {type(data).__name__}")
    if not (data.dim() == 3 or (data.dim() == 5 and data.shape[1] == 1)):
        raise ValueError(f"label map must be [N, 1, D, H, W] or [D, H, W], got {tuple(data.shape)}")
    x = data if data.is_cuda else data.to(torch.device("cuda", torch.cuda.current_device()))
    with torch.cuda.device(x.device):
        lab = x.reshape((-1,) + tuple(x.shape[-3:])).to(torch.uint8, copy=True).contiguous()
        fn(lab)
        out = lab.float().reshape(data.shape)
    return out if data.is_cuda else out.to(data.device)


class KeepLargestConnectedComponent:
    """utils/transforms.py:209-230 (get_largest_component, :579-600) on the GPU, per sample: the 26-connected components
    of labels != 0 with more than `threshold` voxels are kept (threshold <= 0 keeps all), or only the largest one when
    threshold is None (ties: the component whose first voxel comes first in C order); kept voxels keep their value.
    Differs from the reference only where the module docstring says (items 2-4)."""

    def __init__(self, threshold=None):
        _check_int(threshold, "threshold", allow_none=True)
        self.threshold = threshold

    def __call__(self, data):
        return _on_label_map(data, lambda lab: _clean_labels_(lab, self.threshold))


class ReplaceWithClosestValue:
    """utils/transforms.py:233-268 (replace_w_closest_value_3d, :603-647) on the GPU, per sample: values occurring at most
    `thresh` times (0 included) are rare; if a non-zero value is rare, every rare pixel of each slice along `axis`
    (2 = W: the (D, H) planes) takes the value of the nearest non-rare pixel of that slice (exact Euclidean distance),
    or 0 where the slice has none.  `labels` is accepted and ignored, as by the reference.  Ties between different values
    at the same distance: the pixel first in the slice's row-major order (module docstring, item 1)."""

    def __init__(self, labels=None, thresh=20, axis=2):
        _check_int(thresh, "thresh")
        if isinstance(axis, bool) or not isinstance(axis, numbers.Integral) or not 0 <= axis <= 2:
            raise ValueError(f"axis must be 0, 1 or 2, got {axis!r}")
        self.labels, self.thresh, self.axis = labels, thresh, int(axis)

    def __call__(self, data):
        return _on_label_map(data, lambda lab: _replace_rare_labels_(lab, self.thresh, self.axis))


def _post_chain(prob, passes, thresh, cleaning_threshold=None, clean=False, replace_threshold=None, replace=False):
    """get_post_transforms (src/definer.py:679-694) on [N, 3, D, H, W] probability sums (cuda): mean over `passes` ->
    AsDiscrete(>= thresh) -> BraTS labels -> [KeepLargestConnectedComponent] -> [ReplaceWithClosestValue(axis=2)] ->
    TC / WT / ET channels, f32 0/1.  Without either step it is the threshold alone.  No background removal: Engine.evaluate
    applies it after this chain (learning/engine.py:259), so cleaning sees the predictions on zero-image voxels too."""
    if not (clean or replace):
        return finalize_segmentation(prob, passes, None, thresh)
    _, labels = finalize_segmentation(prob, passes, None, thresh, want_labels=True)
    lab = labels[:, 0]
    if clean:
        _clean_labels_(lab, cleaning_threshold)
    if replace:
        _replace_rare_labels_(lab, replace_threshold, 2)
    return convert_to_multichannel(labels.float(), order="monai")


def get_post_transforms(args):
    """Drop-in for src/definer.py:671-698 (same attributes, same hasattr defaults): returns a callable mapping the mean
    probability [N, 3, D, H, W] (CPU or CUDA) to 0/1 float32 TC / WT / ET maps on the input's device.  The work runs on
    the GPU; a CPU input is copied there and back."""
    thresh = 0.5 if not hasattr(args, "logit_threshold") else args.logit_threshold
    clean = hasattr(args, "cleaning_areas") and args.cleaning_areas
    replace = hasattr(args, "replace_value") and args.replace_value
    kw = {}
    if clean:
        _check_int(args.cleaning_areas_threshold, "cleaning_areas_threshold", allow_none=True)
        kw.update(clean=True, cleaning_threshold=args.cleaning_areas_threshold)
    if replace:
        _check_int(args.replace_value_threshold, "replace_value_threshold")
        kw.update(replace=True, replace_threshold=args.replace_value_threshold)

    def post(mean):
        x = mean if mean.is_cuda else mean.to(torch.device("cuda", torch.cuda.current_device()))
        with torch.cuda.device(x.device):
            out = _post_chain(x, 1, float(thresh), **kw)
        return out if mean.is_cuda else out.to(mean.device)
    return post


def perform_staple_on_brats_multi_channel(datas, threshold_value=0.5, return_as_tensor=True):
    """utils/transforms.py:650-687 on the GPU: datas = the raters' thresholded TC / WT / ET maps, a sequence of [N, 3, D, H, W]
    0 / 1 tensors (or numpy arrays); every (sample, channel) is fused by STAPLE on its own (ops.staple; 10000 iterations at
    most, foreground value 1, as the reference sets them) and the weights are binarised with > threshold_value.
    -> float32 0 / 1 [N, 3, D, H, W] on the device of the inputs (CPU inputs are copied to the GPU and back), or a numpy array
    when not return_as_tensor."""
    ops._staple_check_threshold(threshold_value, "threshold_value")
    datas = [torch.from_numpy(np.ascontiguousarray(d)) if isinstance(d, np.ndarray) else d for d in datas]
    if not 1 <= len(datas) <= ops.STAPLE_MAX_RATERS:
        raise ValueError(f"perform_staple_on_brats_multi_channel: {len(datas)} raters (1 .. {ops.STAPLE_MAX_RATERS} supported)")
    for d in datas:
        if not torch.is_tensor(d):
            raise TypeError(f"perform_staple_on_brats_multi_channel: expected tensors or arrays, got {type(d).__name__}")
        if d.dim() != 5 or tuple(d.shape) != tuple(datas[0].shape) or d.device != datas[0].device:
            raise ValueError(f"perform_staple_on_brats_multi_channel: every rater must be [N, C, D, H, W] of one shape on one "
                             f"device, got {tuple(datas[0].shape)} on {datas[0].device} and {tuple(d.shape)} on {d.device}")
    src = datas[0].device
    if src.type != "cuda" and not torch.cuda.is_available():
        raise _lib.BratsHipError("brats21_amd.evaluate.perform_staple_on_brats_multi_channel runs on the GPU only (no CPU fallback)")
    dev = src if src.type == "cuda" else torch.device("cuda", torch.cuda.current_device())
    packer = ops.StaplePacker(datas[0].shape, len(datas), dev)
    for d in datas:  # one rater at a time: a CPU ensemble is never on the GPU as a whole
        packer.add(d.to(dev))
    seg = ops.staple(packer, float(threshold_value))[0]
    seg = seg if src.type == "cuda" else seg.to(src)
    return seg if return_as_tensor else seg.cpu().numpy()


class Evaluator:
    """The per-case body of Engine.evaluate (learning/engine.py:205-285) for one or several models:
    pad to k -> [TTA x] (sliding window | whole volume) -> on-GPU mean of sigmoid -> threshold ->
    background removal -> (labels) -> crop.

    This is the three-channel BraTS chain: the post-processing reads the channels as TC / WT / ET (labels 1 / 2 / 4, cleaning,
    closest-label replacement), whatever the models could take.  The networks themselves run with 1 to 16 input channels and up to 16 classes;
    for K exclusive classes (an ordinary label map, one class per voxel) pass ``activation="softmax"``; for other label sets use
    inferers.sliding_window_inference / tta_predict on the model and post-process the probabilities yourself.

    ``activation="softmax"`` (2 <= K <= 16 classes): ``probability_sum`` sums softmax probabilities over models x TTA passes
    (ops.softmax_planes), the result is ``out["labels"]`` -- uint8 [N, 1, D, H, W], the arg-max of the sum, ties to the lowest
    class, 0 on voxels where every image channel is 0 (ops.argmax_labels) -- and ``out["seg"]`` is its one-hot as float
    [N, K, ...], so that ``dice`` and ``metrics`` are per-class values (the target is then the one-hot of the label map).
    ``thresh``, cleaning, replacement and STAPLE are operations on the BraTS regions: with "softmax" they raise
    NotImplementedError here.

    ``use_graph`` (default: only with a sliding window, whose patch shape is fixed): the patch step of each model is
    captured into a hipGraph once and replayed; the graphs follow the models' weights (GraphedPredictor re-captures when
    a parameter's address / version or ops' packed-weight generation changed).  Whole-volume evaluation
    (sliding_window_size=None, the reference's default path) sees a different padded shape for almost every case, so
    it runs eagerly unless use_graph=True is passed explicitly (then at most ``max_graphs`` shapes stay captured).

    ``cleaning_areas_threshold`` / ``replace_value_threshold`` (default None = off) are the reference's
    ``--cleaning_areas --cleaning_areas_threshold T`` / ``--replace_value --replace_value_threshold T``: with either set,
    the chain is threshold -> labels -> KeepLargestConnectedComponent(T) -> ReplaceWithClosestValue(T, axis=2) ->
    channels -> background removal -> Dice / labels / crop, in the reference's order (get_post_transforms runs before
    remove_background_voxels, learning/engine.py:244-259).

    ``metrics`` (default None: only ``dice``, as before) is a tuple of names of brats21_amd.metrics.METRICS (the
    reference's ``--key_metric`` / ``--additional_metrics``): with a target, ``out`` also holds ``hausdorff_distance95`` /
    ``sensitivity`` / ``specificity`` as device float32 [N, K], computed like ``dice`` on the padded segmentation and
    target after background removal and before cropping (learning/engine.py:259-268).

    ``perform_staple`` / ``staple_threshold`` (default off) are the reference's ``--perform_staple --staple_threshold T``
    (learning/engine.py:244-247): instead of the mean, every model x TTA pass is a rater -- its own sigmoid goes through the post
    chain (threshold, and the per-rater cleaning / replacement when those are set: the reference's apply_f(outputs,
    post_trans)), the 0 / 1 result is packed to one bit per voxel (ops.StaplePacker), and ops.staple fuses the raters per
    channel; W > staple_threshold replaces the thresholded mean, everything after it (background removal, metrics, labels,
    crop) is unchanged.  At most 256 raters.  The only host read is STAPLE's done flag; ``out["staple"]`` holds ops.staple's
    info (p, q, prior, iterations)."""

    def __init__(self, models, tta_transforms=None, sliding_window_size=None, sw_batch_size=1, overlap=0.25,
                 k_divisible=8, thresh=0.5, amp=True, use_graph=None, max_graphs=4, amp_dtype=torch.bfloat16,
                 cleaning_areas_threshold=None, replace_value_threshold=None, metrics=None, perform_staple=False,
                 staple_threshold=0.5, activation="sigmoid"):
        if activation not in ("sigmoid", "softmax"):
            raise ValueError(f"activation must be 'sigmoid' or 'softmax', got {activation!r}")
        if activation == "softmax" and (thresh != 0.5 or cleaning_areas_threshold is not None or replace_value_threshold is not None
                                        or perform_staple):
            raise NotImplementedError("Evaluator(activation='softmax'): thresh, cleaning, replacement and STAPLE are operations on the "
                                      "BraTS regions; the exclusive-class result is the arg-max")
        self.activation = activation
        _check_int(cleaning_areas_threshold, "cleaning_areas_threshold", allow_none=True)
        _check_int(replace_value_threshold, "replace_value_threshold", allow_none=True)
        if metrics is not None:
            from .metrics import _check_names
            metrics = tuple(m for m in _check_names(metrics) if m != "dice")  # dice is always there with a target
        self.metrics = metrics
        self.clean_t, self.replace_t = cleaning_areas_threshold, replace_value_threshold
        self.models = list(models) if isinstance(models, (list, tuple)) else [models]
        self.tta, self.roi, self.swb, self.overlap = tta_transforms, sliding_window_size, sw_batch_size, overlap
        self.k, self.thresh, self.amp, self.amp_dtype = k_divisible, thresh, amp, amp_dtype
        if use_graph is None:
            use_graph = sliding_window_size is not None
        self.predictors = [GraphedPredictor(self._amp(m), modules=m, max_graphs=max_graphs) if use_graph else self._amp(m)
                           for m in self.models]
        self.perform_staple = bool(perform_staple)
        self.staple_threshold = ops._staple_check_threshold(staple_threshold, "staple_threshold")
        if self.perform_staple:
            self.raters = len(self.models) * (1 if tta_transforms is None else sum(1 for _ in tta_transforms))
            if not 1 <= self.raters <= ops.STAPLE_MAX_RATERS:
                raise ValueError(f"perform_staple: {len(self.models)} models x TTA passes = {self.raters} raters "
                                 f"(1 .. {ops.STAPLE_MAX_RATERS} supported)")

    def _amp(self, model):
        def run(x):
            with torch.autocast("cuda", dtype=self.amp_dtype, enabled=self.amp):
                return model(x)
        return run

    def _logits(self, predictor, x):
        if self.roi is not None:
            return sliding_window_inference(x, self.roi, self.swb, predictor, overlap=self.overlap)
        return _first(predictor(x)).float()

    @torch.no_grad()
    def probability_sum(self, image):
        """Sum over models x TTA passes of sigmoid(logits) -- softmax(logits) with activation="softmax" -- on the (padded)
        image -> (sum, passes)."""
        act = torch.sigmoid if self.activation == "sigmoid" else ops.softmax_planes
        acc, passes = None, 0
        for model, predictor in zip(self.models, self.predictors):
            model.eval()
            if self.tta is None:
                logits = self._logits(predictor, image)
                acc = act(logits) if acc is None else acc.add_(act(logits))
                passes += 1
                continue
            for t in self.tta:
                logits = self._logits(predictor, t.augment_image(image))
                if acc is None:
                    acc = torch.zeros(t.deaug_perm.out_shape(logits.shape), dtype=torch.float32, device=image.device)
                t.accumulate_probability(logits, acc, self.activation)
                passes += 1
        return acc, passes

    def _post(self, prob, passes):
        return _post_chain(prob, passes, self.thresh, cleaning_threshold=self.clean_t, clean=self.clean_t is not None,
                           replace_threshold=self.replace_t, replace=self.replace_t is not None)

    @torch.no_grad()
    def staple_segmentation(self, image):
        """Every model x TTA pass on the (padded) image as a STAPLE rater (learning/engine.py:229-247) -> (fused 0 / 1 maps,
        ops.staple's info).  Only one pass's probability exists at a time; the raters are kept as bits."""
        packer = None
        for model, predictor in zip(self.models, self.predictors):
            model.eval()
            for t in ([None] if self.tta is None else self.tta):
                if t is None:
                    prob = torch.sigmoid(self._logits(predictor, image))
                else:
                    logits = self._logits(predictor, t.augment_image(image))
                    prob = torch.zeros(t.deaug_perm.out_shape(logits.shape), dtype=torch.float32, device=image.device)
                    t.accumulate_probability(logits, prob)
                mask = self._post(prob, 1)
                if packer is None:
                    packer = ops.StaplePacker(mask.shape, self.raters, mask.device)
                packer.add(mask)
        return ops.staple(packer, self.staple_threshold)

    @torch.no_grad()
    def __call__(self, image, target=None, return_original_shape=True, want_labels=False):
        """image [N, C, D, H, W] (cuda) -> dict(seg, [labels], [dice]); seg is cropped back to the input
        shape when return_original_shape (learning/engine.py:282-285)."""
        _need_cuda(image, "Evaluator")
        padded, p_b, p_a = shape_to_divisible(image, k=self.k)
        out = {}
        if self.activation == "softmax":  # the arg-max of the probability sum needs no division by the passes
            acc = self.probability_sum(padded)[0]
            labels = ops.argmax_labels(acc, padded)
            classes = torch.arange(acc.shape[1], device=labels.device, dtype=torch.uint8).view(1, -1, 1, 1, 1)
            res, want_labels = ((labels == classes).float(), labels), True
        elif self.perform_staple:
            seg, out["staple"] = self.staple_segmentation(padded)
            res = finalize_segmentation(seg, 1, padded, 0.5, want_labels)
        else:
            acc, passes = self.probability_sum(padded)
            if self.clean_t is None and self.replace_t is None:
                res = finalize_segmentation(acc, passes, padded, self.thresh, want_labels)
            else:
                res = finalize_segmentation(self._post(acc, passes), 1, padded, 0.5, want_labels)
        seg, labels = res if want_labels else (res, None)
        if target is not None:
            tp = shape_to_divisible(target, k=self.k)[0]
            out["dice"] = hard_dice_metric(seg, tp)
            if self.metrics:
                from .metrics import brats_metrics
                out.update(brats_metrics(seg, tp, self.metrics))
        if return_original_shape:
            seg = shape_to_original(seg, p_b, p_a)
            if labels is not None:
                labels = shape_to_original(labels.float(), p_b, p_a).to(torch.uint8)
        out["seg"] = seg
        if labels is not None:
            out["labels"] = labels
        return out
