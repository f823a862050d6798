"""scipy-free restatement of the reference's distance-map criteria (learning/losses.py:43-467, utils/transforms.py:95-122)
in numpy / torch, for the parity tests of csrc/edt.hip and csrc/dist_loss.hip.  Distances are brute force: the squared
distance of a voxel is the minimum over ALL background voxels of the integer squared coordinate difference -- no separable
passes, no envelopes, nothing shared with the kernels.  sqrt is taken in float64 and cast to float32 once, which is what
scipy.ndimage.distance_transform_edt (f64) cast to f32 gives.  Losses are evaluated in the dtype asked for (float64 for the
parity bars); the arg-max one-hot of the prediction is always taken on torch.sigmoid of the FLOAT32 logits, because that is
the discrete decision the reference takes (it runs in f32) and it is not a matter of precision.

tests/test_distance_losses_cpu.py pins every function here to tests/golden/losses*.npz (the reference's own classes over
real scipy), the fields bit for bit.  Tensors may live on any device: the GPU tests run the brute force on the GPU."""
import torch


def sq_dist_to_background(mask, chunk=256):
    """mask: bool [D, H, W] -> int64 [D, H, W], squared Euclidean distance to the nearest False voxel (0 on background).
    No background at all: the distance to a virtual background voxel at index (-1, 0, 0) -- what scipy 1.15 returns."""
    mask = mask.bool()
    dev = mask.device
    shape = mask.shape
    coords = torch.stack(torch.meshgrid(*[torch.arange(s, device=dev) for s in shape], indexing="ij"), -1).reshape(-1, 3)
    flat = mask.reshape(-1)
    bg = coords[~flat]
    if bg.numel() == 0:
        bg = torch.tensor([[-1, 0, 0]], device=dev)
    fg = coords[flat]
    out = torch.zeros(flat.numel(), dtype=torch.int64, device=dev)
    res = torch.empty(fg.shape[0], dtype=torch.int64, device=dev)
    rows = max(1, (chunk * 32768) // max(1, bg.shape[0]))
    for i in range(0, fg.shape[0], rows):
        d = fg[i:i + rows, None, :] - bg[None, :, :]
        res[i:i + rows] = (d * d).sum(-1).min(1).values
    out[flat] = res
    return out.reshape(shape)


def edt(mask):
    """scipy.ndimage.distance_transform_edt(mask) as float64."""
    return sq_dist_to_background(mask).double().sqrt()


def hd_dist(seg, integer=False):
    """one_hot2hd_dist (learning/losses.py:77-95) of seg [K, D, H, W] -> float32.  The function writes scipy's f64 field into
    np.zeros_like(seg): a float32 seg (the target) rounds it to f32, an INTEGER seg truncates it -- and the prediction's
    one-hot is int32 (class2one_hot, :37), so HausdorffLoss's predicted field is floor(distance) (integer=True)."""
    out = torch.zeros(seg.shape, dtype=torch.float32, device=seg.device)
    for k in range(seg.shape[0]):
        pos = seg[k] != 0
        if pos.any():
            out[k] = (edt(pos).floor() if integer else edt(pos)).float()
    return out


def one_hot_to_dist(seg):
    """one_hot2dist / OneHotToDist (learning/losses.py:59-74, utils/transforms.py:95-122) of seg [K, D, H, W] -> float32."""
    out = torch.zeros(seg.shape, dtype=torch.float32, device=seg.device)
    for k in range(seg.shape[0]):
        pos = seg[k] != 0
        if pos.any():
            neg = ~pos
            out[k] = (edt(neg) * neg.double() - (edt(pos) - 1.0) * pos.double()).float()
    return out


def batched(fn, x):
    """fn over every sample of [N, K, D, H, W]."""
    return torch.stack([fn(x[n]) for n in range(x.shape[0])])


def probs_one_hot(logits):
    """probs2one_hot(torch.sigmoid(logits)) (learning/losses.py:43-56): arg-max over the channels of the f32 probabilities,
    the first (lowest) channel on ties."""
    p = torch.sigmoid(logits.float())
    return torch.zeros_like(p).scatter_(1, p.argmax(dim=1, keepdim=True), 1.0)


def hd_loss(logits, target, alpha=2.0, tdm=None):
    p = torch.sigmoid(logits)
    t = target.to(logits.dtype)
    if tdm is None:
        tdm = batched(hd_dist, target)
    pdm = batched(lambda s: hd_dist(s, integer=True), probs_one_hot(logits.detach()))
    w = tdm.to(logits.dtype) ** alpha + pdm.to(logits.dtype) ** alpha
    return ((p - t) ** 2 * w).mean()


def boundary_loss(logits, dist):
    return (torch.sigmoid(logits) * dist.to(logits.dtype)).mean()


def dice_loss(logits, target, batch=False, jaccard=False, smooth_nr=1e-5, smooth_dr=1e-5):
    """monai 0.6 DiceLoss(include_background, sigmoid, squared_pred, reduction mean)."""
    p = torch.sigmoid(logits)
    t = target.to(logits.dtype)
    axes = [0, 2, 3, 4] if batch else [2, 3, 4]
    inter = (t * p).sum(axes)
    den = (t * t).sum(axes) + (p * p).sum(axes)
    if jaccard:
        den = 2.0 * (den - inter)
    return (1.0 - (2.0 * inter + smooth_nr) / (den + smooth_dr)).mean()


def criterion_loss(name, logits, target, dist=None, tdm=None):
    """The criterion make_criterion(name) of src/definer.py:246-282 on one head."""
    if name == "hd":
        return hd_loss(logits, target, 2.0, tdm)
    if name == "dice_hd":
        return dice_loss(logits, target) + hd_loss(logits, target, 2.0, tdm)
    if name == "boundary":
        return boundary_loss(logits, dist)
    if name == "dice_boundary":
        return dice_loss(logits, target) + boundary_loss(logits, dist)
    raise KeyError(name)


def loss_and_grads(name, heads, target, dist=None, dtype=torch.float64):
    """mean over heads of the criterion (learning/engine.py:322-330) evaluated in `dtype` -> (value, [d value / d head])."""
    xs = [h.detach().to(dtype).requires_grad_(True) for h in heads]
    tdm = batched(hd_dist, target) if "hd" in name else None
    loss = torch.stack([criterion_loss(name, x, target, dist, tdm) for x in xs]).mean()
    loss.backward()
    return loss.detach(), [x.grad for x in xs]
