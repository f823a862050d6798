"""Generates tests/golden/losses.npz, losses_grad_hd.npz and losses_grad_boundary.npz from the REFERENCE's own
learning/losses.py (HausdorffLoss, DiceHDLoss, SurfaceLoss, DiceBoundaryLoss, one_hot2hd_dist) and utils/transforms.py
(OneHotToDist) imported under oracle/refshim.py over real scipy, the criteria built by the reference's own make_criterion.

Run here only (the GPU box has no reference checkout):  python tests/golden/make_golden_losses.py
MONAI 0.6.0 is not installed: the three names learning/losses.py imports are restated below -- monai.losses.dice.DiceLoss
(the options DiceHDLoss / DiceBoundaryLoss pass: sigmoid, squared_pred, jaccard, batch, smooth, reduction mean),
monai.networks.one_hot (never reached: to_onehot_y is off) and monai.utils.LossReduction.  src/definer.py imports half of
MONAI, sklearn and ranger21 at module level, so make_criterion is taken out of its source file by name and executed as it
stands against the reference's loss classes.

losses.npz holds the inputs (masks as packed bits, logits), the fields and the loss values; the input gradients live in the
two losses_grad_*.npz files beside it because one archive with all of them would exceed the size limit for a committed
file.  Arrays only.  Every loss case also stores the float64 value of tests/_losses_ref.py (`__f64`), so that the parity bar
of the GPU test -- a multiple of the reference's own f32-CPU error on that case -- is recorded with the case."""
import argparse
import ast
import enum
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import refshim  # noqa: E402

refshim.install()
OUT = os.path.dirname(os.path.abspath(__file__))
CRITERIA = ("hd", "dice_hd", "boundary", "dice_boundary")


# ---- MONAI 0.6.0 restatements ---------------------------------------------------------------------------------------
class LossReduction(enum.Enum):
    NONE = "none"
    MEAN = "mean"
    SUM = "sum"


class DiceLoss(torch.nn.Module):
    def __init__(self, include_background=True, to_onehot_y=False, sigmoid=False, softmax=False, other_act=None,
                 squared_pred=False, jaccard=False, reduction="mean", smooth_nr=1e-5, smooth_dr=1e-5, batch=False):
        super().__init__()
        if not include_background or to_onehot_y or softmax or other_act is not None or LossReduction(reduction) != LossReduction.MEAN:
            raise NotImplementedError("only the options the reference factory sets are restated")
        self.sigmoid, self.squared_pred, self.jaccard, self.batch = sigmoid, squared_pred, jaccard, batch
        self.smooth_nr, self.smooth_dr = float(smooth_nr), float(smooth_dr)

    def forward(self, input, target):
        if self.sigmoid:
            input = torch.sigmoid(input)
        if target.shape != input.shape:
            raise AssertionError(f"ground truth has different shape ({target.shape}) from input ({input.shape})")
        reduce_axis = list(range(2, len(input.shape)))
        if self.batch:
            reduce_axis = [0] + reduce_axis
        intersection = torch.sum(target * input, dim=reduce_axis)
        if self.squared_pred:
            target = torch.pow(target, 2)
            input = torch.pow(input, 2)
        ground_o = torch.sum(target, dim=reduce_axis)
        pred_o = torch.sum(input, dim=reduce_axis)
        denominator = ground_o + pred_o
        if self.jaccard:
            denominator = 2.0 * (denominator - intersection)
        f = 1.0 - (2.0 * intersection + self.smooth_nr) / (denominator + self.smooth_dr)
        return torch.mean(f)


def one_hot(*a, **k):
    raise NotImplementedError("not restated (to_onehot_y is never set)")


refshim._mod("monai.losses.dice", DiceLoss=DiceLoss)
sys.modules["monai.networks"].one_hot = one_hot
sys.modules["monai.utils"].LossReduction = LossReduction
import learning.losses as ref_losses  # noqa: E402
from utils.transforms import OneHotToDist  # noqa: E402
import _losses_ref as R  # noqa: E402


def reference_make_criterion():
    """make_criterion of src/definer.py, compiled from its own source text (see the module docstring)."""
    path = os.path.join(refshim.REFERENCE_ROOT, "src", "definer.py")
    tree = ast.parse(open(path).read())
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "make_criterion")
    fn.returns = None
    ns = {"argparse": argparse, "DiceLoss": DiceLoss}
    for name in ("HausdorffLoss", "DiceHDLoss", "BoundaryLoss", "DiceBoundaryLoss", "DiceCELoss"):
        ns[name] = getattr(ref_losses, name)
    exec(compile(ast.Module(body=[fn], type_ignores=[]), path, "exec"), ns)
    return ns["make_criterion"]


# ---- cases ------------------------------------------------------------------------------------------------------------
def blobs(rng, shape, count, rmax):
    z, y, x = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    m = np.zeros(shape, bool)
    for _ in range(count):
        c = [rng.uniform(0, s) for s in shape]
        r = rng.uniform(1.5, rmax)
        m |= (z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2 <= r * r
    return m


def field_masks(rng, shape):
    """[7, D, H, W]: random sparse, random dense, a solid box, an empty plane, an all-one plane, one voxel, blobs."""
    m = np.zeros((7,) + shape, bool)
    m[0] = rng.random(shape) < 0.04
    m[1] = rng.random(shape) < 0.93
    m[2][tuple(slice(s // 4, s - s // 5) for s in shape)] = True
    m[4] = True
    m[5][tuple(s // 2 for s in shape)] = True
    m[6] = blobs(rng, shape, 3, min(shape) / 2)
    return m


def pack(a):
    return np.packbits(np.asarray(a).astype(bool).ravel())


def main():
    rng = np.random.default_rng(20211017)
    main_arrays, grads = {}, {"hd": {}, "boundary": {}}
    # ---- fields
    names = []
    for name, shape in (("small", (9, 11, 13)), ("wide", (5, 6, 70))):
        m = field_masks(rng, shape)
        seg = m.astype(np.float32)
        names.append(name)
        main_arrays[f"field_{name}__shape"] = np.array(m.shape, np.int64)
        main_arrays[f"field_{name}__mask"] = pack(m)
        main_arrays[f"field_{name}__hd_dist"] = ref_losses.one_hot2hd_dist(seg)
        # an int32 one-hot (what HausdorffLoss passes for the prediction): the field lands in an int32 array, truncated
        main_arrays[f"field_{name}__hd_dist_int"] = ref_losses.one_hot2hd_dist(m.astype(np.int32))
        assert main_arrays[f"field_{name}__hd_dist_int"].dtype == np.int32
        main_arrays[f"field_{name}__dist_map"] = OneHotToDist(sampling=[1, 1, 1])(seg)
        assert main_arrays[f"field_{name}__hd_dist"].dtype == np.float32 and main_arrays[f"field_{name}__dist_map"].dtype == np.float32
    main_arrays["field_cases"] = np.array(names)
    # ---- losses
    N, K, S = 2, 3, (12, 20, 18)
    target = np.stack([np.stack([blobs(rng, S, 3, 6) for _ in range(K)]) for _ in range(N)])
    assert all(0 < target[n, k].sum() < target[n, k].size for n in range(N) for k in range(K))
    t = torch.from_numpy(target.astype(np.float32))
    dist = torch.from_numpy(np.stack([OneHotToDist(sampling=[1, 1, 1])(target[n].astype(np.float32)) for n in range(N)]))
    heads = [torch.from_numpy(rng.uniform(-8.0, 8.0, (N, K) + S).astype(np.float32)) for _ in range(3)]
    tie = rng.uniform(-8.0, 8.0, (N, K) + S).astype(np.float32)
    tie[:, 1, :6] = tie[:, 0, :6] = np.abs(tie[:, 0, :6]) + 0.5     # channels 0 and 1 exactly equal (mostly above channel 2)
    tie[:, 2, 6:9, :10] = tie[:, 1, 6:9, :10]                         # channels 1 and 2 exactly equal
    tie[:, :, 9:, 10:] = rng.uniform(25.0, 40.0, tie[:, :, 9:, 10:].shape).astype(np.float32)  # every sigmoid saturates to 1
    tie = torch.from_numpy(tie)
    main_arrays["loss__shape"] = np.array((N, K) + S, np.int64)
    main_arrays["loss__target"] = pack(target)
    main_arrays["loss__dist_map"] = dist.numpy()
    for i, h in enumerate(heads):
        main_arrays[f"loss__head{i}"] = h.numpy()
    main_arrays["loss__tie"] = tie.numpy()
    make_criterion = reference_make_criterion()
    cases = {"single": heads[:1], "deep3": heads, "tie": [tie]}
    for crit in CRITERIA:
        criterion = make_criterion(argparse.Namespace(criterion=crit, num_classes=K))
        label = [t, dist] if "boundary" in crit else t
        for case, hs in cases.items():
            if case == "tie" and "hd" not in crit:
                continue  # (the tie rule belongs to the arg-max of the hd criteria)
            xs = [h.clone().requires_grad_(True) for h in hs]
            loss = torch.mean(torch.stack([criterion(x, label) for x in xs]))  # learning/engine.py:326-329
            loss.backward()
            f64, g64 = R.loss_and_grads(crit, hs, t, dist)
            main_arrays[f"{crit}__{case}__loss"] = loss.detach().numpy()
            main_arrays[f"{crit}__{case}__f64"] = f64.numpy()
            rel = abs(float(loss.detach()) - float(f64)) / abs(float(f64))
            gerr = max(float((x.grad.double() - g).abs().max() / g.abs().max()) for x, g in zip(xs, g64))
            print(f"{crit:14s} {case:7s} loss {float(loss.detach()):.7f}  f64 {float(f64):.10f}  f32 rel err {rel:.2e}  grad err / max {gerr:.2e}")
            if case != "single":  # (the single case is head 0 of deep3: its gradient is 3 x that head's)
                for i, x in enumerate(xs):
                    grads["hd" if "hd" in crit else "boundary"][f"{crit}__{case}__grad{i}"] = x.grad.numpy()
    for name, arrays in (("losses", main_arrays), ("losses_grad_hd", grads["hd"]), ("losses_grad_boundary", grads["boundary"])):
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **arrays)
        print("wrote", path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
