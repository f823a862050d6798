"""-m "not gpu": tests/_losses_ref.py (the scipy-free restatement the GPU parity tests compare against) is pinned to
tests/golden/losses*.npz -- the reference's own loss classes and OneHotToDist over real scipy (make_golden_losses.py) --
with the distance fields bit-equal; plus the host-side surface of the distance-map criteria: the make_criterion factory,
the constructor errors and the GPU-only errors."""
import argparse
import os

import numpy as np
import pytest
import torch

import _losses_ref as R

CRITERIA = ("hd", "dice_hd", "boundary", "dice_boundary")


def load_goldens(golden_dir):
    g = dict(np.load(os.path.join(golden_dir, "losses.npz")))
    for name in ("losses_grad_hd.npz", "losses_grad_boundary.npz"):
        g.update(np.load(os.path.join(golden_dir, name)))
    return g


def field_case(g, name):
    shape = tuple(int(v) for v in g[f"field_{name}__shape"])
    mask = np.unpackbits(g[f"field_{name}__mask"])[:int(np.prod(shape))].reshape(shape).astype(bool)
    return torch.from_numpy(mask)


def loss_inputs(g):
    shape = tuple(int(v) for v in g["loss__shape"])
    target = np.unpackbits(g["loss__target"])[:int(np.prod(shape))].reshape(shape).astype(np.float32)
    heads = [torch.from_numpy(g[f"loss__head{i}"]) for i in range(3)]
    cases = {"single": heads[:1], "deep3": heads, "tie": [torch.from_numpy(g["loss__tie"])]}
    return torch.from_numpy(target), torch.from_numpy(g["loss__dist_map"]), cases


def loss_cases(crit):
    return ("single", "deep3", "tie") if "hd" in crit else ("single", "deep3")


def golden_grads(g, crit, case, nheads):
    """The reference's f32 gradients; the single case is head 0 of deep3, whose gradient carries the 1/3 of the mean."""
    if case == "single":
        return [torch.from_numpy(g[f"{crit}__deep3__grad0"]) * 3.0]
    return [torch.from_numpy(g[f"{crit}__{case}__grad{i}"]) for i in range(nheads)]


@pytest.fixture(scope="module")
def goldens(golden_dir):
    return load_goldens(golden_dir)


def test_restated_fields_are_bit_equal_to_the_reference(goldens):
    for name in goldens["field_cases"]:
        m = field_case(goldens, name)
        seg = m.float()
        assert m[3].sum() == 0 and m[4].all() and m[5].sum() == 1  # the empty, the all-one and the one-voxel plane
        for key, got in (("hd_dist", R.hd_dist(seg)), ("hd_dist_int", R.hd_dist(seg, integer=True)), ("dist_map", R.one_hot_to_dist(seg))):
            want = goldens[f"field_{name}__{key}"].astype(np.float32)
            assert np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32)), (name, key)
    # scipy's value for a volume without background (the degenerate rule): distance to index (-1, 0, 0)
    full = goldens["field_small__hd_dist"][4]
    assert full[0, 0, 0] == 1.0 and full[0, 0, 1] == np.float32(np.sqrt(2.0)) and full[0, 0, 2] == np.float32(np.sqrt(5.0))
    assert full[2, 3, 4] == np.float32(np.sqrt(9.0 + 9.0 + 16.0))


@pytest.mark.parametrize("crit", CRITERIA)
def test_restated_losses_match_the_reference(goldens, crit):
    target, dist, cases = loss_inputs(goldens)
    assert all(0 < target[n, k].sum() < target[n, k].numel() for n in range(2) for k in range(3))  # no degenerate target plane
    for case in loss_cases(crit):
        heads = cases[case]
        f64, g64 = R.loss_and_grads(crit, heads, target, dist)
        assert abs(float(f64) - float(goldens[f"{crit}__{case}__f64"])) <= 1e-12 * abs(float(f64)), (crit, case)
        ref = float(goldens[f"{crit}__{case}__loss"])
        assert abs(ref - float(f64)) <= 1e-6 * abs(float(f64)), (crit, case, ref, float(f64))
        for got, want in zip(g64, golden_grads(goldens, crit, case, len(heads))):
            torch.testing.assert_close(got.float(), want, rtol=1e-4, atol=1e-9)


def test_tie_case_holds_ties_and_saturated_voxels(goldens):
    x = torch.from_numpy(goldens["loss__tie"])
    p = torch.sigmoid(x)
    assert (x[:, 0, :6] == x[:, 1, :6]).all() and (x[:, 1, 6:9, :10] == x[:, 2, 6:9, :10]).all()
    assert (p[:, :, 9:, 10:] == 1.0).all()
    oh = R.probs_one_hot(x)
    assert (oh[:, 0, 9:, 10:] == 1).all()  # saturated everywhere: the lowest channel wins
    assert (oh[:, 1, :6] == 0).all()       # channel 1 never beats its equal, channel 0


REFERENCE_KWARGS = {  # src/definer.py:246-288
    "hd": ("HausdorffLoss", {"idc": [0, 1, 2], "sigmoid": True, "softmax": False, "alpha": 2, "reduction": "mean"}),
    "dice_hd": ("DiceHDLoss", {"idc_hd": [0, 1, 2], "alpha_hd": 2, "hybrid": False, "include_background": True, "sigmoid": True,
                               "softmax": False, "squared_pred": True, "weight_hd": 0.5, "weight_dice": 0.5, "reduction": "mean"}),
    "boundary": ("BoundaryLoss", {"idc": [0, 1, 2], "sigmoid": True, "softmax": False, "reduction": "mean"}),
    "dice_boundary": ("DiceBoundaryLoss", {"idc_boundary": [0, 1, 2], "include_background": True, "sigmoid": True, "softmax": False,
                                           "squared_pred": True, "reduction": "mean"}),
}


def check_factory(monkeypatch):
    from brats21_amd import definer, losses
    ns = lambda name: argparse.Namespace(criterion=name, num_classes=3)  # noqa: E731
    for name, jac in (("dice", False), ("jaccard", True)):
        c = definer.make_criterion(ns(name))
        assert type(c) is losses.DiceLoss and c.jaccard is jac
    kinds = {"hd": losses.HausdorffLoss, "dice_hd": losses.DiceHDLoss, "boundary": losses.SurfaceLoss,
             "dice_boundary": losses.DiceBoundaryLoss}
    assert losses.BoundaryLoss is losses.SurfaceLoss
    for name, kind in kinds.items():
        assert type(definer.make_criterion(ns(name))) is kind
    c = definer.make_criterion(ns("dice_hd"))
    assert c.hd.idc == [0, 1, 2] and c.hd.alpha == 2.0 and not c.hybrid and not c.dice.batch and not c.dice.jaccard
    c = definer.make_criterion(ns("dice_boundary"))
    assert c.boundary.idc == [0, 1, 2] and not c.dice.batch and c.lambda_dice == c.lambda_boundary == 1.0
    seen = {}
    for name, (cls, _) in REFERENCE_KWARGS.items():
        monkeypatch.setattr(losses, cls, lambda _n=name, **kw: seen.__setitem__(_n, kw))
    for name, (_, want) in REFERENCE_KWARGS.items():
        definer.make_criterion(ns(name))
        assert seen[name] == want, name
    monkeypatch.undo()
    for name in ("generalized_dice", "focal", "tversky", "dice_ce", "dice_focal"):
        with pytest.raises(NotImplementedError, match=name):
            definer.make_criterion(ns(name))
    with pytest.raises(NameError, match="Not Supported Criterion"):
        definer.make_criterion(ns("lovasz"))


def test_make_criterion(monkeypatch):
    check_factory(monkeypatch)


def test_unbuilt_options_and_cpu_tensors_raise():
    from brats21_amd import BratsHipError, losses, ops, transforms
    for kw in ({"softmax": True}, {"to_onehot_y": True}, {"other_act": torch.tanh}, {"reduction": "sum"}, {"reduction": "none"},
               {"sigmoid": False}):
        args = {"sigmoid": True, **kw}
        with pytest.raises(NotImplementedError):
            losses.HausdorffLoss(idc=[0, 1, 2], **args)
        with pytest.raises(NotImplementedError):
            losses.SurfaceLoss(idc=[0, 1, 2], **args)
        with pytest.raises(NotImplementedError):
            losses.DiceHDLoss(idc_hd=[0, 1, 2], squared_pred=True, **args)
        with pytest.raises(NotImplementedError):
            losses.DiceBoundaryLoss(idc_boundary=[0, 1, 2], squared_pred=True, **args)
    with pytest.raises(ValueError):
        losses.DiceBoundaryLoss(idc_boundary=[0], sigmoid=True, squared_pred=True, lambda_dice=-1.0)
    x = torch.zeros(1, 3, 4, 4, 4)
    with pytest.raises(BratsHipError):
        ops.distance_transform_edt(x)
    with pytest.raises(BratsHipError):
        transforms.one_hot_to_dist(x)
    with pytest.raises(BratsHipError):
        losses.HausdorffLoss(idc=[0, 1, 2], sigmoid=True)(x, x)
    with pytest.raises(BratsHipError):
        losses.SurfaceLoss(idc=[0, 1, 2], sigmoid=True)(x, [x, x])
    with pytest.raises(BratsHipError):
        losses.DiceBoundaryLoss(idc_boundary=[0, 1, 2], sigmoid=True, squared_pred=True)(x, [x, x])


def test_edt_entry_point_rejects_bad_arguments():
    import ctypes
    from brats21_amd import _lib
    l = _lib.lib()
    assert l.brats_edt_ws_bytes(6, 128, 128, 128) >= 2 * 6 * 128 ** 3 * 4
    assert l.brats_edt_ws_bytes(1, 2049, 4, 4) == 0 and l.brats_edt_ws_bytes(1, 4, 4, 2049) == 0 and l.brats_edt_ws_bytes(0, 4, 4, 4) == 0
    buf = (ctypes.c_float * 64)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    assert l.brats_edt(None, 0, 1, 4, 4, 4, 0, ptr, ptr, None) == -1 and b"edt" in l.brats_last_error()
    for bad in ((2049, 4, 4), (4, 2049, 4), (4, 4, 2049), (0, 4, 4)):
        assert l.brats_edt(ptr, 0, 1, *bad, 0, ptr, ptr, None) == -1  # BRATS_E_ARG, nothing launched
    assert l.brats_edt(ptr, 2, 1, 4, 4, 4, 0, ptr, ptr, None) == -1   # unknown mask kind
    assert l.brats_edt(ptr, 0, 1, 4, 4, 4, 3, ptr, ptr, None) == -1   # unknown mode
    assert l.brats_hd_loss_stats(None, None, None, None, 2.0, None, None, 8, None) == -1
    assert l.brats_boundary_loss_grad(None, None, None, None, 8, None) == -1
