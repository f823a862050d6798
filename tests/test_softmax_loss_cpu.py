"""CPU tests of the exclusive-class additions: the header declares the entry points of csrc/softmax_loss.hip at ABI version 7, the
criterion's and the Evaluator's option and shape errors hold, CPU tensors raise, the float64 restatement is self-consistent, and
definer.make_criterion still refuses the MONAI-only names."""
import argparse

import pytest
import torch

import _softmax_ref as R
from brats21_amd import _lib

SIGNATURES = {"brats_softmax_ws_floats": ("z", "ii"),
              "brats_softmax_stats": ("i", "ppppiizp"),
              "brats_softmax_grad": ("i", "ppppiizip"),
              "brats_label_stats_ws_floats": ("z", "i"),
              "brats_label_stats": ("i", "pppiizp"),
              "brats_softmax_planes": ("i", "ppiizp"),
              "brats_argmax_labels": ("i", "pppiiizp")}


def test_new_symbols_are_declared_bound_and_the_abi_version_stays_7():
    sigs = _lib._parse_header()
    for name, sig in SIGNATURES.items():
        assert name in _lib.declared_symbols() and sigs[name] == sig, name
    assert _lib._header_abi_version() == 7
    lib = _lib.lib()
    assert lib.brats_abi_version() == 7
    for name, (_, spec) in SIGNATURES.items():
        assert len(getattr(lib, name).argtypes) == len(spec)
    # the workspace queries need no device: one row of 3K + 1 partial sums per workgroup and sample; 0 outside 2 <= K <= 16
    assert lib.brats_softmax_ws_floats(2, 16) >= 2 * 49 and lib.brats_softmax_ws_floats(2, 16) % (2 * 49) == 0
    assert lib.brats_softmax_ws_floats(1, 1) == 0 and lib.brats_softmax_ws_floats(1, 17) == 0 and lib.brats_softmax_ws_floats(0, 4) == 0
    assert lib.brats_label_stats_ws_floats(3) >= 3 * 17 and lib.brats_label_stats_ws_floats(0) == 0


def test_criterion_option_errors():
    from brats21_amd import losses
    for bad in (dict(lambda_dice=-1.0), dict(lambda_ce=-0.5)):
        with pytest.raises(ValueError):
            losses.SoftmaxDiceCELoss(**bad)
    c = losses.SoftmaxDiceCELoss(include_background=False, squared_pred=False, jaccard=True, batch=False, smooth_nr=0.0, smooth_dr=1e-6,
                                 lambda_dice=0.0, lambda_ce=2.0)
    assert (c.include_background, c.squared_pred, c.jaccard, c.batch, c.smooth_nr, c.smooth_dr, c.lambda_dice, c.lambda_ce) == \
        (False, False, True, False, 0.0, 1e-6, 0.0, 2.0)
    d = losses.SoftmaxDiceCELoss()
    assert (d.include_background, d.squared_pred, d.jaccard, d.batch, d.smooth_nr, d.smooth_dr, d.lambda_dice, d.lambda_ce) == \
        (True, True, False, True, 1e-5, 1e-5, 1.0, 1.0)
    assert hasattr(d, "prepare")  # TrainStep shares one target pass between the heads through it


def test_class_count_shape_and_device_errors():
    from brats21_amd import losses
    c = losses.SoftmaxDiceCELoss()
    y = torch.zeros((2, 1, 4, 4, 4), dtype=torch.uint8)
    for k in (1, 17):
        with pytest.raises(NotImplementedError):
            c(torch.zeros((2, k, 4, 4, 4)), y)
    for bad in (torch.zeros((2, 1, 4, 4, 5)), torch.zeros((2, 4, 4, 5)), torch.zeros((1, 1, 4, 4, 4)), torch.zeros((2, 2, 4, 4, 4))):
        with pytest.raises(AssertionError):
            c(torch.zeros((2, 3, 4, 4, 4)), bad)
    for good in (y, y[:, 0], y.float(), torch.zeros((2, 3, 4, 4, 4))):  # label maps and the one-hot: only the device is wrong
        with pytest.raises(_lib.BratsHipError):
            c(torch.zeros((2, 3, 4, 4, 4)), good)
    with pytest.raises(_lib.BratsHipError):
        c.prepare(y)
    from brats21_amd import ops
    with pytest.raises(_lib.BratsHipError):
        ops.softmax_planes(torch.zeros((1, 3, 2, 2, 2)))
    with pytest.raises(_lib.BratsHipError):
        ops.argmax_labels(torch.zeros((1, 3, 2, 2, 2)))


def test_evaluator_softmax_refuses_the_brats_region_operations():
    from brats21_amd.evaluate import Evaluator
    model = torch.nn.Identity()
    ev = Evaluator([model], activation="softmax", use_graph=False)
    assert ev.activation == "softmax" and Evaluator([model], use_graph=False).activation == "sigmoid"
    for bad in (dict(thresh=0.4), dict(cleaning_areas_threshold=10), dict(replace_value_threshold=5), dict(perform_staple=True)):
        with pytest.raises(NotImplementedError):
            Evaluator([model], activation="softmax", use_graph=False, **bad)
        Evaluator([model], use_graph=False, **bad)  # still fine with the sigmoid chain
    with pytest.raises(ValueError):
        Evaluator([model], activation="tanh", use_graph=False)
    from brats21_amd.tta.base import SignedPerm, Transformer
    t = Transformer(SignedPerm(), SignedPerm())
    with pytest.raises(ValueError):
        t.accumulate_probability(torch.zeros((1, 3, 2, 2, 2)), torch.zeros((1, 3, 2, 2, 2)), activation="tanh")
    for act in ("sigmoid", "softmax"):
        with pytest.raises(_lib.BratsHipError):
            t.accumulate_probability(torch.zeros((1, 3, 2, 2, 2)), torch.zeros((1, 3, 2, 2, 2)), activation=act)


def test_make_criterion_still_refuses_dice_ce():
    from brats21_amd import definer
    with pytest.raises(NotImplementedError):
        definer.make_criterion(argparse.Namespace(criterion="dice_ce", num_classes=3))


def test_restatement_is_the_torch_composition():
    """Without ignored voxels the restatement is softmax + one_hot + the Dice algebra + F.cross_entropy written out; an ignored
    voxel changes neither part when its logits change."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn((2, 4, 3, 4, 5), generator=g, dtype=torch.float64)
    y = torch.randint(0, 4, (2, 3, 4, 5), generator=g)
    p = torch.softmax(x, 1)
    t = torch.nn.functional.one_hot(y, 4).movedim(-1, 1).double()
    inter, den = (p * t).sum((0, 2, 3, 4)), (t * t).sum((0, 2, 3, 4)) + (p * p).sum((0, 2, 3, 4))
    want = (1 - (2 * inter + 1e-5) / (den + 1e-5)).mean() + torch.nn.functional.cross_entropy(x, y)
    assert abs(float(R.softmax_dice_ce(x, y)) - float(want)) < 1e-14
    y[0, 0, 0, 0] = 255
    a = R.softmax_dice_ce(x, y, jaccard=True, batch=False, include_background=False)
    x2 = x.clone()
    x2[0, :, 0, 0, 0] += torch.tensor([3.0, -2.0, 0.5, 7.0], dtype=torch.float64)
    assert float(a) == float(R.softmax_dice_ce(x2, y, jaccard=True, batch=False, include_background=False))
    f, grads = R.deep_loss_and_grads([x, x2], y, torch.float64)
    assert float(grads[0][0, :, 0, 0, 0].abs().max()) == 0.0 and float(grads[0].abs().max()) > 0
    assert torch.equal(R.ignore_above(torch.tensor([0, 2, 3, 200, 255]), 3), torch.tensor([0, 2, 255, 255, 255], dtype=torch.uint8))
