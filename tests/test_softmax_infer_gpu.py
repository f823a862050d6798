"""GPU tests of exclusive-class inference: ops.softmax_planes / ops.argmax_labels (csrc/softmax_loss.hip),
Transformer.accumulate_probability(activation="softmax") and Evaluator(activation="softmax").

Bars.  softmax_planes against torch.softmax in float64: 4 x the max abs error of torch.softmax in float32 on the CPU on the same
logits (summation order, __expf).  argmax_labels and the end-to-end label maps: exactly equal, at every voxel."""
import argparse
import contextlib
import io

import pytest
import torch

from test_softmax_loss_gpu import SHAPES, make_logits, on_device

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("k", [2, 3, 5, 16])
def test_softmax_planes_matches_float64(k):
    from brats21_amd import ops
    g = torch.Generator().manual_seed(300 + k)
    for n in (1, 3):
        for shape in SHAPES:
            mis = shape == "misaligned"
            sp = (8, 12, 20) if mis else shape
            for stress in (False, True):
                x = make_logits(n, k, sp, g, stress=stress)
                want = torch.softmax(x.double(), 1)
                ref_err = float((torch.softmax(x, 1).double() - want).abs().max())
                xd = on_device(x, mis)
                got = ops.softmax_planes(xd)
                assert got.dtype == torch.float32 and got.shape == x.shape and got.data_ptr() != xd.data_ptr()
                assert torch.equal(xd.cpu(), x)  # the input is left alone
                err = float((got.cpu().double() - want).abs().max())
                line = f"K={k} N={n} {shape} stress={stress}: max abs err {err:.2e} (bar {4 * ref_err:.2e}, float32 CPU {ref_err:.2e})"
                print("\n" + line)
                assert bool(torch.isfinite(got).all()) and err <= 4.0 * ref_err, line
                same = ops.softmax_planes(xd, inplace=True)
                assert same.data_ptr() == xd.data_ptr() and torch.equal(same, got), line  # in place: the same bits


def planted_sums(n, k, shape, c, g):
    """probability sums with exact ties planted (two, three and all classes equal at the maximum) and an image with all-zero
    voxels planted; every value distinct elsewhere"""
    s = torch.rand((n, k) + shape, generator=g)
    v = s.flatten(2)  # a view
    nv = v.shape[2]
    top = v.max(1).values
    for i in range(0, nv, 3):  # the maximum repeated in another class, below or above the first one
        v[:, (i * 7) % k, i] = top[:, i]
    for i in range(1, nv, 11):
        v[:, :, i] = 0.25
    if k > 2:
        for i in range(2, nv, 13):
            v[:, k - 1, i] = v[:, k - 2, i] = v[:, 0, i] = 2.0
    img = torch.randn((n, c) + shape, generator=g)
    iv = img.flatten(2)
    iv[:, :, ::5] = 0.0          # background
    iv[:, 0, 1::5] = 0.0         # one channel zero only: still foreground
    iv[:, :, 2::25] = -0.0       # negative zero is zero
    return s, img


@pytest.mark.parametrize("k", [2, 5, 16])
def test_argmax_labels_equal_torch_argmax(k):
    from brats21_amd import ops
    g = torch.Generator().manual_seed(500 + k)
    for n in (1, 3):
        for shape in SHAPES:
            mis = shape == "misaligned"
            sp = (8, 12, 20) if mis else shape
            s, img = planted_sums(n, k, sp, 4, g)
            want = torch.argmax(s, 1, keepdim=True)
            first = (s == s.max(1, keepdim=True).values).float().argmax(1, keepdim=True)  # the lowest class at the maximum
            assert torch.equal(want, first)
            got = ops.argmax_labels(on_device(s, mis))
            assert got.dtype == torch.uint8 and tuple(got.shape) == (n, 1) + sp
            assert torch.equal(got.cpu().long(), want), (k, n, shape)
            fg = (img != 0).any(1, keepdim=True)
            assert 0.1 < float(fg.float().mean()) < 0.9
            got = ops.argmax_labels(on_device(s, mis), on_device(img, mis))
            assert torch.equal(got.cpu().long(), torch.where(fg, want, 0)), (k, n, shape, "background removal")


class Pointwise(torch.nn.Module):
    """logits[n, k, v] = sum_c w[k, c] x[n, c, v] + b[k] with small integer weights: on an integer image every logit is an integer"""

    def __init__(self):
        super().__init__()
        self.register_buffer("w", torch.tensor([[1, 0, -1, 0], [0, 1, 0, -1], [1, 1, 0, 0], [0, -1, 1, 1], [1, 0, 0, -1]], dtype=torch.float32))
        self.register_buffer("b", torch.tensor([0, 1, -1, 0, 0], dtype=torch.float32))

    def forward(self, x):
        return (x[:, None].to(self.w.dtype) * self.w.view(1, 5, 4, 1, 1, 1)).sum(2) + self.b.view(1, 5, 1, 1, 1)


class Regions(Pointwise):
    """the first three channels: a stand-in for a TC / WT / ET model"""

    def forward(self, x):
        return super().forward(x)[:, :3]


def integer_case():
    g = torch.Generator().manual_seed(24)
    img = torch.randint(-3, 4, (2, 4, 21, 22, 24), generator=g).float()
    img[:, :, :4] = 0.0
    img[:, :, :, :, 20:] = 0.0
    img[1, :, 8:12, 8:12, 8:12] = 0.0
    labels = torch.randint(0, 5, (2, 1, 21, 22, 24), generator=g)
    return img, labels


def test_evaluator_softmax_labels_equal_the_float64_composition():
    from brats21_amd import tta
    from brats21_amd.evaluate import Evaluator, hard_dice_metric, shape_to_divisible
    img, target = integer_case()
    onehot = torch.nn.functional.one_hot(target[:, 0], 5).movedim(-1, 1).float()
    model = Pointwise().to(DEV)
    ev = Evaluator(model, activation="softmax", tta_transforms=tta.get_tta_transforms(), amp=False)
    out = ev(img.to(DEV), onehot.to(DEV))
    # float64 composition on the CPU: pad to 24, the same 16 passes, softmax, sum, arg-max, background removal, crop
    pad = torch.zeros((2, 4, 24, 24, 24), dtype=torch.float64)
    pad[:, :, 2:23, 1:23, :] = img.double()  # the odd voxel of an odd padding goes in front (shape_to_divisible)
    ref_model = Pointwise().double()
    with torch.no_grad():
        logits = ref_model(pad)
        acc = torch.softmax(logits, 1) * 16.0  # a pointwise model: every de-augmented pass is the same tensor
    assert float((logits - logits.round()).abs().max()) == 0.0
    top2 = logits.topk(2, 1).values
    assert bool((top2[:, 0] == top2[:, 1]).any()) and bool((top2[:, 0] > top2[:, 1]).any())  # exact ties and clear winners
    want = torch.where((pad != 0).any(1, keepdim=True), acc.argmax(1, keepdim=True), 0)
    assert torch.equal(want, torch.where((pad != 0).any(1, keepdim=True), logits.argmax(1, keepdim=True), 0))
    want_c = want[:, :, 2:23, 1:23, :]
    assert out["labels"].dtype == torch.uint8 and tuple(out["labels"].shape) == (2, 1, 21, 22, 24)
    assert torch.equal(out["labels"].cpu().long(), want_c)  # every voxel, no exclusions
    assert len(torch.unique(want_c)) == 5
    assert out["seg"].dtype == torch.float32 and tuple(out["seg"].shape) == (2, 5, 21, 22, 24)
    assert torch.equal(out["seg"].cpu(), torch.nn.functional.one_hot(out["labels"][:, 0].cpu().long(), 5).movedim(-1, 1).float())
    seg_p = torch.nn.functional.one_hot(want[:, 0], 5).movedim(-1, 1).float().to(DEV)
    assert torch.equal(out["dice"], hard_dice_metric(seg_p, shape_to_divisible(onehot.to(DEV), k=8)[0]))
    assert tuple(out["dice"].shape) == (2, 5)
    # the probability sum itself, and one pass of the accumulation against torch
    acc_gpu, passes = ev.probability_sum(shape_to_divisible(img.to(DEV), k=8)[0])
    assert passes == 16
    torch.testing.assert_close(acc_gpu.cpu().double(), acc, rtol=0, atol=16 * 4e-7)
    t = list(tta.get_tta_transforms())[5]
    x = torch.randn((1, 3, 6, 6, 6), device=DEV)
    a = torch.ones(t.deaug_perm.out_shape(x.shape), device=DEV)
    t.accumulate_probability(x, a, activation="softmax")
    torch.testing.assert_close(a, 1.0 + t.deaugment_mask(torch.softmax(x, 1)), rtol=0, atol=4e-7)
    # no TTA, two models: the sum over models
    ev2 = Evaluator([model, model], activation="softmax", amp=False)
    out2 = ev2(img.to(DEV), want_labels=False)
    assert torch.equal(out2["labels"], out["labels"]) and "dice" not in out2


def test_evaluator_softmax_runs_a_network_whole_and_windowed():
    from brats21_amd import get_model
    from brats21_amd.evaluate import Evaluator
    from oracle import synth
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        m = get_model(argparse.Namespace(model="equiunet", width=8, norm="group", act="relu", num_classes=4, dropout=0)).to(DEV).eval()
    x = synth.random_image(1, 4, (32, 32, 32), seed=3).to(DEV)
    x[:, :, :3] = 0.0
    for roi in (None, (16, 16, 16)):
        out = Evaluator(m, activation="softmax", sliding_window_size=roi)(x)
        assert out["labels"].dtype == torch.uint8 and tuple(out["labels"].shape) == (1, 1, 32, 32, 32)
        assert out["seg"].dtype == torch.float32 and tuple(out["seg"].shape) == (1, 4, 32, 32, 32)
        assert int(out["labels"].max()) < 4 and int(out["labels"][:, :, :3].max()) == 0
        assert torch.equal(out["seg"].sum(1), torch.ones_like(out["seg"][:, 0]))


def test_sigmoid_mode_is_bit_identical_to_the_default():
    from brats21_amd import tta
    from brats21_amd.evaluate import Evaluator
    img, _ = integer_case()
    model = Regions().to(DEV)
    x = (img * 0.37).to(DEV)
    a = Evaluator(model, tta_transforms=tta.get_tta_transforms(), amp=False)(x, want_labels=True)
    b = Evaluator(model, tta_transforms=tta.get_tta_transforms(), amp=False, activation="sigmoid")(x, want_labels=True)
    assert a.keys() == b.keys() and all(torch.equal(a[key], b[key]) for key in a)
    pa = Evaluator(model, tta_transforms=tta.get_tta_transforms(), amp=False).probability_sum(x[:, :, :16, :16, :16])
    pb = Evaluator(model, tta_transforms=tta.get_tta_transforms(), amp=False, activation="sigmoid").probability_sum(x[:, :, :16, :16, :16])
    assert pa[1] == pb[1] == 16 and torch.equal(pa[0], pb[0])
    t = list(tta.get_tta_transforms())[3]
    lg = torch.randn((1, 3, 6, 6, 6), device=DEV)
    a1, a2 = torch.zeros(t.deaug_perm.out_shape(lg.shape), device=DEV), torch.zeros(t.deaug_perm.out_shape(lg.shape), device=DEV)
    t.accumulate_probability(lg, a1)
    t.accumulate_probability(lg, a2, activation="sigmoid")
    assert torch.equal(a1, a2) and float(a1.abs().max()) > 0
