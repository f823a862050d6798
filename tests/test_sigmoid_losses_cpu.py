"""CPU tests of the multi-label criteria losses.DiceCELoss, DiceFocalLoss, FocalLoss and TverskyLoss (csrc/sigmoid_loss.hip): the
float64 restatement tests/_sigmoid_losses_ref.py is self-consistent, the closed forms the kernels and the [N, K] algebra use
(the focal gradient, the coefficient table) equal autograd on it, each class constructs with the keyword set src/definer.py
passes, every unbuilt option raises, and the header declares the new entry points at ABI version 7."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import _sigmoid_losses_ref as R
from brats21_amd import _lib

# what src/definer.py:204-245 passes (reduction="mean" is added at :286)
REFERENCE_KWARGS = {
    "DiceCELoss": dict(include_background=True, sigmoid=True, softmax=False, squared_pred=True, batch=True, reduction="mean"),
    "DiceFocalLoss": dict(include_background=True, sigmoid=True, softmax=False, squared_pred=True, batch=False, reduction="mean"),
    "FocalLoss": dict(gamma=2.0, reduction="mean"),
    "TverskyLoss": dict(include_background=True, sigmoid=True, softmax=False, alpha=0.5, beta=0.5, reduction="mean"),
}
RESTATEMENT = {"DiceCELoss": "dice_ce", "DiceFocalLoss": "dice_focal", "FocalLoss": "focal", "TverskyLoss": "tversky"}
SIGNATURES = {"brats_sigmoid_loss_ws_floats": ("z", "ii"),
              "brats_sigmoid_target_prepare": ("i", "ppppiizp"),
              "brats_sigmoid_loss_stats": ("i", "pppppiizifp"),
              "brats_sigmoid_loss_grad": ("i", "pppppiizifp")}


def _case(seed=3, n=2, k=3, shape=(3, 4, 5), soft=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n, k) + shape, generator=g, dtype=torch.float64) * 3.0
    t = torch.rand((n, k) + shape, generator=g, dtype=torch.float64)
    return x, t if soft else (t < 0.4).double()


# ------------------------------------------------------------------------------------------ the restatement's own identities
def test_focal_at_gamma_0_is_bce_with_logits():
    for soft in (False, True):
        x, t = _case(soft=soft)
        assert abs(float(R.focal(x, t, gamma=0.0)) - float(F.binary_cross_entropy_with_logits(x, t))) < 1e-14


def test_focal_is_one_minus_pt_to_the_gamma_times_bce_on_binary_targets():
    x, t = _case()
    p = torch.sigmoid(x)
    pt = torch.where(t == 1, p, 1 - p)
    for gamma in (2.0, 3.5):
        want = (1 - pt) ** gamma * F.binary_cross_entropy_with_logits(x, t, reduction="none")
        torch.testing.assert_close(R.focal_elements(x, t, gamma), want, rtol=1e-12, atol=1e-14)


def test_tversky_at_half_half_is_the_non_squared_dice():
    x, t = _case()
    p = torch.sigmoid(x)
    for batch in (False, True):
        axes = (0, 2, 3, 4) if batch else (2, 3, 4)
        inter, p1, t1 = (p * t).sum(axes), p.sum(axes), t.sum(axes)
        want = (1 - (2 * inter + 2 * 1e-3) / (p1 + t1 + 2 * 1e-4)).mean()
        assert abs(float(R.tversky(x, t, 0.5, 0.5, batch, smooth_nr=1e-3, smooth_dr=1e-4)) - float(want)) < 1e-14


def test_class_map_of_the_eight_brats_channel_patterns():
    """argmax with ties to the lowest channel: only 010 / 011 give class 1 and 001 class 2; the background 000 and 111 are class 0."""
    patterns = torch.tensor([[a, b, c] for a in (0, 1) for b in (0, 1) for c in (0, 1)], dtype=torch.float64)
    t = patterns.t().reshape(1, 3, 2, 2, 2)
    assert R.class_map(t).flatten().tolist() == [0, 2, 1, 1, 0, 0, 0, 0]
    x = torch.randn((1, 3, 2, 2, 2), dtype=torch.float64)
    want = R.dice(x, t, batch=True) + (torch.logsumexp(x, 1) - x.gather(1, R.class_map(t)[:, None])[:, 0]).mean()
    assert abs(float(R.dice_ce(x, t)) - float(want)) < 1e-14
    assert float(R.dice_ce(x[:, :1], t[:, :1])) == float(R.dice(x[:, :1], t[:, :1], batch=True))  # K = 1: the CE term is exactly 0


# ------------------------------------------------------------------------------------------ the closed forms of kernels and algebra
def _focal_gradient(x, t, gamma):
    """d focal / dx as csrc/sigmoid_loss.hip writes it"""
    u = 2 * t - 1
    q = F.logsigmoid(-x * u)
    return (gamma * q).exp() * (torch.sigmoid(x) - t - gamma * R.bce_with_logits(x, t) * u * torch.sigmoid(x * u))


@pytest.mark.parametrize("gamma", [0.0, 2.0, 3.5])
@pytest.mark.parametrize("soft", [False, True])
def test_focal_gradient_formula_is_autograd(gamma, soft):
    x, t = _case(soft=soft)
    x[0, 0, 0, 0, :2] = torch.tensor([100.0, -100.0], dtype=torch.float64)
    x = x.requires_grad_(True)
    R.focal_elements(x, t, gamma).sum().backward()
    torch.testing.assert_close(_focal_gradient(x.detach(), t, gamma), x.grad, rtol=1e-11, atol=1e-13)


OPTION_SETS = {
    "DiceCELoss": [dict(), dict(jaccard=True, batch=False, lambda_dice=0.7, lambda_ce=1.3, smooth_nr=1e-3, smooth_dr=1e-4)],
    "DiceFocalLoss": [dict(), dict(jaccard=True, batch=True, gamma=3.5, lambda_dice=0.7, lambda_focal=1.3)],
    "FocalLoss": [dict(), dict(gamma=0.0)],
    "TverskyLoss": [dict(), dict(alpha=0.3, beta=0.7, batch=True, smooth_nr=1e-3, smooth_dr=1e-4)],
}


@pytest.mark.parametrize("name", list(RESTATEMENT))
def test_the_algebra_on_the_sums_is_the_restatement(name):
    """The criterion's [N, K] algebra, fed with sums formed in float64 here instead of by the statistics pass: its value is the
    restatement's, and dx put together from its coefficient table as the gradient pass does is the restatement's autograd."""
    from brats21_amd import losses
    x, t = _case(seed=5)
    n, k = x.shape[:2]
    vox = x[0, 0].numel()
    p = torch.sigmoid(x)
    y = R.class_map(t)
    for options in OPTION_SETS[name]:
        crit = getattr(losses, name)(**{**REFERENCE_KWARGS[name], **options})
        xr = x.clone().requires_grad_(True)
        want = R.CRITERIA[RESTATEMENT[name]](xr, t, **options)
        want.backward()
        want = want.detach()
        gamma = crit.gamma
        sums = [(p * t).sum((2, 3, 4)), (p * p).sum((2, 3, 4)), p.sum((2, 3, 4)), R.focal_elements(x, t, gamma).sum((2, 3, 4))]
        ce = (torch.logsumexp(x, 1) - x.gather(1, y[:, None])[:, 0]).sum((1, 2, 3))
        value, table, c = crit._algebra(*sums, ce, t.sum((2, 3, 4)), (t * t).sum((2, 3, 4)), vox)
        assert abs(float(value) - float(want)) < 1e-13, (options, float(value), float(want))
        a, b, cc, fc = [torch.zeros((n, k), dtype=torch.float64) if v is None else v.expand(n, k) for v in table]
        e = lambda v: v[:, :, None, None, None]
        dx = p * (1 - p) * (e(a) * t + 2 * e(b) * p + e(cc)) + e(fc) * _focal_gradient(x, t, gamma) \
            + c * (torch.softmax(x, 1) - F.one_hot(y, k).movedim(-1, 1))
        torch.testing.assert_close(dx, xr.grad, rtol=1e-10, atol=1e-15)
        assert bool(crit.terms & losses.SIG_CE) == (name == "DiceCELoss") and bool(crit.terms & losses.SIG_FOCAL) == ("Focal" in name)


# ------------------------------------------------------------------------------------------ constructors and errors
@pytest.mark.parametrize("name", list(REFERENCE_KWARGS))
def test_constructs_with_the_reference_keyword_set(name):
    from brats21_amd import losses
    crit = getattr(losses, name)(**REFERENCE_KWARGS[name])
    assert isinstance(crit, torch.nn.Module) and hasattr(crit, "prepare")  # TrainStep shares one target pass between the heads through it
    if name == "DiceCELoss":
        assert (crit.dice.batch, crit.dice.jaccard, crit.dice.smooth_nr, crit.dice.smooth_dr, crit.lambda_dice, crit.lambda_ce) == \
            (True, False, 1e-5, 1e-5, 1.0, 1.0)
    elif name == "DiceFocalLoss":
        assert (crit.dice.batch, crit.gamma, crit.lambda_dice, crit.lambda_focal) == (False, 2.0, 1.0, 1.0)
    elif name == "FocalLoss":
        assert crit.gamma == 2.0
    else:
        assert (crit.alpha, crit.beta, crit.batch, crit.smooth_nr, crit.smooth_dr) == (0.5, 0.5, False, 1e-5, 1e-5)


def test_defaults_are_the_references():
    """without sigmoid=True the reference's classes apply no activation: not built, so the bare constructors raise; FocalLoss has
    no activation option"""
    from brats21_amd import losses
    for name in ("DiceCELoss", "DiceFocalLoss", "TverskyLoss"):
        with pytest.raises(NotImplementedError):
            getattr(losses, name)()
    assert losses.FocalLoss().gamma == 2.0
    assert losses.DiceFocalLoss(sigmoid=True, squared_pred=True).dice.batch is False
    assert losses.DiceCELoss(sigmoid=True, squared_pred=True).dice.batch is False


UNBUILT = {
    "DiceCELoss": [dict(softmax=True), dict(to_onehot_y=True), dict(other_act=torch.tanh), dict(sigmoid=False), dict(include_background=False),
                   dict(squared_pred=False), dict(ce_weight=torch.ones(3)), dict(reduction="sum"), dict(reduction="none")],
    "DiceFocalLoss": [dict(softmax=True), dict(to_onehot_y=True), dict(other_act=torch.tanh), dict(sigmoid=False), dict(include_background=False),
                      dict(squared_pred=False), dict(focal_weight=[1.0, 2.0, 3.0]), dict(reduction="sum"), dict(reduction="none")],
    "FocalLoss": [dict(to_onehot_y=True), dict(include_background=False), dict(weight=[1.0, 2.0, 3.0]), dict(reduction="sum"),
                  dict(reduction="none")],
    "TverskyLoss": [dict(softmax=True), dict(to_onehot_y=True), dict(other_act=torch.tanh), dict(sigmoid=False), dict(include_background=False),
                    dict(reduction="sum"), dict(reduction="none")],
}


@pytest.mark.parametrize("name", list(UNBUILT))
def test_unbuilt_options_raise(name):
    from brats21_amd import losses
    for bad in UNBUILT[name]:
        with pytest.raises(NotImplementedError):
            getattr(losses, name)(**{**REFERENCE_KWARGS[name], **bad})
    with pytest.raises(NotImplementedError, match="SoftmaxDiceCELoss"):
        losses.DiceCELoss(softmax=True, to_onehot_y=True)
    for cls, bad in ((losses.DiceCELoss, dict(lambda_dice=-1.0)), (losses.DiceCELoss, dict(lambda_ce=-0.5)),
                     (losses.DiceFocalLoss, dict(lambda_dice=-1.0)), (losses.DiceFocalLoss, dict(lambda_focal=-0.5))):
        with pytest.raises(ValueError):
            cls(**{**REFERENCE_KWARGS[cls.__name__], **bad})


@pytest.mark.parametrize("name", list(REFERENCE_KWARGS))
def test_shape_class_count_and_device_errors(name):
    from brats21_amd import losses
    crit = getattr(losses, name)(**REFERENCE_KWARGS[name])
    x = torch.zeros((2, 3, 4, 4, 4))
    for bad in (torch.zeros((2, 3, 4, 4, 5)), torch.zeros((2, 1, 4, 4, 4)), torch.zeros((1, 3, 4, 4, 4))):
        with pytest.raises(AssertionError):
            crit(x, bad)
    with pytest.raises(NotImplementedError):
        crit(torch.zeros((1, 17, 2, 2, 2)), torch.zeros((1, 17, 2, 2, 2)))
    with pytest.raises(_lib.BratsHipError):  # no CPU fallback
        crit(x, torch.zeros_like(x))
    with pytest.raises(_lib.BratsHipError):
        crit.prepare(torch.zeros_like(x))


# ------------------------------------------------------------------------------------------ the C ABI
def test_new_symbols_are_declared_bound_and_the_abi_version_stays_7():
    sigs = _lib._parse_header()
    for name, sig in SIGNATURES.items():
        assert name in _lib.declared_symbols() and sigs[name] == sig, name
    assert _lib._header_abi_version() == 7
    lib = _lib.lib()
    assert lib.brats_abi_version() == 7
    for name, (_, spec) in SIGNATURES.items():
        assert len(getattr(lib, name).argtypes) == len(spec)
    # the workspace query needs no device: one row of 4K + 1 partial sums per workgroup and sample; 0 outside 1 <= K <= 16
    assert lib.brats_sigmoid_loss_ws_floats(2, 16) >= 2 * 65 and lib.brats_sigmoid_loss_ws_floats(2, 16) % (2 * 65) == 0
    assert lib.brats_sigmoid_loss_ws_floats(1, 1) >= 5
    assert lib.brats_sigmoid_loss_ws_floats(1, 0) == 0 and lib.brats_sigmoid_loss_ws_floats(1, 17) == 0 and lib.brats_sigmoid_loss_ws_floats(0, 4) == 0


def test_argument_errors_come_before_any_launch():
    lib = _lib.lib()
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.brats_sigmoid_loss_stats(None, p, None, p, p, 1, 3, 8, 0, 2.0, None) == -1 and b"sigmoid_loss_stats" in lib.brats_last_error()
    assert lib.brats_sigmoid_loss_grad(p, p, None, None, p, 1, 3, 8, 0, 2.0, None) == -1 and b"sigmoid_loss_grad" in lib.brats_last_error()
    assert lib.brats_sigmoid_target_prepare(p, None, None, p, 1, 3, 8, None) == -1 and b"sigmoid_target_prepare" in lib.brats_last_error()
    for k in (0, 17):
        assert lib.brats_sigmoid_loss_stats(p, p, None, p, p, 1, k, 8, 0, 2.0, None) == -1 and b"classes" in lib.brats_last_error()
        assert lib.brats_sigmoid_target_prepare(p, p, None, p, 1, k, 8, None) == -1
    assert lib.brats_sigmoid_loss_stats(p, p, None, p, p, 1, 3, 8, 2, 2.0, None) == -1 and b"class map" in lib.brats_last_error()
    assert lib.brats_sigmoid_loss_grad(p, p, None, p, p, 1, 3, 8, 4, 2.0, None) == -1 and b"term mask" in lib.brats_last_error()
    assert lib.brats_sigmoid_loss_stats(p, p, p, p, p, 1, 3, 8, 3, 2.0, None) == -2 and b"together" in lib.brats_last_error()
