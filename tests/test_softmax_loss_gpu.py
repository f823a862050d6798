"""GPU tests of the exclusive-class criterion brats21_amd.losses.SoftmaxDiceCELoss (csrc/softmax_loss.hip: brats_softmax_stats,
brats_softmax_grad, brats_label_stats) against the float64 restatement tests/_softmax_ref.py.

Bar.  For each case the restatement is also evaluated in float32 on the CPU; the GPU may be at most 4 x that error away from
float64, and the bar is not set below 1e-6 relative -- the rule of the distance-map criteria (tests/test_distance_losses_gpu.py):
the margin is for the different summation order and __expf.  It is applied to the loss value (relative) and to each head's
gradient (max abs error over max abs gradient).  The measured errors are printed (pytest -s) and carried in the assertion
messages."""
import argparse
import contextlib
import io
import itertools

import numpy as np
import pytest
import torch

import _softmax_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = ((1, 1, 65),      # a single partial, scalar tail
          (16, 16, 36),    # 16-byte path, several workgroups
          (9, 37, 70),     # V % 4 != 0: scalar path, several workgroups, ragged end
          "misaligned")    # (8, 12, 20) on a view one float into its allocation: V % 4 == 0 but no plane is 16-byte aligned
LABEL_KINDS = ("random", "absent", "one_class_sample", "ignored")


def make_logits(n, k, shape, g, stress=False):
    x = torch.randn((n, k) + shape, generator=g) * 3.0
    if stress:  # +-100 at the same voxel: exp() of the raw logits overflows, the result must be finite and right
        sel = torch.rand(shape, generator=g) < 0.2
        x[:, 0][:, sel] = 100.0
        x[:, 1][:, sel] = -100.0
        sel2 = torch.rand(shape, generator=g) < 0.05
        x[:, k - 1][:, sel2] = -100.0
        x[:, 0][:, sel2] = 100.0 if k == 2 else 99.0
    return x


def make_labels(kind, n, k, shape, g):
    y = torch.randint(0, k, (n,) + shape, generator=g)
    if kind == "absent":  # one class absent from the whole batch
        y[y == k - 1] = 0
    elif kind == "one_class_sample":  # one sample entirely one class
        y[n - 1] = 1
    elif kind == "ignored":  # 10 % unlabelled
        y[torch.rand((n,) + shape, generator=g) < 0.1] = 255
    return y.to(torch.uint8)


def on_device(x, misaligned=False):
    """the logits on the GPU; misaligned: a contiguous view that starts one float into its allocation"""
    if not misaligned:
        return x.to(DEV)
    buf = torch.empty(x.numel() + 1, dtype=torch.float32, device=DEV)
    view = buf[1:].view(x.shape)
    view.copy_(x)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def run_gpu(criterion, heads, labels, prepared=True, misaligned=False):
    from brats21_amd import losses
    xs = [on_device(h, misaligned).requires_grad_(True) for h in heads]
    y = labels.to(DEV)
    if len(xs) == 1:
        loss = criterion(xs[0], y)
    else:
        fn = losses.deep_supervision_prepared_loss if prepared else losses.deep_supervision_loss
        loss, main = fn(criterion, (xs[0], xs[1:]), y)
        assert main is xs[0]
    loss.backward()
    return loss.detach(), [x.grad for x in xs]


def check_case(what, heads, labels, report, misaligned=False, **options):
    from brats21_amd import losses
    f64, g64 = R.deep_loss_and_grads(heads, labels, torch.float64, **options)
    f32, g32 = R.deep_loss_and_grads(heads, labels, torch.float32, **options)
    loss, grads = run_gpu(losses.SoftmaxDiceCELoss(**options), heads, labels, misaligned=misaligned)
    assert np.isfinite(f64) and bool(torch.isfinite(loss)) and loss.dtype == torch.float32
    ref_err = abs(f32 - f64) / abs(f64)
    bar = max(4.0 * ref_err, 1e-6)
    err = abs(float(loss.double()) - f64) / abs(f64)
    lines = [f"{what}: value {float(loss):.8f} vs float64 {f64:.10f}: rel err {err:.2e} (bar {bar:.2e}, float32 CPU {ref_err:.2e})"]
    ok = err <= bar
    for i, (g, w64, w32) in enumerate(zip(grads, g64, g32)):
        assert g.dtype == torch.float32 and g.shape == w64.shape and bool(torch.isfinite(g).all())
        scale = float(w64.abs().max())
        ref_g = float((w32.double() - w64).abs().max()) / scale
        gbar = max(4.0 * ref_g, 1e-6)
        gerr = float((g.cpu().double() - w64).abs().max()) / scale
        lines.append(f"   head {i}: gradient max err / max {gerr:.2e} (bar {gbar:.2e}, float32 CPU {ref_g:.2e})")
        ok = ok and gerr <= gbar
    report.extend(lines)
    print("\n" + "\n".join(lines))
    assert ok, lines


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("k", [2, 3, 5, 16])
def test_value_and_gradient_match_float64(k, n):
    g = torch.Generator().manual_seed(1000 * k + n)
    report = []
    for shape in SHAPES:
        mis = shape == "misaligned"
        sp = (8, 12, 20) if mis else shape
        for kind in LABEL_KINDS:
            check_case(f"K={k} N={n} {shape} labels {kind}", [make_logits(n, k, sp, g)], make_labels(kind, n, k, sp, g), report, misaligned=mis)
        check_case(f"K={k} N={n} {shape} +-100 logits", [make_logits(n, k, sp, g, stress=True)], make_labels("random", n, k, sp, g), report,
                   misaligned=mis)


@pytest.mark.parametrize("squared_pred,jaccard,batch,include_background", list(itertools.product([True, False], repeat=4)))
def test_options_on_two_heads(squared_pred, jaccard, batch, include_background):
    g = torch.Generator().manual_seed(77)
    n, k, shape = 3, 3, (9, 37, 70)
    heads = [make_logits(n, k, shape, g), make_logits(n, k, shape, g)]
    labels = make_labels("ignored", n, k, shape, g)
    weights = dict(lambda_dice=0.7, lambda_ce=1.3, smooth_nr=1e-3, smooth_dr=1e-4) if jaccard != batch else {}
    check_case(f"squared_pred={squared_pred} jaccard={jaccard} batch={batch} include_background={include_background} {weights}", heads, labels,
               [], squared_pred=squared_pred, jaccard=jaccard, batch=batch, include_background=include_background, **weights)


def _three_heads():
    g = torch.Generator().manual_seed(5)
    n, k, shape = 2, 5, (9, 37, 70)
    return [make_logits(n, k, shape, g) for _ in range(3)], make_labels("ignored", n, k, shape, g)


def test_prepared_target_is_bit_equal_and_runs_are_deterministic():
    from brats21_amd import losses
    heads, labels = _three_heads()
    crit = losses.SoftmaxDiceCELoss(batch=False)
    la, ga = run_gpu(crit, heads, labels, prepared=True)
    lb, gb = run_gpu(crit, heads, labels, prepared=False)
    assert torch.equal(la, lb) and all(torch.equal(a, b) for a, b in zip(ga, gb))
    la2, ga2 = run_gpu(crit, heads, labels, prepared=True)  # no float atomics anywhere: bit-reproducible
    assert torch.equal(la, la2) and all(torch.equal(a, b) for a, b in zip(ga, ga2))
    prep = crit.prepare(labels.to(DEV))
    assert isinstance(prep, losses.PreparedTarget) and prep.labels.dtype == torch.uint8
    counts, valid = prep.stats(5)
    want = torch.stack([(labels == c).flatten(1).sum(1) for c in range(5)], 1).float()
    assert torch.equal(counts.cpu(), want) and torch.equal(valid.cpu(), want.sum(1))
    with pytest.raises(ValueError):
        losses.SoftmaxDiceCELoss()(heads[0].to(DEV), prep)  # made by another criterion


def test_target_forms_give_the_same_result():
    """[N, 1, D, H, W] or [N, D, H, W], any integer or float dtype, or the one-hot [N, K, D, H, W]."""
    from brats21_amd import losses
    g = torch.Generator().manual_seed(9)
    n, k, shape = 2, 4, (5, 6, 8)
    x = make_logits(n, k, shape, g).to(DEV)
    y = make_labels("random", n, k, shape, g).to(DEV)
    crit = losses.SoftmaxDiceCELoss()
    base = crit(x, y)
    forms = {"u8 [N,1,...]": y[:, None], "int64": y.long(), "int32 [N,1,...]": y.int()[:, None], "float32": y.float()[:, None],
             "float64": y.double(), "one-hot": torch.nn.functional.one_hot(y.long(), k).movedim(-1, 1).float()}
    for name, t in forms.items():
        assert torch.equal(crit(x, t), base), name
    # -1 and 300 are no class: ignored like 255
    yi = y.long()
    yi[0, 0, 0, :4] = torch.tensor([-1, 300, 255, k], device=DEV)
    y255 = yi.clone()
    y255[0, 0, 0, :4] = 255
    assert torch.equal(crit(x, yi), crit(x, y255.to(torch.uint8)))


def test_no_label_value_can_fault():
    """Every value 0 .. 255 with K = 3: the same loss and gradient as with every value >= 3 replaced by 255."""
    from brats21_amd import losses
    g = torch.Generator().manual_seed(11)
    n, k, shape = 2, 3, (4, 16, 16)
    labels = torch.arange(256, dtype=torch.uint8).repeat(n * 4).reshape((n,) + shape)
    labels = labels.flatten()[torch.randperm(labels.numel(), generator=g)].reshape((n,) + shape)
    assert len(torch.unique(labels)) == 256
    heads = [make_logits(n, k, shape, g)]
    crit = losses.SoftmaxDiceCELoss()
    la, ga = run_gpu(crit, heads, labels)
    lb, gb = run_gpu(crit, heads, R.ignore_above(labels, k))
    assert torch.equal(la, lb) and torch.equal(ga[0], gb[0])
    ignored = (labels >= k).to(DEV)
    assert float(ga[0].movedim(1, -1)[ignored].abs().max()) == 0.0  # no gradient on an ignored voxel
    check_case("labels 0..255, K=3", heads, R.ignore_above(labels, k), [])


def test_other_logit_dtypes_are_upcast():
    from brats21_amd import losses
    heads, labels = _three_heads()
    crit = losses.SoftmaxDiceCELoss()
    xb = heads[0].to(DEV).bfloat16().requires_grad_(True)
    lb = crit(xb, labels.to(DEV))
    lb.backward()
    xf = xb.detach().float().requires_grad_(True)
    lf = crit(xf, labels.to(DEV))
    lf.backward()
    assert xb.grad.dtype == torch.bfloat16 and torch.equal(lb, lf) and torch.equal(xb.grad, xf.grad.bfloat16())


def test_graphed_train_step_replays_the_eager_losses():
    """A width-8 EquiUnet(num_classes=4) step with the criterion captured into one hipGraph: three replays reproduce the losses
    of three eager steps -- nothing in the criterion reads the host (the valid-voxel count is a device scalar)."""
    from brats21_amd import get_model, losses
    from brats21_amd.engine import GraphedTrainStep, TrainStep
    from brats21_amd.optim import Ranger2020
    from oracle import synth
    ns = argparse.Namespace(model="equiunet", width=8, norm="group", act="relu", num_classes=4, dropout=0)
    size = (32, 32, 32)
    xs = [synth.random_image(1, 4, size, seed=40 + i).to(DEV) for i in range(3)]
    ts = [synth.nested_spheres(1, size).sum(1, keepdim=True).to(DEV).roll(i, dims=-1) for i in range(3)]  # labels 0 .. 3, new every step
    assert sorted(torch.unique(ts[0]).tolist()) == [0.0, 1.0, 2.0, 3.0]
    ts[1][..., :2] = 255.0  # some unlabelled voxels in one step: the count changes between replays
    results = []
    for graphed in (False, True):
        torch.manual_seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            m = get_model(ns).to(DEV).train()
        opt = Ranger2020(m.parameters(), lr=1e-3, weight_decay=1e-5, use_gc=True, capturable=graphed)
        step = TrainStep(m, opt, criterion=losses.SoftmaxDiceCELoss(), amp=True)
        if graphed:
            step = GraphedTrainStep(step, warmup=2)  # the first call: two eager warm-up steps on batch 0, the capture, one replay
            got = [float(step(x, t).detach()) for x, t in zip(xs, ts)]
        else:
            got = [float(step(x, t).detach()) for x, t in zip([xs[0]] * 2 + xs, [ts[0]] * 2 + ts)][2:]
        torch.cuda.synchronize()
        results.append(got)
    assert len(results[1]) == 3 and all(np.isfinite(results[1]))
    assert len(set(results[0])) == 3  # the three steps differ: a replay that baked one target in would not follow them
    np.testing.assert_allclose(results[0], results[1], rtol=1e-5, atol=1e-6)
