"""-m gpu: the loss end of a training step -- brats_head_fwd / brats_head_bwd (csrc/head.hip), brats_dice_stats /
brats_dice_grad and the block-ordered reduction they share with norm.hip and dist_loss.hip (csrc/dice.hip) -- beyond one
workgroup, one op at a time, in the style of tests/test_size_forms_gpu.py: inputs generated on the device from seeded
generators, the reference a float64 statement of the same operation on the same stored inputs (torch, on the device), every
check printing  worst |got - ref| / bound.

The other value tests of these kernels stop at one workgroup (tests/test_ops_gpu.py: 960 voxels per Dice plane, 64 voxels per
head).  The shapes here are the smallest that reach a second block and its slot of the partial layout, the scalar path of
voxel counts that are no multiple of 4 (planes that are not 16-byte aligned), the grid caps (512 / 2048 Dice blocks, 8192 /
1024 head blocks), ordered_sum_kernel's eight-in-flight loop beside its remainder loop (nb = 240), head_bwd_kernel's
two-voxels-in-flight loop mixed with its tail, the C > 64 head, K = 1..4, no bias, and channel-slice operands between
poisoned neighbours.  Every case asserts the launch geometry it is there for.

Tolerances are derived, not measured.
  * eps_sig(x), the relative error of the kernels' p = 1.f / (1.f + __expf(-x)), from the instructions hipcc emits for that
    expression on gfx950 (-O3 -ffp-contract=off; read from the disassembly):
        v_mul_f32 u, 0xbfb8aa3b, x      u = -x * log2(e): the constant is log2(e) rounded to f32 (relative error 2^-26.2), the
                                        product rounds once (2^-24) -> 2^u is off by the factor 2^(u * 1.22 * 2^-24), i.e. by
                                        |x| * 1.22 * 2^-24 relative
        v_exp_f32 e, u                  1 ulp (the ISA manual's figure for the transcendental unit): 2^-23
        v_add_f32 d, 1.0, e             one rounding, 2^-24; the error of e enters d scaled by e / (1 + e) <= 1
        v_div_scale / v_rcp / 4 x v_fma / v_div_fmas / v_div_fixup     the IEEE division sequence: correctly rounded, 2^-24
    sum: (1.22 |x| + 2 + 1 + 1) * 2^-24 -> eps_sig(x) = (4 + 1.25 |x|) * 2^-24, |x| cut off at 128: from |x| = 104 on p is
    exactly 0 or 1.  Below x = -88.7 v_exp_f32 overflows and p is 0 where the true value is below 2^-126: an absolute 2^-120
    per term covers that and subnormal results.
  * Dice sums over n = N * V terms t: 2^-24 * sqrt(n) * sum|t| (the sum rule of test_size_forms_gpu.py) + sum |t_i| *
    eps_sig(x_i) for sum t p, + sum p_i^2 * 2 eps_sig(x_i) for sum p^2 (d p^2 = 2 p dp); sum t^2 has the sum rule alone.
  * Dice gradient, per element: (|a t| + |b2| p) * p * (3 eps_sig(x) + 2^-22): p enters the first factor, the second and --
    as an absolute error -- 1 - p; 2^-22 for the five roundings of the expression.
  * exact-count cases (x = 0, t = 1: p = 0.5 exactly; dout = 1, x = 1 for the heads): every partial is an integer or a
    multiple of 0.25 below 2^24, so the sums are asserted with ==.
  * end to end: loss within max(4 x the error of the same loss evaluated by torch in f32 against f64, 1e-6 relative), the
    bar of tests/test_distance_losses_gpu.py; gradients rtol 1e-4, atol 1e-9 against f64, the bar of tests/test_ops_gpu.py.
  * head logits (f32): 2^-24 * sqrt(n) * M, M = sum_c |w_c x_c| + |b| in f64, n = C + 1 (the sum rule).  A plain f32
    evaluation of the same dot products in torch on the CPU stays within it at every shape here (worst 0.3 - 0.8 of it) but
    the forward-cap shape, whose 6.4 million logits reach 1.13 (matmul) and 1.28 (channel by channel) of it: that one case
    uses the deterministic n * 2^-24 * M.
  * head dx: an element stored in 16 bits max(ulp16 * |ref|, smallest storage step) + 2^-22 * M, in f32 2^-21 * M,
    M = sum_k |g_k w_kc| (the element rule of test_size_forms_gpu.py, fp16's subnormal floor included); dw, db: the sum rule
    with n = N * V, dout given a positive offset so that sum t is comparable to sum|t|.

Not reached: the MFMA head's fallback to the plain kernel at voxels * pitch * 2 >= 2^31 bytes needs an activation buffer of
more than 2 GB and is left untested.

The fp16 head with weights of N(0, 1) * 2^-9 is the case of the fp16 weight split (csrc/head.hip): without the power-of-two
scale in front of the three-term split the mid and lo terms fall into half's subnormals and every logit carries up to
2^-25 * sum|x_c|.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
ULP16 = {BF: 2.0 ** -8, HF: 2.0 ** -11}
STEP_MIN = {BF: 0.0, HF: 2.0 ** -24}   # fp16 is subnormal below 2^-14: the storage step stops shrinking at 2^-24
P_FLOOR = 2.0 ** -120                  # absolute error of p where v_exp_f32 overflows / the result is subnormal
NAN = float("nan")


@pytest.fixture(autouse=True)
def _release():
    yield
    torch.cuda.empty_cache()  # (float64 copies of up to 70 MB of activations per case)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _gen(seed):
    return torch.Generator(device=_dev()).manual_seed(seed)


def _report(name, ratio, got):
    worst = float(ratio.max())
    print(f"  {name}: worst |got - ref| / bound = {worst:.3f}")
    assert bool(torch.isfinite(got).all()), name
    assert worst <= 1.0, (name, worst)


# =====================================================================================================================
# A. Dice kernels and the ordered sum
# =====================================================================================================================
DICE_SHAPES = {  # N, K, shape, blocks of the stats launch, blocks of the grad launch
    "ragged": (2, 3, (5, 7, 9), 1, 1),               # 315 voxels: % 4 == 3, planes off 16-byte alignment, scalar path
    "tiny": (2, 3, (1, 1, 3), 1, 1),                 # 3 voxels: less than one 16-byte vector
    "two_blocks": (2, 3, (11, 13, 53), 2, 2),        # 7579 voxels: the second block's slot of the [n][block][K][3] partials
    "mixed_sum": (3, 3, (40, 86, 95), 80, 80),       # 326,800 voxels: nb = 240 partial vectors, total = 9 entries
    "stats_cap": (1, 2, (130, 128, 128), 512, 520),  # 2,129,920 voxels: gx = 520 capped to 512, a second trip for some blocks
    "grad_cap": (1, 1, (208, 208, 200), 512, 2048),  # 8,652,800 voxels: gx = 2112 capped to 2048 in the gradient launch
}


def _dice_gx(vox, cap):
    """csrc/dice.hip: gx = ((voxels / 4 + 255) / 256) / 4, at least 1, at most the cap."""
    return min(max((vox // 4 + 255) // 256 // 4, 1), cap)


def _dice_case(case):
    n, k, shape, gs, gg = DICE_SHAPES[case]
    vox = shape[0] * shape[1] * shape[2]
    assert (_dice_gx(vox, 512), _dice_gx(vox, 2048)) == (gs, gg), f"{case}: the launch geometry is not what the case is for"
    return n, k, shape, vox


def _dice_inputs(seed, n, k, shape):
    """logits 3 * N(0, 1) clamped to +-12, targets rand > 0.6 as f32"""
    g = _gen(seed)
    x = torch.randn((n, k, *shape), generator=g, device=_dev()).mul_(3.0).clamp_(-12.0, 12.0)
    t = (torch.rand((n, k, *shape), generator=g, device=_dev()) > 0.6).float()
    return x, t


def _dice_stats(x, t, want_ws=False):
    """brats_dice_stats -> [K, 3] (and the workspace of per-block partials [n][block][K][3]); both start as NaN so that a slot
    read before it is written shows."""
    from brats21_amd import _lib, ops
    lib = _lib.lib()
    n, k = x.shape[:2]
    sums = torch.full((k, 3), NAN, device=x.device)
    ws = torch.full((lib.brats_dice_ws_floats(n, k),), NAN, device=x.device)
    _lib.check(lib.brats_dice_stats(x.data_ptr(), t.data_ptr(), sums.data_ptr(), ws.data_ptr(), n, k, x[0, 0].numel(), ops._stream()),
               "dice_stats")
    return (sums, ws) if want_ws else sums


def _dice_grad(x, t, coef):
    """brats_dice_grad with coef [K, 2] f32 = (dL/dI, dL/dP2); dx starts as NaN."""
    from brats21_amd import _lib, ops
    n, k = x.shape[:2]
    dx = torch.full_like(x, NAN)
    _lib.check(_lib.lib().brats_dice_grad(x.data_ptr(), t.data_ptr(), coef.data_ptr(), dx.data_ptr(), n, k, x[0, 0].numel(), ops._stream()),
               "dice_grad")
    return dx


def _eps_sig(x64):
    return (4.0 + 1.25 * x64.abs().clamp(max=128.0)) * 2.0 ** -24


def _sums_ref(x, t):
    """f64 [K, 3] sums and their tolerance (module docstring)."""
    n = x.shape[0] * x[0, 0].numel()
    x64, t64 = x.double(), t.double()
    p, e = torch.sigmoid(x64), _eps_sig(x64)
    ax = (0, 2, 3, 4)
    tp, pp, tt = t64 * p, p * p, t64 * t64
    ref = torch.stack([tp.sum(ax), pp.sum(ax), tt.sum(ax)], -1)
    rule = 2.0 ** -24 * math.sqrt(n)
    tol = torch.stack([tp.sum(ax) * rule + (tp * e).sum(ax) + n * P_FLOOR, pp.sum(ax) * rule + (pp * e).sum(ax) * 2.0 + n * P_FLOOR,
                       tt.sum(ax) * rule], -1)
    return ref, tol


def _check_sums(name, got, x, t):
    ref, tol = _sums_ref(x, t)
    _report(name, (got.double() - ref).abs() / tol.clamp_min(1e-300), got)


def _grad_ref(x, t, coef):
    """f64 dx = (a t + b2 p) p (1 - p) with the f32 coefficients as given, and the per-element bound."""
    k = x.shape[1]
    x64, t64 = x.double(), t.double()
    p, e = torch.sigmoid(x64), _eps_sig(x64)
    a = coef[:, 0].double().view(1, k, 1, 1, 1)
    b2 = 2.0 * coef[:, 1].double().view(1, k, 1, 1, 1)
    ref = (a * t64 + b2 * p) * p * (1.0 - p)
    bound = ((a * t64).abs() + b2.abs() * p) * (p * (3.0 * e + 2.0 ** -22) + P_FLOOR)
    return ref, bound


def _loss_coef(x, t):
    """The coefficients the Dice loss hands to the gradient kernel at these inputs (f64 algebra, cast to f32)."""
    x64, t64 = x.double(), t.double()
    p = torch.sigmoid(x64)
    ax = (0, 2, 3, 4)
    inter, den = (t64 * p).sum(ax), (t64 * t64).sum(ax) + (p * p).sum(ax) + 1e-5
    k = x.shape[1]
    return torch.stack([-2.0 / den / k, (2.0 * inter + 1e-5) / den ** 2 / k], -1).float().contiguous()


@pytest.mark.parametrize("case", list(DICE_SHAPES))
def test_dice_stats_raw_sums(case):
    """brats_dice_stats called directly: { sum t p, sum p^2, sum t^2 } per class against f64."""
    n, k, shape, _ = _dice_case(case)
    x, t = _dice_inputs(201, n, k, shape)
    _check_sums(f"sums {case}", _dice_stats(x, t), x, t)


@pytest.mark.parametrize("case", [c for c in DICE_SHAPES if c != "tiny"])
def test_dice_exact_count(case):
    """x = 0, t = 1: p = 0.5, every partial is exact, so sums == { 0.5, 0.25, 1 } * N * V and dx == one constant everywhere:
    a dropped or doubled block, partial slot or tail element cannot hide."""
    n, k, shape, vox = _dice_case(case)
    x = torch.zeros((n, k, *shape), device=_dev())
    t = torch.ones_like(x)
    got = _dice_stats(x, t)
    want = torch.tensor([0.5, 0.25, 1.0], dtype=torch.float64, device=x.device).mul(n * vox).expand(k, 3)
    assert n * vox < 2 ** 24
    print(f"  sums {case}: got {got[0].tolist()} want {want[0].tolist()}")
    assert torch.equal(got.double(), want), (case, got.tolist())
    g = _gen(202)
    coef = torch.stack([-(0.5 + torch.rand(k, generator=g, device=x.device)), 0.5 + torch.rand(k, generator=g, device=x.device)], -1).mul_(1e-3).contiguous()
    dx = _dice_grad(x, t, coef)
    const = ((coef[:, 0] * 1.0 + (2.0 * coef[:, 1]) * 0.5) * 0.5 * 0.5).view(1, k, 1, 1, 1)  # the kernel's f32 expression: one rounding
    assert torch.equal(dx, const.expand_as(dx)), case


@pytest.mark.parametrize("case", list(DICE_SHAPES))
def test_dice_grad(case):
    """brats_dice_grad called directly with the loss's coefficients at these inputs handed in as f32, against f64 with the
    same coefficients, per element."""
    n, k, shape, _ = _dice_case(case)
    x, t = _dice_inputs(203, n, k, shape)
    coef = _loss_coef(x, t)
    dx = _dice_grad(x, t, coef)
    ref, bound = _grad_ref(x, t, coef)
    print(f"  largest |gradient| {float(ref.abs().max()):.2e}")
    _report(f"dx {case}", (dx.double() - ref).abs_().div_(bound.clamp_min_(1e-300)), dx)


def test_dice_extreme_logits():
    """A ragged plane mixing +-30, +-90, +-inf and 0: finite sums within the bound; the gradient is exactly 0 where p is 0 or 1
    (+30: 1 + e^-30 rounds to 1; +-90 and +-inf: v_exp_f32 under- / overflows) and within its bound elsewhere."""
    n, k, shape = 1, 2, (3, 5, 7)
    inf = float("inf")
    vals = torch.tensor([30.0, -30.0, 90.0, -90.0, inf, -inf, 0.0], device=_dev())
    i = torch.arange(n * k * 105, device=_dev())
    x = vals[(i * 3 + i // 7) % 7].view(n, k, *shape).contiguous()
    t = ((i % 3) != 1).float().view(n, k, *shape).contiguous()
    for v in vals.tolist():
        assert bool(((x == v) & (t == 1)).any()) and bool(((x == v) & (t == 0)).any()), v
    _check_sums("sums extreme", _dice_stats(x, t), x, t)
    coef = torch.tensor([[-3e-3, 1e-3], [-2e-3, 4e-3]], device=x.device)
    dx = _dice_grad(x, t, coef)
    ref, bound = _grad_ref(x, t, coef)
    _report("dx extreme", (dx.double() - ref).abs() / bound.clamp_min(1e-300), dx)
    saturated = (x == 30.0) | (x.abs() >= 90.0)
    assert bool((dx[saturated] == 0.0).all()), "the gradient is not exactly 0 where p is 0 or 1"
    assert bool((dx[~saturated] != 0.0).all())


def _closed_form_case():
    """An aligned two-block case that no random generator enters (7680 voxels per plane: gx = 2)."""
    n, k, shape = 2, 3, (12, 16, 40)
    i = torch.arange(n * k * 7680, device=_dev(), dtype=torch.int64)
    x = (((i * 7919) % 2001 - 1000).float() / 128.0).view(n, k, *shape).contiguous()
    t = (((i * 31) % 5) < 2).float().view(n, k, *shape).contiguous()
    coef = torch.tensor([[-3.0e-4, 1.0e-4], [-6.0e-4, 2.5e-4], [-9.0e-4, 4.0e-4]], dtype=torch.float32, device=_dev())
    return i, x, t, coef


def test_dice_aligned_shapes_keep_their_order_of_addition():
    """An aligned shape takes the 16-byte path as before: the batch route (N = 2) and the per-sample route of
    losses._DiceFn(batch=False) (N = 1 on each sample's slice, itself 16-byte aligned) give the same block partials and the
    same dx bit for bit, and the [K, 3] sums are those partials added in block order in f32 -- ordered_sum_kernel's
    contract for nb <= 32 -- on either route."""
    assert _dice_gx(7680, 512) == 2
    _, x, t, coef = _closed_form_case()
    n, k = x.shape[:2]
    assert x.data_ptr() % 16 == 0 and t.data_ptr() % 16 == 0 and (k * 7680 * 4) % 16 == 0
    sums, ws = _dice_stats(x, t, want_ws=True)
    part = ws[:n * 2 * k * 3].view(n * 2, k, 3).clone()
    _check_sums("sums closed form", sums, x, t)
    per_sample = []
    for s in range(n):
        s_i, ws_i = _dice_stats(x[s:s + 1], t[s:s + 1], want_ws=True)
        p_i = ws_i[:2 * k * 3].view(2, k, 3).clone()
        assert torch.equal(s_i, p_i[0] + p_i[1]), f"sample {s}: sums != partials added in block order"
        per_sample.append(p_i)
        assert torch.equal(_dice_grad(x[s:s + 1], t[s:s + 1], coef), _dice_grad(x, t, coef)[s:s + 1]), f"sample {s}: dx differs between the routes"
    assert torch.equal(part, torch.cat(per_sample)), "the block partials differ between the routes"
    acc = part[0]
    for b in range(1, n * 2):
        acc = acc + part[b]
    assert torch.equal(sums, acc), "batch sums != partials added in block order"


def _dice_torch(x, t, jaccard, batch, eps=1e-5):
    """monai DiceLoss(sigmoid, squared_pred, smooth 1e-5, reduction mean) in the dtype of x, batch = True / False"""
    p = torch.sigmoid(x)
    ax = (0, 2, 3, 4) if batch else (2, 3, 4)
    inter = (t * p).sum(ax)
    den = (t * t).sum(ax) + (p * p).sum(ax)
    if jaccard:
        den = 2.0 * (den - inter)
    return (1.0 - (2.0 * inter + eps) / (den + eps)).mean()


E2E_MODES = ["fused", "fused_jaccard", "sigmoid_dice_per_sample", "sigmoid_dice_batch"]


@pytest.mark.parametrize("mode", E2E_MODES)
@pytest.mark.parametrize("case", ["ragged", "two_blocks"])
def test_dice_end_to_end(case, mode):
    """fused_deep_supervision_dice over three heads (plain, Jaccard) and losses._SigmoidDice (batch = False: one call per
    sample on its slice, whose planes start off 16-byte alignment when K * V % 4 != 0; batch = True) against f64 autograd."""
    from brats21_amd import losses
    n, k, shape, _ = _dice_case(case)
    fused = mode.startswith("fused")
    jaccard = mode == "fused_jaccard"
    batch = fused or mode == "sigmoid_dice_batch"
    heads = []
    for h in range(3 if fused else 1):
        x, t = _dice_inputs(210 + h, n, k, shape)  # (the target of the first head is the one used)
        heads.append(x)
        if h == 0:
            target = t
    xs = [h.clone().requires_grad_(True) for h in heads]
    if fused:
        loss = losses.fused_deep_supervision_dice((xs[0], xs[1:]), target, jaccard=jaccard)
    else:
        loss = losses._SigmoidDice("test", True, True, False, 1e-5, 1e-5, batch)(xs[0], target)
    grads = torch.autograd.grad(loss, xs)
    x64 = [h.double().requires_grad_(True) for h in heads]
    ref = torch.stack([_dice_torch(h, target.double(), jaccard, batch) for h in x64]).mean()
    g64 = torch.autograd.grad(ref, x64)
    f32 = torch.stack([_dice_torch(h, target, jaccard, batch) for h in heads]).mean()
    f64 = float(ref)
    ref_err = abs(float(f32.double()) - f64) / abs(f64)
    bar = max(4.0 * ref_err, 1e-6)
    err = abs(float(loss.double()) - f64) / abs(f64)
    print(f"  loss {case} {mode}: {float(loss):.8f} vs float64 {f64:.10f}: relative error {err:.2e} / bar {bar:.2e} = {err / bar:.3f} "
          f"(torch f32's own error {ref_err:.2e})")
    assert err <= bar, (err, bar)
    worst = max(float(((g.double() - w).abs() / (1e-9 + 1e-4 * w.abs())).max()) for g, w in zip(grads, g64))
    print(f"  gradients {case} {mode}: worst |got - ref| / (1e-9 + 1e-4 |ref|) = {worst:.3f}")
    for g, w in zip(grads, g64):
        torch.testing.assert_close(g, w.float(), rtol=1e-4, atol=1e-9)


# =====================================================================================================================
# B. Heads (scale = 1: the up-sampling is pinned bit for bit by tests/test_memory_passes_gpu.py)
# =====================================================================================================================
def _head_fwd(x, w, b):
    """brats_head_fwd at scale 1 on an NDHWC tensor or channel-slice view -> f32 logits [N, K, D, H, W] (NaN before the call)"""
    from brats21_amd import _lib, ops
    ptr, c, p = ops._desc(x)
    n, d, h, wd, _ = x.shape
    k = w.shape[0]
    out = torch.full((n, k, d, h, wd), NAN, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().brats_head_fwd(ptr, p, w.data_ptr(), b.data_ptr() if b is not None else None, None, out.data_ptr(),
                                         ops._code(x.dtype), n, c, k, d, h, wd, 1, ops._stream()), "head_fwd")
    return out


def _head_bwd(x, w, dout, dx=None):
    """brats_head_bwd at scale 1; dx: None (not wanted) or the NDHWC tensor / channel-slice view it is written into.
    -> (dw [K, C], db [K]); workspace and results are NaN before the call."""
    from brats21_amd import _lib, ops
    lib = _lib.lib()
    ptr, c, p = ops._desc(x)
    n, d, h, wd, _ = x.shape
    k = w.shape[0]
    ws = torch.full((lib.brats_head_bwd_ws_bytes(n, c, k, d, h, wd, 1) // 4,), NAN, dtype=torch.float32, device=x.device)
    dw = torch.full((k, c), NAN, dtype=torch.float32, device=x.device)
    db = torch.full((k,), NAN, dtype=torch.float32, device=x.device)
    dptr, dp = (None, c) if dx is None else (ops._desc(dx)[0], ops._desc(dx)[2])
    _lib.check(lib.brats_head_bwd(ptr, p, w.data_ptr(), dout.data_ptr(), ws.data_ptr(), dptr, dp, dw.data_ptr(), db.data_ptr(),
                                  ops._code(x.dtype), n, c, k, d, h, wd, 1, ops._stream()), "head_bwd")
    return dw, db


def _head_inputs(seed, dtype, c, n, k, shape, wstd=0.2, bias=True):
    g = _gen(seed)
    dev = _dev()
    x = torch.randn((n, *shape, c), generator=g, device=dev).to(dtype)
    w = (torch.randn((k, c), generator=g, device=dev) * wstd).contiguous()
    b = torch.randn((k,), generator=g, device=dev) * 0.1 if bias else None
    dout = torch.randn((n, k, *shape), generator=g, device=dev).abs_().add_(0.5)
    return x, w, b, dout


def _bwd_geometry(dtype, c, vox):
    """csrc/head.hip brats_head_bwd: voxels per block trip and blocks per sample"""
    vl = 256 // (c // (4 if dtype == F32 else 8))
    return vl, min(max(-(-vox // (vl * 16)), 1), 1024)


def _check_logits(name, logits, x, w, b, deterministic=False):
    n, k = logits.shape[:2]
    c = x.shape[-1]
    x64, w64 = x.double().reshape(n, -1, c), w.double()
    ref = (x64 @ w64.t()).transpose(1, 2)
    m = (x64.abs() @ w64.abs().t()).transpose(1, 2)
    if b is not None:
        ref = ref + b.double().view(1, k, 1)
        m = m + b.double().abs().view(1, k, 1)
    bound = m * (2.0 ** -24 * ((c + 1) if deterministic else math.sqrt(c + 1)))
    _report(name, (logits.double().reshape(n, k, -1) - ref).abs_().div_(bound.clamp_min_(1e-300)), logits)


def _check_bwd(name, dtype, x, w, dout, dx, dw, db):
    n, k = dout.shape[:2]
    c = x.shape[-1]
    x64, w64, g64 = x.double().reshape(n, -1, c), w.double(), dout.double().reshape(n, k, -1)
    vox = x64.shape[1]
    if dx is not None:
        ref = g64.transpose(1, 2) @ w64
        m = g64.abs().transpose(1, 2) @ w64.abs()
        bound = m * (2.0 ** -21 if dtype == F32 else 2.0 ** -22)
        if dtype != F32:
            bound += (ref.abs() * ULP16[dtype]).clamp_min_(STEP_MIN[dtype])
        _report(f"dx {name}", (dx.double().reshape(n, vox, c) - ref).abs_().div_(bound.clamp_min_(1e-300)), dx)
        del ref, m, bound
    rule = 2.0 ** -24 * math.sqrt(n * vox)
    ref = (g64 @ x64).sum(0)
    tol = (g64.abs() @ x64.abs()).sum(0) * rule
    _report(f"dw {name}", (dw.double() - ref).abs() / tol.clamp_min(1e-300), dw)
    ref = g64.sum((0, 2))
    _report(f"db {name}", (db.double() - ref).abs() / (g64.abs().sum((0, 2)) * rule), db)


ODD = (9, 11, 13)   # 1287 voxels: neither a multiple of 64 nor of 16
HEAD_CASES = (
    [("odd_trips", dt, 48, 2, 3, ODD, 0.2, True) for dt in (BF, HF, F32)]
    + [(f"k{k}", dt, 16, 1, k, (6, 7, 9), 0.2, k != 2) for k in (1, 2, 3, 4) for dt in (BF, HF, F32)]
    + [("wide", dt, 96, 2, 3, (8, 10, 12), 0.2, True) for dt in (BF, HF)]
    + [("small_weights", dt, 48, 2, 3, ODD, 2.0 ** -9, True) for dt in (BF, HF)]
)


@pytest.mark.parametrize("name,dtype,c,n,k,shape,wstd,bias", HEAD_CASES, ids=[f"{c[0]}-{str(c[1])[6:]}" for c in HEAD_CASES])
def test_head_values(name, dtype, c, n, k, shape, wstd, bias):
    """brats_head_fwd / brats_head_bwd against f64.  odd_trips: the MFMA forward's 21 waves on gx = 5 blocks (one wave takes a
    second trip, the last chunk is ragged), the backward's two-voxels-in-flight loop mixed with its tail on 2 (16-bit: vl =
    42, four idle threads) or 4 (f32: vl = 21) blocks; k1..k4: the HEAD_KMAX guards, K = 2 without a bias; wide: C > 64, the
    plain 16-bit kernel; small_weights: weights of N(0, 1) * 2^-9, the fp16 three-term split."""
    vox = shape[0] * shape[1] * shape[2]
    if name == "odd_trips":
        vl, gx = _bwd_geometry(dtype, c, vox)
        assert (vl, gx) == ((21, 4) if dtype == F32 else (42, 2)) and 256 % (c // (4 if dtype == F32 else 8)) == 4
        trips = [len(range(blk * vl + lane, vox, gx * vl)) for blk in range(gx) for lane in range(vl)]
        assert any(t >= 2 for t in trips) and any(t % 2 for t in trips), "both the two-in-flight loop and the tail must run"
        assert -(-vox // 64) == 21 and max(-(-vox // 64) // 4, 1) == 5 and vox % 16
    x, w, b, dout = _head_inputs(300 + c + k, dtype, c, n, k, shape, wstd, bias)
    tag = f"{name} {str(dtype)[6:]}"
    _check_logits(f"logits {tag}", _head_fwd(x, w, b), x, w, b)
    dx = torch.full_like(x, NAN)
    dw, db = _head_bwd(x, w, dout, dx)
    _check_bwd(tag, dtype, x, w, dout, dx, dw, db)


@pytest.mark.parametrize("dtype,shape", [(BF, (96, 96, 80)), (F32, (72, 72, 72))], ids=["bfloat16", "float32"])
def test_head_backward_cap(dtype, shape):
    """More voxels than HEAD_MAX_BLOCKS = 1024 blocks take at 16 trips each (737,280 > 672 * 1024; f32 373,248 > 336 * 1024):
    every block walks further, 1024 partial vectors go through ordered_sum2.  Values against f64, then dout = 1, x = 1:
    db == dw == V exactly."""
    c, n, k = 48, 1, 3
    vox = shape[0] * shape[1] * shape[2]
    vl, gx = _bwd_geometry(dtype, c, vox)
    assert gx == 1024 and vox > vl * 16 * 1024
    x, w, b, dout = _head_inputs(320, dtype, c, n, k, shape)
    dx = torch.full_like(x, NAN)
    dw, db = _head_bwd(x, w, dout, dx)
    _check_bwd(f"cap {str(dtype)[6:]}", dtype, x, w, dout, dx, dw, db)
    del dx
    dw, db = _head_bwd(torch.ones_like(x), w, torch.ones_like(dout), None)
    assert n * vox < 2 ** 24
    print(f"  exact count: db {db.tolist()} dw in [{float(dw.min())}, {float(dw.max())}] want {n * vox}")
    assert bool((db == n * vox).all()) and bool((dw == n * vox).all())


def test_head_forward_cap():
    """2,129,920 voxels > 8192 blocks * 4 waves * 64: the MFMA head's grid cap, a second trip for 512 of the 32768 waves.
    (6.4 million logits: the deterministic n * 2^-24 * M, see the module docstring.)"""
    c, n, k, shape = 16, 1, 3, (130, 128, 128)
    vox = shape[0] * shape[1] * shape[2]
    assert -(-vox // 64) // 4 > 8192
    x, w, b, _ = _head_inputs(330, BF, c, n, k, shape)
    _check_logits("logits forward cap", _head_fwd(x, w, b), x, w, b, deterministic=True)


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bfloat16", "float16"])
def test_head_channel_slice(dtype):
    """x and dx as the 16 channels at offset 24 of pitch-48 buffers whose other channels hold NaN and +-Inf (x) or a sentinel
    (dx): logits, dx, dw and db are finite and equal the dense run's bit for bit, the dx buffer is untouched outside the
    slice; and a run that does not want dx."""
    c, off, pitch, n, k, shape = 16, 24, 48, 2, 3, (5, 6, 7)
    x, w, b, dout = _head_inputs(340, dtype, c, n, k, shape)
    tag = f"slice {str(dtype)[6:]}"
    logits = _head_fwd(x, w, b)
    dx = torch.full_like(x, NAN)
    dw, db = _head_bwd(x, w, dout, dx)
    _check_logits(f"logits {tag}", logits, x, w, b)
    _check_bwd(tag, dtype, x, w, dout, dx, dw, db)
    buf = torch.empty((n, *shape, pitch), dtype=dtype, device=x.device)
    buf[..., 0::3] = NAN
    buf[..., 1::3] = float("inf")
    buf[..., 2::3] = float("-inf")
    buf[..., off:off + c] = x
    xs = buf[..., off:off + c]
    assert not bool(torch.isfinite(buf[..., :off].float()).any()) and not bool(torch.isfinite(buf[..., off + c:].float()).any())
    dxbuf = torch.full((n, *shape, pitch), 7.0, dtype=dtype, device=x.device)
    logits_s = _head_fwd(xs, w, b)
    dw_s, db_s = _head_bwd(xs, w, dout, dxbuf[..., off:off + c])
    for nm, a, d in (("logits", logits_s, logits), ("dx", dxbuf[..., off:off + c], dx), ("dw", dw_s, dw), ("db", db_s, db)):
        assert bool(torch.isfinite(a.float()).all()), f"{nm}: the poisoned neighbours leaked into the slice run"
        assert torch.equal(a, d), f"{nm}: slice run != dense run"
    assert bool((dxbuf[..., :off] == 7.0).all()) and bool((dxbuf[..., off + c:] == 7.0).all()), "dx was written outside its slice"
    dw_n, db_n = _head_bwd(xs, w, dout, None)
    assert torch.equal(dw_n, dw) and torch.equal(db_n, db), "want_dx = False changes dw / db"
