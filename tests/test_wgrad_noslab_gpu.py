"""-m gpu: the no-slab weight-gradient form (csrc/conv_wgrad.hip, conv_wgrad_noslab_kernel<DIL>): a workgroup owns 48 co x 16 ci
x 27 taps of dW over the whole batch and writes them once into dw -- no split-K slabs, no reduction launch.

1. exactness on the integer operands of tests/_conv_exact_ref.py (bit for bit), bf16 and fp16, with channel-slice views and
   with `out=` inside a larger buffer whose neighbours must stay untouched (16-byte aligned: the 16-byte store path; not
   aligned: the 4-byte path);
2. accuracy on normal operands against float64, next to the slab form's (switch 0 = the arithmetic before this form existed):
   new <= 2 x slab.  The kernel walks the tiles in the slab plan's groups and adds the groups in the reduction's order, so
   beyond that bound dW has the slab form's very bits (a training run must not change when the rule takes the form): asserted
   on the layers the rule takes.  Measured (MI355X): profiles/wgrad_noslab_tests.txt;
3. two calls are bit-equal;
4. the rule (switch -1) takes the form for the layers it was measured to win on and leaves 48 -> 48 at 2 x 128^3 alone.

The form is forced with brats_conv3d_set_wgrad_noslab(1) and confirmed through brats_conv3d_wgrad_noslab_taken()."""
import contextlib

import pytest
import torch

import _conv_exact_ref as R

pytestmark = pytest.mark.gpu

BF, FH = torch.bfloat16, torch.float16
SENTINEL = -12345.0

CASES = [  # c1, c2, cout, dil, n, size
    (32, 0, 48, 1, 1, (4, 4, 16)),        # one tile, two ci blocks
    (48, 0, 96, 1, 2, (5, 6, 18)),        # ragged in z, y, x; two co blocks
    (16, 16, 48, 1, 2, (8, 8, 16)),       # the source boundary falls on a ci block
    (48, 0, 48, 2, 1, (8, 8, 16)),        # dilation 2, halo wider than a tile
    (48, 0, 48, 2, 2, (5, 6, 18)),        # dilation 2, ragged
    (384, 0, 384, 2, 2, (16, 16, 16)),    # the real layer
]


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@contextlib.contextmanager
def _noslab(mode):
    """All-taps switch on (its default), no-slab switch `mode`."""
    from brats21_amd import _lib
    l = _lib.lib()
    old_a, old_n = l.brats_conv3d_set_wgrad_alltaps(1), l.brats_conv3d_set_wgrad_noslab(mode)
    try:
        yield
    finally:
        l.brats_conv3d_set_wgrad_alltaps(old_a)
        l.brats_conv3d_set_wgrad_noslab(old_n)


def _taken(dtype, dil, n, size, c1, c2, cout):
    from brats21_amd import _lib, ops
    return _lib.lib().brats_conv3d_wgrad_noslab_taken(ops._code(dtype), dil, n, *size, c1, c2, cout)


def _slice_view(t, dtype, pitch, off):
    """CPU channels-last tensor -> a channel slice of a device buffer full of 7s."""
    buf = torch.full(tuple(t.shape[:4]) + (pitch,), 7.0, dtype=dtype, device=_dev())
    buf[..., off:off + t.shape[-1]] = t.to(_dev()).to(dtype)
    return buf[..., off:off + t.shape[-1]]


@pytest.mark.parametrize("c1,c2,cout,dil,n,size", CASES)
@pytest.mark.parametrize("dtype", [BF, FH])
def test_noslab_exact_views_and_out(dtype, c1, c2, cout, dil, n, size):
    from brats21_amd import ops
    x, x2, dy, dw_ref, _ = R.wgrad_case(c1, c2, cout, n, size, dil)
    what = f"noslab {c1}+{c2}->{cout} d{dil} {n}x{size}"
    with _noslab(1):
        assert _taken(dtype, dil, n, size, c1, c2, cout) == 1
        # x, x2 and dy as channel slices of padded buffers
        xd = _slice_view(x, dtype, c1 + 16, 8)
        x2d = _slice_view(x2, dtype, c2 + 8, 0) if x2 is not None else None
        dyd = _slice_view(dy, dtype, cout + 24, 16)
        dw, _ = ops.conv3d_wgrad(xd, dyd, 3, dil, x2=x2d)
        torch.cuda.synchronize()
        R.assert_exact(dw, dw_ref, what=what + " views")
        # out= inside a larger f32 buffer: 16-byte aligned (offset 8 floats) and not (offset 5)
        numel = dw_ref.numel()
        xc, dyc = x.to(_dev()).to(dtype), dy.to(_dev()).to(dtype)
        x2c = x2.to(_dev()).to(dtype) if x2 is not None else None
        for off in (8, 5):
            big = torch.full((numel + 16,), SENTINEL, dtype=torch.float32, device=_dev())
            assert big.data_ptr() % 16 == 0
            got, _ = ops.conv3d_wgrad(xc, dyc, 3, dil, x2=x2c, out=big[off:off + numel])
            torch.cuda.synchronize()
            assert got.data_ptr() == big.data_ptr() + 4 * off
            R.assert_exact(got, dw_ref, what=f"{what} out= at float {off}")
            assert bool((big[:off] == SENTINEL).all()) and bool((big[off + numel:] == SENTINEL).all()), f"{what}: wrote outside dw"


@pytest.mark.parametrize("dil", [1, 2])
def test_noslab_accuracy_against_the_slab_form(dil):
    from brats21_amd import ops
    c, n, size = 384, 2, (16, 16, 16)
    g = torch.Generator().manual_seed(100 + dil)
    x = torch.randn((n, *size, c), generator=g).to(BF)
    dy = torch.randn((n, *size, c), generator=g).to(BF)
    ref = R.wgrad_ref(x.float(), dy.float(), dil)  # float64, from the bf16-rounded operands
    xd, dyd = x.to(_dev()), dy.to(_dev())
    err, got = {}, {}
    for name, mode in (("noslab", 1), ("slab", 0)):
        with _noslab(mode):
            assert _taken(BF, dil, n, size, c, 0, c) == mode
            dw, _ = ops.conv3d_wgrad(xd, dyd, 3, dil)
            torch.cuda.synchronize()
        got[name] = dw.cpu()
        err[name] = float((got[name].double() - ref).abs().max())
    print(f"\n384->384 d={dil} @2x16^3 bf16: max|dW - dW64| no-slab {err['noslab']:.6e}, slab {err['slab']:.6e}, "
          f"max|dW64| {float(ref.abs().max()):.3f}")
    assert err["noslab"] <= 2 * err["slab"], err
    assert torch.equal(got["noslab"], got["slab"]), "the no-slab form must keep the slab form's summation order"


def test_noslab_two_sources_has_the_slab_forms_bits():
    """384 | 384 -> 192 at 2 x 16^3, the third layer the rule takes: bit-equal to its slab form (all-taps <3, 3>)."""
    from brats21_amd import ops
    n, size = 2, (16, 16, 16)
    g = torch.Generator().manual_seed(103)
    x, x2 = (torch.randn((n, *size, 384), generator=g).to(BF).to(_dev()) for _ in range(2))
    dy = torch.randn((n, *size, 192), generator=g).to(BF).to(_dev())
    got = {}
    for mode in (1, 0):
        with _noslab(mode):
            assert _taken(BF, 1, n, size, 384, 384, 192) == mode
            got[mode], _ = ops.conv3d_wgrad(x, dy, 3, 1, x2=x2)
            torch.cuda.synchronize()
    assert torch.equal(got[1], got[0])


@pytest.mark.parametrize("dil", [1, 2])
def test_noslab_is_bitwise_reproducible(dil):
    from brats21_amd import ops
    g = torch.Generator().manual_seed(7)
    x = torch.randn((2, 16, 16, 16, 192), generator=g).to(BF).to(_dev())
    dy = torch.randn((2, 16, 16, 16, 96), generator=g).to(BF).to(_dev())
    with _noslab(1):
        assert _taken(BF, dil, 2, (16, 16, 16), 192, 0, 96) == 1
        a, _ = ops.conv3d_wgrad(x, dy, 3, dil)
        b, _ = ops.conv3d_wgrad(x, dy, 3, dil)
        torch.cuda.synchronize()
    assert torch.equal(a, b)


WINNERS = [  # c1, c2, cout, dil at 2 x 16^3: profiles/wgrad_noslab_layers.txt
    (384, 0, 384, 2), (384, 384, 192, 1), (384, 0, 384, 1),
]
NOT_TAKEN = [  # c1, c2, cout, dil, n, size
    (48, 0, 48, 1, 2, (128, 128, 128)),
    (192, 0, 384, 1, 2, (16, 16, 16)),   # 96 blocks of dW: measured slower than its slab form
    (384, 0, 192, 1, 2, (32, 32, 32)), (192, 0, 192, 1, 2, (32, 32, 32)), (192, 0, 96, 1, 2, (32, 32, 32)), (96, 0, 192, 1, 2, (32, 32, 32)),
]


def test_noslab_rule():
    for dtype in (BF, FH):
        with _noslab(-1):
            for c1, c2, cout, dil in WINNERS:
                assert _taken(dtype, dil, 2, (16, 16, 16), c1, c2, cout) == 1, (c1, c2, cout, dil)
            for c1, c2, cout, dil, n, size in NOT_TAKEN:
                assert _taken(dtype, dil, n, size, c1, c2, cout) == 0, (c1, c2, cout, dil, n, size)
        with _noslab(0):
            for c1, c2, cout, dil in WINNERS:
                assert _taken(dtype, dil, 2, (16, 16, 16), c1, c2, cout) == 0
        with _noslab(1):  # wherever it is built -- and only there
            assert _taken(dtype, 1, 2, (128, 128, 128), 48, 0, 48) == 1
            assert _taken(dtype, 1, 2, (16, 16, 16), 8, 0, 48) == 0 and _taken(dtype, 1, 2, (16, 16, 16), 64, 0, 64) == 0
    from brats21_amd import _lib
    with _noslab(1):
        assert _lib.lib().brats_conv3d_wgrad_noslab_taken(_lib.F32, 1, 2, 16, 16, 16, 384, 0, 384) == 0
        old = _lib.lib().brats_conv3d_set_wgrad_alltaps(0)  # all-taps off: the tap-plane kernel everywhere
        try:
            assert _lib.lib().brats_conv3d_wgrad_noslab_taken(_lib.BF16, 1, 2, 16, 16, 16, 384, 0, 384) == 0
        finally:
            _lib.lib().brats_conv3d_set_wgrad_alltaps(old)
