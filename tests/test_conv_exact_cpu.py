"""The exact integer-operand references of tests/_conv_exact_ref.py against torch's f32 CPU convolution and autograd: on
integer operands under the stated bounds both are exact, so they agree bit for bit; one voxel changed by 1 makes the
comparison the GPU tests use (assert_exact) report a mismatch; the preconditions reject operands that violate them; the
mirror of the weight-gradient host rules gives the values worked out by hand from csrc/conv_wgrad.hip."""
import pytest
import torch
import torch.nn.functional as F

import _conv_exact_ref as R

SHAPES = [  # c1, c2, cout, n, size, dil
    (16, 0, 32, 2, (5, 6, 18), 1),     # ragged on every axis
    (8, 0, 48, 1, (8, 8, 16), 2),      # dilation 2
    (16, 48, 32, 2, (4, 6, 7), 1),     # two sources of different widths
    (48, 48, 24, 1, (6, 5, 9), 2),     # two sources at dilation 2
]


def _nc(t):
    return t.permute(0, 4, 1, 2, 3).contiguous()


def _torch_f32(x, x2, w, bias, dy, dil):
    xr = _nc(R._cat(x, x2)).requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    br = bias.clone().requires_grad_(True)
    y = F.conv3d(xr, wr, br, 1, dil, dil)
    y.backward(_nc(dy))
    return y.detach().permute(0, 2, 3, 4, 1), xr.grad.permute(0, 2, 3, 4, 1), wr.grad, br.grad


@pytest.mark.parametrize("c1,c2,cout,n,size,dil", SHAPES)
def test_references_equal_torch_f32_exactly(c1, c2, cout, n, size, dil):
    x, x2, w, bias, y_ref = R.fwd_case(c1, c2, cout, n, size, dil)
    dy = R.int_tensor((n, *size, cout), 11)
    R.require_wgrad_exact(x, dy, x2)
    R.require_fwd_exact(dy, w.transpose(0, 1))
    y, dx, dw, db = _torch_f32(x, x2, w, bias, dy, dil)
    R.assert_exact(y, y_ref, what="forward")
    R.assert_exact(dx, R.dgrad_ref(dy, w, dil), what="input gradient")
    R.assert_exact(dw, R.wgrad_ref(x, dy, dil, 3, x2), what="weight gradient")
    R.assert_exact(db, R.dbias_ref(dy), what="bias gradient")
    for dt in (torch.bfloat16, torch.float16):  # the 16-bit statement: RNE of the exact integer
        R.assert_exact(y.to(dt), y_ref, dt, what="forward, 16-bit")


def test_one_by_one_references_equal_torch():
    x, _, w, bias, y_ref = R.fwd_case(24, 0, 48, 2, (5, 6, 7), 1, 1)
    dy = R.int_tensor((2, 5, 6, 7, 48), 12)
    xr, wr = _nc(x).requires_grad_(True), w.clone().requires_grad_(True)
    y = F.conv3d(xr, wr, bias)
    y.backward(_nc(dy))
    R.assert_exact(y.detach().permute(0, 2, 3, 4, 1), y_ref, what="1x1x1 forward")
    R.assert_exact(wr.grad, R.wgrad_ref(x, dy, 1, 1), what="1x1x1 weight gradient")
    R.assert_exact(xr.grad.permute(0, 2, 3, 4, 1), R.dgrad_ref(dy, w, 1), what="1x1x1 input gradient")


@pytest.mark.parametrize("dil", [4, 6])
def test_wide_dilation_weight_gradient_reference_equals_torch(dil):
    x, _, dy, dw_ref, _ = R.wgrad_case(16, 0, 24, 1, (10, 12, 20), dil)
    wr = torch.zeros(24, 16, 3, 3, 3, requires_grad=True)
    F.conv3d(_nc(x), wr, None, 1, dil, dil).backward(_nc(dy))
    R.assert_exact(wr.grad, dw_ref, what=f"dilation {dil}")


def test_one_voxel_changes_the_comparison():
    """One element of x off by 1 (what a dropped, doubled or misplaced voxel does to a sum) fails assert_exact for the weight
    gradient and for the forward output, f32 and 16-bit."""
    c1, c2, cout, n, size, dil = SHAPES[0]
    x, x2, w, bias, y_ref = R.fwd_case(c1, c2, cout, n, size, dil)
    dy = R.int_tensor((n, *size, cout), 11)
    dw_ref = R.wgrad_ref(x, dy, dil)
    xb = x.clone()
    xb[1, 4, 5, 17, 3] += 1  # the last voxel: a corner of the volume
    assert int((dy[1, 3:, 4:, 16:] != 0).sum()) > 0
    with pytest.raises(AssertionError, match="entries differ"):
        R.assert_exact(R.wgrad_ref(xb, dy, dil).float(), dw_ref, what="dW")
    yb = R.fwd_ref(xb, w, bias, dil)
    with pytest.raises(AssertionError, match="entries differ"):
        R.assert_exact(yb.float(), y_ref, what="y")
    with pytest.raises(AssertionError, match="entries differ"):
        R.assert_exact(yb.float().to(torch.bfloat16), y_ref, torch.bfloat16, what="y bf16")
    st = torch.stack([yb.sum((1, 2, 3)), (yb * yb).sum((1, 2, 3))], -1).float()[:, None]  # one "tile" per sample
    with pytest.raises(AssertionError, match="differs"):
        R.assert_stats_exact(st, y_ref, what="stats")
    good = torch.stack(R.tile_sums_ref(y_ref), -1).float()[:, None]
    R.assert_stats_exact(good, y_ref, squares=R.stats_exact_ok(y_ref), what="stats")


def test_preconditions_reject_violations():
    x = R.int_tensor((1, 4, 4, 16, 8), 1)
    dy = R.int_tensor((1, 4, 4, 16, 8), 2)
    R.require_wgrad_exact(x, dy)
    with pytest.raises(AssertionError, match="2\\^24"):
        R.require_wgrad_exact(x * 2 ** 9, dy * 2 ** 6)           # 256 * 1024 * 128 = 2^25
    with pytest.raises(AssertionError, match="integers"):
        R.require_wgrad_exact(x + 0.5, dy)
    # K alone: 2 x 128 x 128 x 128 voxels of [-2, 2] operands is exactly the bound (K = 4,194,304)
    big = torch.zeros((2, 128, 128, 128, 1))
    big[0, 0, 0, 0, 0] = 2
    with pytest.raises(AssertionError, match="2\\^24"):
        R.require_wgrad_exact(big, big)
    w = R.int_tensor((8, 8, 3, 3, 3), 3)
    R.require_fwd_exact(x, w, R.int_tensor((8,), 4))
    with pytest.raises(AssertionError, match="2\\^24"):
        R.require_fwd_exact(x * 2 ** 10, w * 2 ** 6)             # 27 * 8 * 2048 * 128 > 2^24
    y = torch.full((1, 16, 16, 16, 2), 64.0)                      # 4096 voxels * 64^2 = 2^24
    assert not R.stats_exact_ok(y)
    with pytest.raises(AssertionError, match="y\\^2"):
        R.require_stats_exact(y)
    R.require_stats_exact(y / 2)
    # thinning brings a deep layer's sum of y^2 under its bound
    _, _, _, _, y_thin = R.fwd_case(192, 0, 16, 1, (8, 8, 16), 1, thin=True)
    R.require_stats_exact(y_thin)


def test_generators_are_seeded_integer_and_thin():
    a, b = R.int_tensor((4, 1000), 5), R.int_tensor((4, 1000), 5)
    assert torch.equal(a, b) and not torch.equal(a, R.int_tensor((4, 1000), 6))
    assert set(a.unique().tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    t = R.int_tensor((100000,), 7, 0.25)
    assert 0.24 < float((t != 0).float().mean()) < 0.26 and float(t.abs().max()) == 2.0
    for dt in (torch.bfloat16, torch.float16, torch.float8_e4m3fn):
        assert torch.equal(a.to(dt).float(), a)


def test_mirror_of_the_weight_gradient_host_rules():
    """Values worked out by hand from csrc/conv_wgrad.hip for a 256-CU device."""
    assert [R.wgrad_nlane(t) for t in (4, 16, 31, 32, 63, 64, 127, 128, 1024)] == [1, 1, 1, 2, 2, 4, 4, 8, 8]
    assert R.wgrad_tiles(False, 48, 0, 48) == (3, 3) and R.wgrad_tiles(False, 16, 48, 32) == (2, 1)
    assert R.wgrad_tiles(False, 32, 32, 64) == (2, 2) and R.wgrad_tiles(True, 48, 0, 40) == (3, 1)
    assert R.wgrad_tiles(False, 8, 0, 8) == (1, 1) and R.wgrad_tiles(False, 24, 0, 40) == (3, 2)
    # 384 -> 384 at 16^3, one sample: 16 tiles, one lane; tap-plane: ceil(512 / (3 * 64)) = 3 slabs; all-taps: 64 blocks,
    # g8 = 4, and 16 tiles is exactly the threshold 4 * 1 * 4
    p0 = R.wgrad_plan(True, 1, 384, 0, 384, 1, 16, 16, 16, 0, 256)
    assert (p0["ntiles"], p0["nlane"], p0["nsplit"], p0["cof"], p0["cif"], p0["reduce"]) == (16, 1, 3, 3, 3, "reduce_taps")
    p1 = R.wgrad_plan(True, 1, 384, 0, 384, 1, 16, 16, 16, 1, 256)
    assert (p1["kernel"], p1["nsplit"]) == ("alltaps2<3, 3>", 4)
    assert R.wgrad_plan(True, 2, 384, 0, 384, 1, 16, 16, 16, 1, 256)["kernel"] == "tapplane<16, 2, 3, 3>"
    assert R.wgrad_alltaps_ok(1, True, 1, 384, 0, 384, 15, 256) is None
    # 48 -> 48: one block, 8 lanes x 32: 1024 tiles = 2 x 32 x 64 x 64
    assert R.wgrad_alltaps_ok(1, True, 1, 48, 0, 48, 1023, 256) is None
    assert R.wgrad_alltaps_ok(1, True, 1, 48, 0, 48, 1024, 256) == (32, "alltaps2<3, 3>")
    assert R.smallest_alltaps_volume(48, 0, 48, 256) == (2, (32, 64, 64))
    assert R.wgrad_alltaps_ok(1, True, 1, 8, 0, 64, 1024, 256)[1] == "alltaps_kernel<1, 4>"
    assert R.wgrad_alltaps_ok(1, True, 1, 32, 32, 128, 1024, 256)[1] == "alltaps2<4, 2>"
    assert R.wgrad_alltaps_ok(1, True, 1, 16, 0, 48, 1024, 256)[1] == "alltaps2<3, 1>"
    assert R.wgrad_alltaps_ok(1, False, 1, 48, 0, 48, 1024, 256) is None
    # the reduction: the all-taps-per-block form from 32768 (co, ci) pairs on
    assert R.wgrad_reduce_kind(192, 192, 27) == "reduce_taps" and R.wgrad_reduce_kind(128, 248, 27) == "reduce"
    assert R.wgrad_reduce_kind(384, 96, 1) == "reduce"
    # n = 2, (16, 16, 64) at 48 -> 48: 128 tiles, 8 lanes, g8 = min(ceil(512 / 24), 16) = 16: 128 slabs
    p = R.wgrad_plan(True, 1, 48, 0, 48, 2, 16, 16, 64, 0, 256)
    assert (p["ntiles"], p["nlane"], p["nsplit"], p["reduce"], p["memset"]) == (128, 8, 128, "reduce", False)
    assert R.wgrad_plan(True, 1, 24, 0, 40, 2, 5, 6, 18, 0, 256)["memset"]
    s = R.wgrad_shift_plan(True, 1, 384, 96, 1, 8, 8, 16)
    assert (s["ntiles"], s["nlane"], s["cof"], s["cif"], s["nsplit"]) == (4, 1, 3, 3, 4)
