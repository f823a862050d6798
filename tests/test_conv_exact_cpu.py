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


# ---------------------------------------------------------------------------------------------- first layer: per-tile statistics, walk
def test_tile_statistics_reference_and_what_the_summed_check_cannot_see():
    """tile_stats_ref against a loop over the clipped tiles of a ragged volume; then a correct statistics tensor with two tile rows
    of one sample swapped: the summed comparison (assert_stats_exact) passes it, the per-tile one reports it."""
    x, _, w, bias, y_ref = R.fwd_case(8, 0, 48, 2, (9, 6, 37), real_cin=4)
    ref = R.tile_stats_ref(y_ref)
    tz, ty, tx = 3, 2, 3
    assert ref.shape == (2, tz * ty * tx, 48, 2) and ref.dtype == torch.float64
    for n in range(2):
        for t in range(tz * ty * tx):
            z, y, xx = t // (ty * tx), t // tx % ty, t % tx   # x fastest, then y, then z
            blk = y_ref[n, 4 * z:4 * z + 4, 4 * y:4 * y + 4, 16 * xx:16 * xx + 16].double()
            assert blk.numel() > 0
            assert torch.equal(ref[n, t, :, 0], blk.sum((0, 1, 2))) and torch.equal(ref[n, t, :, 1], (blk * blk).sum((0, 1, 2)))
    assert R.tile_stats_exact_ok(y_ref) and R.stats_exact_ok(y_ref)
    good = ref.float()
    R.assert_stats_exact(good, y_ref, what="summed")
    R.assert_tile_stats_exact(good, y_ref, what="per tile")
    swapped = good.clone()
    swapped[1, 4], swapped[1, 11] = good[1, 11], good[1, 4]
    assert not torch.equal(swapped, good)
    R.assert_stats_exact(swapped, y_ref, what="summed")          # the old check cannot see it
    with pytest.raises(AssertionError, match="per-tile sum of y differs at"):
        R.assert_tile_stats_exact(swapped, y_ref, what="per tile")
    sq = good.clone()
    sq[0, 7, 5, 1] += 1                                            # one sum of squares off by one
    with pytest.raises(AssertionError, match="per-tile sum of y\\^2 differs at 1 of"):
        R.assert_tile_stats_exact(sq, y_ref, what="per tile")
    R.assert_tile_stats_exact(sq, y_ref, squares=False, what="per tile")
    # the preconditions, asserted on the reference alone: one tile of 256 voxels at 2^16 sums to 2^24; at 256, its squares do
    with pytest.raises(AssertionError, match="sum of \\|y\\| = 16777216 >= 2\\^24"):
        R.assert_tile_stats_exact(good, torch.full((1, 4, 4, 16, 2), 2.0 ** 16))
    y256 = torch.full((1, 4, 4, 16, 2), 256.0)
    s256 = R.tile_stats_ref(y256).float()
    with pytest.raises(AssertionError, match="sum of y\\^2 = 16777216 >= 2\\^24"):
        R.assert_tile_stats_exact(s256, y256)
    R.assert_tile_stats_exact(s256, y256, squares=False)
    assert not R.tile_stats_exact_ok(y256) and R.tile_stats_exact_ok(y256, squares=False) and R.tile_stats_exact_ok(y256 / 2)


def test_mirror_of_the_first_layer_walk_and_dispatch():
    """first_walk / first_layer_form: values worked out by hand from csrc/conv_igemm_first.hpp and csrc/conv_bf16_k3_d1.hip for a
    256-CU device, and every property the GPU volumes are listed for."""
    for ntiles, (n, size) in list(R.FIRST_WALKS.items()) + [(2295, R.FIRST_DEFAULT[0])]:
        assert R.ntiles_of(n, size) == ntiles
        for what, holds in R.first_walk_properties(ntiles, n, 256):
            assert holds, (ntiles, what)
    w = R.first_walk(9, 256)
    assert (w.grid, w.per_xcd, w.wg_per_xcd) == (8, 2, 1) and w.slices[4:] == [(8, 9), (10, 9), (12, 9), (14, 9)]
    assert w.tiles == [[0, 1], [2, 3], [4, 5], [6, 7], [8], [], [], []]
    w = R.first_walk(36, 256)
    assert w.slices[3] == (15, 20) and w.slices[7] == (35, 36) and w.tiles[0] == [0, 4] and w.tiles[8] == [1] and w.tiles[31] == []
    w = R.first_walk(525, 256)
    assert (w.grid, w.per_xcd, w.wg_per_xcd) == (512, 66, 64) and w.slices[7] == (462, 525) and w.tiles[0] == [0, 64] and w.tiles[16] == [2]
    assert w.tiles[7 + 8 * 62] == [462 + 62] and w.tiles[7 + 8 * 63] == []
    w = R.first_walk(1170, 256)
    assert (w.per_xcd, w.slices[7][1] - w.slices[7][0]) == (147, 141) and w.trips.count(3) == 7 * 19 + 13
    w = R.first_walk(2295, 256)
    assert (w.per_xcd, w.slices[7][1] - w.slices[7][0]) == (287, 286)
    w = R.first_walk(2048, 256)                                   # the one shape the suite ran before: even in every respect
    assert set(w.trips) == {4} and all(hi - lo == 256 for lo, hi in w.slices)
    assert R.first_walk(12, 2).grid == 8                          # never an empty grid
    # the dispatch: conv_first_ok, then the ck == 8 rule
    assert R.first_layer_form(1, (64, 64, 128)) == "first" and R.first_layer_form(1, (64, 64, 128), dense=False) == "vs8"
    assert R.first_layer_form(1, (64, 64, 128), dense=False, vs8=False) == "tile" and R.first_layer_form(2, (32, 64, 64)) == "tile"
    assert R.first_layer_form(1, (36, 52, 240)) == "tile" and R.first_layer_form(1, (36, 60, 272)) == "first"
    assert R.first_layer_form(1, (28, 4, 16), 8) == "tile" and R.first_layer_form(1, (28, 4, 16), 1) == "vs8"
    assert R.first_layer_form(1, (12, 12, 24), 8) == "vs8" and R.first_layer_form(1, (8, 16, 16), 8, aligned=False) == "vs8"
    assert R.first_layer_form(1, (8, 16, 16), 8, stats=False) == "vs8" and R.first_layer_form(1, (8, 16, 16), 8) == "first"
    for n, size in R.FIRST_RAGGED:
        assert R.first_layer_form(n, size, 8) == "vs8"


@pytest.mark.parametrize("real_cin", [4, 8])
def test_first_layer_cases_meet_the_per_tile_bound_on_dense_operands(real_cin):
    """Every volume of tests/test_first_layer_gpu.py up to 1170 tiles, built here: the dense operand set meets the per-tile bounds
    of assert_tile_stats_exact (sum of |y| and of y^2 below 2^24 per tile and channel), so none of them needs the thinned set --
    although the two largest miss the per-sample bound of the summed check.  (The sum of |y| cannot miss: 1024 voxels x
    (27 taps x 8 channels x 2 x 2 + 2) = 886,784.  The two volumes of the default-threshold test assert the same when they run.)"""
    cases = [(n, size, True) for n, size in list(R.FIRST_WALKS.values()) + R.FIRST_RAGGED + [(1, (28, 4, 16)), (1, (12, 12, 24))]]
    cases.append((*R.FIRST_WALKS[36], False))
    if real_cin == 4:   # (half the terms per output: the two large volumes are built once, with all 8 channels)
        cases = [c for c in cases if R.ntiles_of(c[0], c[1]) < 500]
    per_sample = {}
    for n, size, with_bias in cases:
        y_ref = R.fwd_case(8, 0, 48, n, size, with_bias=with_bias, real_cin=real_cin)[4]
        assert R.tile_stats_exact_ok(y_ref), (n, size, with_bias)
        assert float(R.tile_stats_ref(y_ref)[..., 1].max()) < R.EXACT / 4, (n, size)   # not by a hair either
        per_sample[(n, size)] = R.stats_exact_ok(y_ref)
    assert per_sample[(2, (8, 12, 48))]
    assert real_cin == 4 or (not per_sample[(1, (36, 52, 160))] and not per_sample[(1, (20, 28, 240))])


def _emulated_first_kernel(y_ref, n, ncu, rig=None):
    """What conv_first_kernel leaves behind in an output full of 7s and a statistics buffer full of NaN if its walk is the mirrored
    one and every visited tile gets the reference's values -- or, rigged, with one of three faults put into conv_launch_first's kernel:
    "skip_last": the last tile of every XCD slice is not done; "slot_t": a tile's statistics go to slot t instead of t % tps (a
    slot beyond the buffer is dropped here; on the device it would be a write out of bounds); "no_flip": cur ^= 1 is dropped,
    so from its second tile on a workgroup computes on the halo buffer of its first."""
    _, d, h, w, c = y_ref.shape
    tz, ty, tx = d // 4, h // 4, w // 16
    tps = tz * ty * tx
    walk = R.first_walk(n * tps, ncu)
    ref = R.tile_stats_ref(y_ref)
    y = torch.full(y_ref.shape, 7.0, dtype=torch.float64)
    stats = torch.full((n * tps, c, 2), float("nan"), dtype=torch.float64)

    def block(t):
        s, r = t // tps, t % tps
        z, yy, x = r // (ty * tx), r // tx % ty, r % tx
        return (s, slice(4 * z, 4 * z + 4), slice(4 * yy, 4 * yy + 4), slice(16 * x, 16 * x + 16))
    for b, tiles in enumerate(walk.tiles):
        for k, t in enumerate(tiles):
            if rig == "skip_last" and t == walk.slices[b & 7][1] - 1:
                continue
            src = tiles[0] if rig == "no_flip" and k else t
            y[block(t)] = y_ref[block(src)].double()
            slot = (t // tps) * tps + (t if rig == "slot_t" else t % tps)
            if slot < n * tps:
                stats[slot] = ref[src // tps, src % tps]
    return y, stats.reshape(n, tps, c, 2)


@pytest.mark.parametrize("ntiles", [8, 9, 36])
def test_the_first_layer_checks_see_a_rigged_walk(ntiles):
    """The evidence that the GPU cases would fail on a subtly wrong persistent kernel, from the walk mirror and the reference (no
    rigged kernel is run on a device: the second fault writes out of bounds there).  Unrigged, the emulation passes the two
    assertions the GPU tests make; a skipped last tile of a slice fails both on every volume; statistics in slot t fail on the
    two-sample volume (36 tiles), the only way to tell t from t % tps; a dropped buffer flip fails wherever a workgroup has a
    second tile (9 and 36 tiles; not 8: no workgroup prefetches there)."""
    n, size = R.FIRST_WALKS[ntiles]
    y_ref = R.fwd_case(8, 0, 48, n, size, real_cin=4)[4]

    def check(rig):
        y, stats = _emulated_first_kernel(y_ref, n, 256, rig)
        R.assert_exact(y.float().to(torch.bfloat16), y_ref, torch.bfloat16, what="y")
        R.assert_tile_stats_exact(stats.float(), y_ref, what="stats")
    check(None)
    with pytest.raises(AssertionError, match="y: .* entries differ"):
        check("skip_last")
    y, stats = _emulated_first_kernel(y_ref, n, 256, "skip_last")
    with pytest.raises(AssertionError, match="per-tile sum of y differs"):
        R.assert_tile_stats_exact(stats.float(), y_ref, what="stats")
    if n > 1:
        with pytest.raises(AssertionError, match="per-tile sum of y differs"):
            check("slot_t")
    else:
        check("slot_t")     # one sample: t == t % tps, nothing to see
    if ntiles > 8:
        with pytest.raises(AssertionError, match="y: .* entries differ"):
            check("no_flip")
    else:
        check("no_flip")


# ---------------------------------------------------------------------------------------------- direct (gather) convolution
def _torch_term(x, w, dy, k, dil):
    """F.conv3d (padding = dilation for k = 3) and its autograd input gradient, channels-last f32."""
    xr = _nc(x).requires_grad_(True)
    y = F.conv3d(xr, w, None, 1, dil if k == 3 else 0, dil)
    y.backward(_nc(dy))
    return y.detach().permute(0, 2, 3, 4, 1), xr.grad.permute(0, 2, 3, 4, 1)


@pytest.mark.parametrize("k,dil,n,size", [(3, 3, 2, (5, 6, 7)), (3, 4, 1, (8, 8, 8)), (3, 6, 2, (5, 6, 7)), (3, 6, 1, (7, 13, 14)),
                                          (1, 1, 2, (5, 6, 7)), (1, 1, 1, (1, 1, 33))])
def test_wide_dilation_and_pointwise_references_equal_torch(k, dil, n, size):
    """fwd_ref and dgrad_ref at the dilations of the ASPP branches (3, 4, 6; on 5x6x7 every extent is thinner than dilation 6)
    and at k = 1, against torch's f32 CPU convolution and autograd, bit for bit."""
    cin, cout = 24, 16
    x, _, w, bias, y_ref = R.fwd_case(cin, 0, cout, n, size, dil, k, seed=3)
    dy = R.int_tensor((n, *size, cout), 13)
    R.require_fwd_exact(dy, w.transpose(0, 1))
    y, dx = _torch_term(x, w, dy, k, dil)
    R.assert_exact(y + bias, y_ref, what=f"forward k {k} dilation {dil}")
    R.assert_exact(dx, R.dgrad_ref(dy, w, dil), what=f"input gradient k {k} dilation {dil}")


def test_dilation_wider_than_the_volume_leaves_the_centre_tap():
    """2 x (5, 6, 7) at dilation 6: every tap that moves in z (extent 5) or y (extent 6) leaves the volume, and an x tap stays
    inside only between the columns x = 0 and x = 6 (extent 7).  So the branch equals a 1x1x1 convolution with the centre
    weights at x = 1..5, and the three (centre, centre, *) taps everywhere -- what the direct kernel's tap masks must reproduce.
    On 2 x (5, 6, 6) the centre tap is all that is left."""
    x, _, w, bias, y_ref = R.fwd_case(16, 0, 32, 2, (5, 6, 7), 6, 3, seed=4)
    centre = w[:, :, 1:2, 1:2, 1:2].contiguous()
    assert torch.equal(y_ref[:, :, :, 1:6], R.fwd_ref(x, centre, bias, 1)[:, :, :, 1:6])
    assert not torch.equal(y_ref[:, :, :, 0], R.fwd_ref(x, centre, bias, 1)[:, :, :, 0])
    wx = torch.zeros_like(w)
    wx[:, :, 1, 1, :] = w[:, :, 1, 1, :]
    assert torch.equal(y_ref, R.fwd_ref(x, wx, bias, 6))
    dy = R.int_tensor((2, 5, 6, 7, 32), 14)
    assert torch.equal(R.dgrad_ref(dy, w, 6), R.dgrad_ref(dy, wx, 6))
    assert torch.equal(R.dgrad_ref(dy, w, 6)[:, :, :, 1:6], R.dgrad_ref(dy, centre, 1)[:, :, :, 1:6])
    x6, _, w6, b6, y6 = R.fwd_case(16, 0, 32, 2, (5, 6, 6), 6, 3, seed=4)
    assert torch.equal(y6, R.fwd_ref(x6, w6[:, :, 1:2, 1:2, 1:2].contiguous(), b6, 1))


def test_four_term_sum_equals_the_sum_of_four_torch_input_gradients():
    """The reference of a four-term PACK_DGRAD job (dconv_case, mode "dgrad") = the sum of four F.conv3d autograd input gradients
    (summed in float64: every one of them is an exact integer), and that of a forward job = the sum of four F.conv3d outputs."""
    n, size = R.VOL_RAGGED
    terms = ((16, 1, 1), (48, 3, 3), (32, 3, 6), (8, 3, 2))
    case = R.dconv_case(n, size, ((36, terms, False),), "dgrad")
    job = case.jobs[0]
    tot = torch.zeros((n, *size, 36), dtype=torch.float64)
    for t in job.terms:
        xr = torch.zeros((n, 36, *size), requires_grad=True)
        F.conv3d(xr, t.w, None, 1, t.dil if t.k == 3 else 0, t.dil).backward(_nc(t.x))
        tot += xr.grad.permute(0, 2, 3, 4, 1).double()
    R.assert_exact(tot.float(), job.ref, what="four-term input gradient")
    fwd = R.dconv_case(n, size, ((36, terms, True),), "fwd").jobs[0]
    tot = sum(F.conv3d(_nc(t.x), t.w, None, 1, t.dil if t.k == 3 else 0, t.dil).permute(0, 2, 3, 4, 1).double() for t in fwd.terms)
    R.assert_exact((tot + fwd.bias.double()).float(), fwd.ref, what="four-term forward")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "f32"])
def test_every_dconv_case_meets_its_preconditions(dtype):
    """Every launch of tests/test_dconv_exact_gpu.py, built on the CPU: the builders assert the 2^24 bound on the operands and, for
    the 16-bit types, max|reference| <= 256 (bf16) / 2048 (fp16) -- the store then rounds nothing and a change of 1 in any output
    is visible.  Checked again here from outside the builders, with the operands' exactness in the storage type."""
    bound = R.OUT_BOUND[dtype]
    cases = R.dconv_cases(dtype)
    assert len(cases) == len(R.dconv_cases(torch.float32))
    for name, args in cases.items():
        case = R.dconv_case(*args)
        for job in case.jobs:
            assert job.ref.shape == (case.n, *case.size, job.rows) and float(job.ref.abs().max()) > 0, name
            assert torch.equal(job.ref, job.ref.round()), name
            if bound is not None:
                assert float(job.ref.abs().max()) <= bound, name
                assert torch.equal(job.ref.float().to(dtype).double(), job.ref), name  # the final rounding is the identity
            for t in job.terms:
                assert torch.equal(t.x.to(dtype).float(), t.x) and torch.equal(t.w.to(dtype).float(), t.w), name
    for c1, c2, cout, (n, size), k, dil in R.DCONV_SPLIT_CASES:
        y = R.dconv_split_case(c1, c2, cout, n, size, k, dil, bound)[-1]
        assert bound is None or torch.equal(y.float().to(dtype).double(), y)
    for nb, cin, q, n, size in R.ASPP_CASES:
        a = R.aspp_case(nb, cin, q, n, size, bound)
        assert len(a.dx_parts) == (nb + 3) // 4 and torch.equal(sum(a.dx_parts), a.dx)
        if bound is not None:
            # each launch's partial is stored unrounded, so torch's 16-bit adds of the parts are exact too
            run = torch.zeros_like(a.dx)
            for p in a.dx_parts:
                run = run + p
                assert float(p.abs().max()) <= bound and float(run.abs().max()) <= bound
            for t in (a.acat, a.dx):
                assert torch.equal(t.float().to(dtype).double(), t)


def test_dconv_case_list_reaches_the_kernel_geometry():
    """The properties of the case list that the kernel's branches need (NF = 3 row fragments of 32 per workgroup, 256 voxels per
    workgroup, a pipeline three steps deep), asserted on the list itself."""
    for dtype in (torch.bfloat16, torch.float32):
        kch, cases = R.DCONV_KCH[dtype], R.dconv_cases(dtype)
        steps = {sum(R._taps_of(k) * cin // kch for cin, k, _ in jobs[0][1]) for name, (_, _, jobs, _, _) in cases.items() if name.startswith("k1-")}
        assert steps == {1, 2, 3, 4, 7}   # below, at and above the pipeline depth, and no multiple of it
        rows = sorted({jobs[0][0] for name, (_, _, jobs, _, _) in cases.items() if name.startswith("rows")})
        assert rows == [4, 16, 36, 96, 100, 132]
        frags = [(r + 31) // 32 for r in rows]
        assert [(f + R.DCONV_NF - 1) // R.DCONV_NF for f in frags] == [1, 1, 1, 1, 2, 2]     # 100, 132: a second blockIdx.y ...
        assert [f - R.DCONV_NF for f in frags[4:]] == [1, 2]                                  # ... with one and with two live fragments
        assert [r % 32 for r in rows] == [4, 16, 4, 0, 4, 4]                                  # tails inside a fragment at a granule of 4
        net = cases["net-rows-2x5x6x7"][2]
        assert [j[0] for j in net] == [100, 16, 36, 4] and [j[1][0][1:] for j in net] == [(1, 1), (3, 2), (3, 4), (3, 6)]
    vox = [n * s[0] * s[1] * s[2] for n, s in R.DCONV_VOLUMES]
    assert vox == [420, 90, 33, 1024]
    assert vox[0] % R.DCONV_WG_VOX and vox[0] % 32 and (vox[0] // 2) % 32     # partial workgroup and fragment, a fragment across samples
    assert vox[1] < R.DCONV_WG_VOX - 64 and vox[3] % R.DCONV_WG_VOX == 0      # a whole wave idle / whole workgroups only


def test_dconv_preconditions_reject_violations():
    x, w = R.int_tensor((1, 2, 2, 4, 16), 1), R.int_tensor((8, 16, 3, 3, 3), 2)
    R.require_terms_exact([(x, w), (x, w)], R.int_tensor((8,), 3))
    with pytest.raises(AssertionError, match="2\\^24"):
        R.require_terms_exact([(x * 2 ** 7, w * 2 ** 5)] * 4)      # 4 * 27 * 16 * 256 * 64 > 2^24 though one term alone is below
    R.require_terms_exact([(x * 2 ** 7, w * 2 ** 5)])
    with pytest.raises(AssertionError, match="integers"):
        R.require_terms_exact([(x, w + 0.5)])
    R.require_within(torch.tensor([256.0, -3.0]), 256.0)
    with pytest.raises(AssertionError, match="exceeds 256"):
        R.require_within(torch.tensor([257.0]), 256.0)
    with pytest.raises(AssertionError, match="exceeds 256"):      # dense operands at cin = 96 do not fit bf16 (the builder thins them)
        R.require_within(R.fwd_case(96, 0, 32, 2, (8, 8, 8), 1)[-1], 256.0)
    assert R.thin_density(16, 256.0) == 1.0 and R.thin_density(27 * 96, 256.0) < 0.5 and R.thin_density(27 * 96, None) == 1.0
