"""-m gpu: every convolution kernel form on small INTEGER operands against the float64 shifted-GEMM references of
tests/_conv_exact_ref.py, bit for bit (torch.equal; no tolerance anywhere in this file).

x, dy, w and the bias are integers in [-2, 2]: exact in bf16, fp16, f32, e4m3 and in the hi half of a split-precision pair
(the lo halves are zero).  Under the preconditions asserted by the reference module every partial sum of every summation
order is an exact f32 integer, so a weight gradient must equal the reference in all bits whatever the split-K schedule, the
slab order, the reduction kernel or the MFMA shape, and a 16-bit output is the round-to-nearest-even of an exact integer.  A
single missing, doubled or misplaced voxel, tap or channel changes an integer (tests/test_conv_exact_cpu.py shows the
comparison used here failing on one voxel off by one).

Which kernel and which reduction a weight-gradient case takes is stated by the Python mirror of the host rules
(_conv_exact_ref.wgrad_plan) and tied to the library by the workspace size: brats_conv3d_wgrad_ws_bytes returns
nsplit * 27 * cout * cin * 4 of the form the current switch selects, so a changed rule fails the test.
Channel-slice inputs are views of wider buffers filled with the integer 7: a leak changes an integer."""
import contextlib

import pytest
import torch

import _conv_exact_ref as R

pytestmark = pytest.mark.gpu

BF, FH, F32 = torch.bfloat16, torch.float16, torch.float32
SMALL, MID = (5, 6, 18), (16, 16, 64)   # n = 2: 16 tiles, ragged on every axis (nlane 1) / 128 tiles (nlane 8)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _dv(t, dtype, pitch=None, off=0):
    """CPU channels-last integer tensor -> device tensor of `dtype`, optionally as a channel slice of a buffer full of 7s."""
    if t is None:
        return None
    d = t.to(_dev()).to(dtype)
    assert torch.equal(d.float().cpu(), t)  # the operands really are exact in the storage type
    if pitch is None:
        return d.contiguous()
    buf = torch.full(tuple(t.shape[:4]) + (pitch,), 7.0, dtype=dtype, device=_dev())
    buf[..., off:off + t.shape[-1]] = d
    return buf[..., off:off + t.shape[-1]]


@contextlib.contextmanager
def _alltaps(mode):
    from brats21_amd import _lib
    old = _lib.lib().brats_conv3d_set_wgrad_alltaps(mode)
    try:
        yield
    finally:
        _lib.lib().brats_conv3d_set_wgrad_alltaps(old)


def _wgrad(case, dtype, dil, mode, views=False, want_dbias=False):
    """Run brats_conv3d_wgrad on a _conv_exact_ref.wgrad_case under all-taps switch `mode`; assert the mirrored workspace size
    and the exact result.  -> the mirrored plan."""
    from brats21_amd import _lib, ops
    x, x2, dy, dw_ref, db_ref = case
    n, d, h, w, c1 = x.shape
    c2, cout = (x2.shape[-1] if x2 is not None else 0), dy.shape[-1]
    plan = R.wgrad_plan(dtype != F32, dil, c1, c2, cout, n, d, h, w, mode, _ncu())
    xd = _dv(x, dtype, c1 + 16 if views else None, 8)
    x2d = _dv(x2, dtype, c2 + 8 if views else None, 0)
    dyd = _dv(dy, dtype, cout + 24 if views else None, 16)
    with _alltaps(mode):
        ws = _lib.lib().brats_conv3d_wgrad_ws_bytes(ops._code(dtype), 3, n, d, h, w, c1, c2, cout)
        assert ws == plan["ws_bytes"], (ws, plan)
        dw, db = ops.conv3d_wgrad(xd, dyd, 3, dil, want_dbias=want_dbias, x2=x2d)
        torch.cuda.synchronize()
    R.assert_exact(dw, dw_ref, what=f"dW {plan['kernel']} nsplit {plan['nsplit']} {plan['reduce']}")
    if want_dbias:
        R.assert_exact(db, db_ref, what="dbias")
    return plan


# ---------------------------------------------------------------------------------------------- 1. tap-plane, every instantiation
COF = {48: 3, 32: 2, 16: 1, 8: 1, 40: 3}
CIF = {48: 3, 32: 2, 16: 1, 8: 1, 24: 2}
_FULL = [(ci, co) for co in (48, 32, 16) for ci in (48, 32, 16)]
_PADDED = [(8, 48), (24, 48), (48, 8), (48, 40), (24, 40), (8, 8)]   # partial ci_lim / co_lim lanes: the slab is cleared first


@pytest.mark.parametrize("size", [SMALL, MID])
@pytest.mark.parametrize("dil", [1, 2])
@pytest.mark.parametrize("cin,cout", _FULL + _PADDED)
@pytest.mark.parametrize("dtype", [BF, FH])
def test_tapplane_wgrad_every_16bit_instantiation(dtype, cin, cout, dil, size):
    """conv_wgrad_kernel<T, DIL, COF, CIF> for every (COF, CIF) of wgrad_dispatch at dilation 1 and 2, the all-taps switch off.
    MID at 48 -> 48 is 128 slabs through the 8-in-flight loop of wgrad_reduce_kernel."""
    plan = _wgrad(R.wgrad_case(cin, 0, cout, 2, size, dil), dtype, dil, 0)
    assert plan["kernel"] == f"tapplane<16, {dil}, {COF[cout]}, {CIF[cin]}>"
    assert (plan["cof"], plan["cif"], plan["nlane"]) == (COF[cout], CIF[cin], 1 if size == SMALL else 8)
    assert plan["ntiles"] == (16 if size == SMALL else 128) and plan["reduce"] == "reduce"
    assert plan["memset"] == ((cin, cout) in _PADDED)
    if size == MID and (cin, cout) == (48, 48):
        assert plan["nsplit"] == 128


@pytest.mark.parametrize("size", [SMALL, MID])
@pytest.mark.parametrize("dil", [1, 2])
@pytest.mark.parametrize("cin,cout", [(16, 48), (16, 32), (16, 16), (8, 48), (24, 40), (48, 8)])
def test_tapplane_wgrad_f32_instantiations(cin, cout, dil, size):
    """The exact-f32 MFMA instantiations <float, DIL, COF, 1> (CIF is always 1), padded lanes included."""
    plan = _wgrad(R.wgrad_case(cin, 0, cout, 2, size, dil), F32, dil, 0)
    assert (plan["cof"], plan["cif"], plan["nlane"]) == (COF[cout], 1, 1 if size == SMALL else 8)
    assert plan["kernel"] == f"tapplane<f32, {dil}, {COF[cout]}, 1>"


# ---------------------------------------------------------------------------------------------- 2. two sources and views
@pytest.mark.parametrize("views", [False, True])
@pytest.mark.parametrize("c1,c2,cout,cif", [(48, 48, 48, 3), (32, 32, 64, 2), (16, 48, 32, 1)])
@pytest.mark.parametrize("dtype", [BF, FH, F32])
def test_tapplane_wgrad_two_sources_views_and_dbias(dtype, c1, c2, cout, cif, views):
    """[x | x2] inputs (the ci tile must not straddle the boundary: 16 | 48 falls to CIF 1), x, x2 and dy as channel slices of
    buffers full of 7s, the bias gradient out of the same call."""
    for size, dil in ((SMALL, 1), (SMALL, 2), (MID, 1)):
        plan = _wgrad(R.wgrad_case(c1, c2, cout, 2, size, dil), dtype, dil, 0, views=views, want_dbias=True)
        assert plan["cif"] == (1 if dtype == F32 else cif) and plan["kernel"].startswith("tapplane")


@pytest.mark.parametrize("c1,c2,cout,name", [(48, 48, 48, "alltaps2<3, 3>"), (32, 32, 64, "alltaps2<4, 2>")])
@pytest.mark.parametrize("dtype", [BF, FH])
def test_alltaps_wgrad_two_sources_views_and_dbias(dtype, c1, c2, cout, name):
    """The same two-source layers at the smallest volume at which the all-taps form is taken, switch on and off, channel-slice
    views, with the bias gradient."""
    n, size = R.smallest_alltaps_volume(c1, c2, cout, _ncu())
    case = R.wgrad_case(c1, c2, cout, n, size, 1)
    assert _wgrad(case, dtype, 1, 1, views=True, want_dbias=True)["kernel"] == name
    assert _wgrad(case, dtype, 1, 0, views=True, want_dbias=True)["kernel"].startswith("tapplane")


# ---------------------------------------------------------------------------------------------- 3. deep-level shapes
DEEP_LAYERS = [(384, 0, 384, 1), (384, 0, 384, 2), (384, 384, 192, 1), (192, 0, 192, 1)]
DEEP_VOLUMES = [(1, (16, 16, 16)), (2, (16, 16, 16)), (1, (8, 8, 16))]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n,size", DEEP_VOLUMES)
@pytest.mark.parametrize("c1,c2,cout,dil", DEEP_LAYERS)
@pytest.mark.parametrize("dtype", [BF, FH])
def test_deep_level_wgrad(dtype, c1, c2, cout, dil, n, size, mode):
    """The networks' 192 / 384-channel layers at 16^3 and 8^3: wgrad_nlane 1 or 2, the <16, DIL, 3, 3> tap-plane instantiations
    or alltaps2<3, 3>, and wgrad_reduce_taps_kernel (cout * cin >= 32768) with few slabs."""
    plan = _wgrad(R.wgrad_case(c1, c2, cout, n, size, dil), dtype, dil, mode)
    assert plan["reduce"] == "reduce_taps" and (plan["cof"], plan["cif"]) == (3, 3)
    assert plan["nlane"] == (2 if n == 2 else 1)
    if mode == 0 or dil == 2:
        assert plan["kernel"] == f"tapplane<16, {dil}, 3, 3>"
    assert plan["kernel"] in (f"tapplane<16, {dil}, 3, 3>", "alltaps2<3, 3>")


def test_deep_level_list_reaches_the_required_branches():
    """On the device at hand the list above includes: all-taps taken with ntiles == 4 * nlane * g8 exactly; a
    wgrad_reduce_taps_kernel run with fewer than 8 slabs; one with a slab count that is no multiple of 8; dilation 2 on the
    tap-plane form; both kernels."""
    ncu = _ncu()
    plans = [(R.wgrad_plan(True, dil, c1, c2, cout, n, *size, mode, ncu), dil)
             for c1, c2, cout, dil in DEEP_LAYERS for n, size in DEEP_VOLUMES for mode in (0, 1)]
    at = [p for p, _ in plans if p["kernel"].startswith("alltaps")]
    assert any(p["ntiles"] == 4 * p["nsplit"] for p in at), [(p["ntiles"], p["nsplit"]) for p in at]
    assert any(p["reduce"] == "reduce_taps" and p["nsplit"] < 8 for p, _ in plans)
    assert any(p["reduce"] == "reduce_taps" and p["nsplit"] % 8 for p, _ in plans)
    assert any(p["kernel"] == "tapplane<16, 2, 3, 3>" for p, _ in plans)
    assert any(p["kernel"] == "tapplane<16, 1, 3, 3>" for p, _ in plans)


# ---------------------------------------------------------------------------------------------- 4. all-taps forms
@pytest.mark.parametrize("c1,c2,cout,ragged,name", [
    (48, 0, 48, False, "alltaps2<3, 3>"),        # the largest case of this file: 2 x 32 x 64 x 64 on a 256-CU device
    (96, 0, 96, True, "alltaps2<3, 3>"),         # 2 x 2 channel blocks, ragged in z, y and x
    (64, 0, 64, False, "alltaps2<4, 2>"),
    (32, 32, 128, True, "alltaps2<4, 2>"),
    (8, 0, 48, False, "alltaps2<3, 1>"),         # the first layer: one 16-channel ci block, 8 real channels
    (16, 0, 48, True, "alltaps2<3, 1>"),
    (8, 0, 64, False, "alltaps_kernel<1, 4>"),   # the first layer of a width-64 network
])
@pytest.mark.parametrize("dtype", [BF, FH])
def test_alltaps_wgrad_forms(dtype, c1, c2, cout, ragged, name):
    """Every all-taps kernel at the smallest volume (of a fixed candidate list) at which the mirror says it is taken."""
    n, size = R.smallest_alltaps_volume(c1, c2, cout, _ncu(), ragged)
    assert n * size[0] * size[1] * size[2] <= 2 * 32 * 64 * 64
    plan = _wgrad(R.wgrad_case(c1, c2, cout, n, size, 1), dtype, 1, 1)
    assert plan["kernel"] == name and not plan["memset"]


# ---------------------------------------------------------------------------------------------- 5. shifted-tap form
SHIFT = [  # cin, cout, k, dil, n, size
    (48, 24, 1, 1, 2, SMALL),
    (24, 48, 1, 1, 2, SMALL),          # padded ci lanes: the slab is cleared first
    (48, 24, 1, 1, 2, MID),
    (384, 96, 1, 1, 1, (8, 8, 16)),
    (32, 48, 3, 4, 1, (10, 12, 20)),
    (48, 32, 3, 6, 1, (10, 12, 20)),
    (24, 40, 3, 4, 2, SMALL),          # dilation wider than the volume's z extent, padded lanes
    (192, 192, 3, 4, 1, (8, 8, 16)),   # 27 taps x 36864 (co, ci) pairs: wgrad_reduce_taps_kernel behind the shifted-tap form
]


def _shift(dtype, cin, cout, k, dil, n, size, x3=None):
    from brats21_amd import _lib, ops
    x, _, dy, dw_ref, db_ref = R.wgrad_case(cin, 0, cout, n, size, dil, k)
    plan = R.wgrad_shift_plan(dtype != F32 or x3 is not None, k, cin, cout, n, *size)
    xd, dyd = _dv(x, dtype), _dv(dy, dtype)
    if x3 is None:
        ws = _lib.lib().brats_conv3d_wgrad_shift_ws_bytes(ops._code(dtype), k, n, *size, cin, cout)
        assert ws == plan["ws_bytes"], (ws, plan)
        dw, db = ops.conv3d_wgrad_shift(xd, dyd, k, dil, want_dbias=True)
        R.assert_exact(db, db_ref, what="dbias")
    else:
        amax = dyd.abs().max().reshape(1).float()
        assert float(amax) == 2.0
        with ops.split_precision(x3):
            dw, _ = ops.conv3d_wgrad_shift(xd, dyd, k, dil, amax_dy=amax)
    torch.cuda.synchronize()
    R.assert_exact(dw, dw_ref, what=f"dW {plan['kernel']} nsplit {plan['nsplit']} {plan['reduce']}")
    return plan


@pytest.mark.parametrize("cin,cout,k,dil,n,size", SHIFT)
@pytest.mark.parametrize("dtype", [BF, FH, F32])
def test_shifted_tap_wgrad(dtype, cin, cout, k, dil, n, size):
    """conv_wgrad_kernel<T, 1, COF, CIF, KS = 1>: 1x1x1 layers and 3x3x3 layers at dilation 4 and 6."""
    plan = _shift(dtype, cin, cout, k, dil, n, size)
    assert plan["memset"] == bool(cin % 16 or cout % 16)
    if (cin, cout) == (384, 96):
        assert plan["reduce"] == "reduce" and plan["nlane"] == 1   # one tap: never the all-taps reduction
    if (cin, cout) == (192, 192):
        assert plan["reduce"] == "reduce_taps"


# ---------------------------------------------------------------------------------------------- 6. split precision
@pytest.mark.parametrize("fused", [2, 0])
@pytest.mark.parametrize("c1,c2,cout,dil,n,size", [
    (48, 0, 48, 1, 1, (8, 16, 32)),
    (48, 48, 48, 1, 2, SMALL),
    (96, 0, 96, 1, 1, (5, 6, 19)),
    (8, 0, 48, 1, 2, (8, 8, 16)),       # the first layer
    (48, 0, 48, 1, 1, (20, 8, 16)),     # two z segments in the fused form
    (32, 0, 64, 2, 2, SMALL),           # never fused (dilation 2, not 48-blocks): three launches in either setting
])
@pytest.mark.parametrize("mode", ["x3_bf16", "x3_f16"])
def test_split_precision_wgrad(mode, c1, c2, cout, dil, n, size, fused):
    """brats_conv3d_x3_wgrad in the fused form (switch 2: any tile count) and as split pass + three 16-bit launches + one
    reduction over three slab groups (switch 0), integer f32 operands, amax_dy given.  The lo halves are zero here, so the
    lo x hi products contribute exact zeros: what is tested is the placement, the scaling by the power of two of amax and the
    summation.  The arithmetic of non-zero lo halves remains the business of tests/test_x3_gpu.py."""
    from brats21_amd import ops
    x, x2, dy, dw_ref, db_ref = R.wgrad_case(c1, c2, cout, n, size, dil)
    xd, x2d, dyd = _dv(x, F32), _dv(x2, F32), _dv(dy, F32)
    amax = torch.tensor([2.0], device=_dev())
    assert float(dy.abs().max()) == 2.0
    old = ops.set_x3_wgrad_fused(fused)
    try:
        with ops.split_precision(mode):
            dw, db = ops.conv3d_wgrad(xd, dyd, 3, dil, want_dbias=True, x2=x2d, amax_dy=amax)
        torch.cuda.synchronize()
    finally:
        ops.set_x3_wgrad_fused(old)
    R.assert_exact(dw, dw_ref, what=f"x3 dW fused={fused}")
    R.assert_exact(db, db_ref, what="dbias")


@pytest.mark.parametrize("cin,cout,k,dil,n,size", [SHIFT[0], SHIFT[1], SHIFT[4], SHIFT[5]])
def test_split_precision_shifted_tap_wgrad(cin, cout, k, dil, n, size):
    """conv3d_wgrad_shift in x3 mode (three runs of the 16-bit shifted-tap kernel into three slab groups)."""
    _shift(F32, cin, cout, k, dil, n, size, x3="x3_f16")


# ---------------------------------------------------------------------------------------------- 7. e4m3 forms
# f8_scale_from_amax (csrc/common.hpp) builds its result from an exponent field alone: a power of two, so x / scale and the
# per-row weight scales keep the integers exact (amax 2 -> scale 2^-6: the e4m3 values are 0, +-64, +-128).
@pytest.mark.parametrize("c1,c2,cout,size,n", [(48, 0, 48, (32, 64, 64), 2), (48, 48, 96, (16, 36, 60), 2),
                                               (64, 0, 64, (32, 32, 64), 2), (32, 32, 128, (10, 32, 64), 3)])
@pytest.mark.parametrize("dtype", [BF, FH])
def test_e4m3_wgrad(dtype, c1, c2, cout, size, n):
    from brats21_amd import ops
    x, x2, dy, dw_ref, _ = R.wgrad_case(c1, c2, cout, n, size, 1)
    xd, x2d, dyd = _dv(x, dtype), _dv(x2, dtype), _dv(dy, dtype)
    two = torch.tensor([2.0], device=_dev())
    assert float(x.abs().max()) == 2.0 and float(dy.abs().max()) == 2.0
    assert ops.conv3d_wgrad_f8_ok(xd, dyd, x2d)
    dw = ops.conv3d_wgrad_f8(xd, dyd, two, two, x2=x2d, amax2=two if c2 else None)
    torch.cuda.synchronize()
    R.assert_exact(dw, dw_ref, what="e4m3 dW")


@pytest.mark.parametrize("cin,cin2,cout,dil,size", [
    (48, 0, 48, 1, (8, 8, 16)), (48, 48, 48, 1, (12, 8, 20)), (48, 0, 96, 1, (8, 8, 32)), (96, 0, 192, 2, (8, 8, 16)),
    (16, 0, 32, 1, (8, 8, 16)), (32, 32, 64, 1, (4, 8, 16)), (64, 0, 16, 1, (4, 4, 4))])
@pytest.mark.parametrize("dtype", [BF, FH])
def test_e4m3_forward(dtype, cin, cin2, cout, dil, size):
    from brats21_amd import ops
    x, x2, w, bias, y_ref = R.fwd_case(cin, cin2, cout, 2, size, dil)
    two = torch.tensor([2.0], device=_dev())
    assert float(x.abs().max()) == 2.0
    wpk = ops.pack_weights_f8(w.to(_dev()), ops.PACK_FWD, c1=cin if cin2 else None)
    y, stats = ops.conv3d_f8(_dv(x, dtype), wpk, cout, dil, bias=bias.to(_dev()), want_stats=True, x2=_dv(x2, dtype), amax=two,
                             amax2=two if cin2 else None)
    torch.cuda.synchronize()
    R.assert_exact(y, y_ref, dtype, what="e4m3 y")
    R.assert_stats_exact(stats, y_ref, squares=R.stats_exact_ok(y_ref), what="e4m3 stats")


# ---------------------------------------------------------------------------------------------- 8. forward and input gradient
def _poison(numel, dtype=torch.float32):
    """Hands the caching allocator blocks full of NaN for the next torch.empty of this size, so that a statistics slot or output
    voxel the kernel leaves unwritten is not found holding an earlier, identical run's correct value."""
    blocks = [torch.full((numel,), float("nan"), dtype=dtype, device=_dev()) for _ in range(4)]
    torch.cuda.synchronize()
    del blocks


def _fwd(dtype, c1, c2, cout, n, size, dil=1, k=3, views=False, real_cin=None, out_slice=False, x3=None, chunk=None,
         with_bias=True, tile_stats=False, out_base=None, want_stats=True):
    """conv3d on integer operands: y bit-equal after rounding to the storage type, the tile statistics summed over the tiles
    equal to the reference's sums (sum of y on the dense operands; sum of y^2 on the dense operands where their reference meets
    the bound, otherwise on a second, thinned operand set).  tile_stats: the statistics are compared per tile instead
    (assert_tile_stats_exact, sum of y and of y^2), on the dense operands alone -- their per-tile bound is asserted, not worked
    around.  out_base (an element count): the dense output is a view that far into a flat buffer full of 7s (0: a prefilled
    tensor), so that a tile nobody writes is seen.  -> [(y, stats)] of the runs."""
    from brats21_amd import ops
    dev = _dev()
    dense = R.fwd_case(c1, c2, cout, n, size, dil, k, with_bias=with_bias, real_cin=real_cin)
    runs = [(dense, tile_stats or R.stats_exact_ok(dense[4]))]
    if not runs[0][1]:
        runs.append((R.fwd_case(c1, c2, cout, n, size, dil, k, thin=True, with_bias=with_bias, real_cin=real_cin), True))
    outs = []
    for (x, x2, w, bias, y_ref), squares in runs:
        xd = _dv(x, dtype, c1 + 16 if views else None, 8)
        x2d = _dv(x2, dtype, c2 + 8 if views else None, 0)
        with ops.split_precision(x3):
            if chunk is not None:
                assert ops.conv_chunk(ops._conv_dtype(dtype, k), k, dil, c1, c2, cout) == chunk
            wpk = ops.pack_weights(w.to(dev), dtype, ops.PACK_FWD, dil=dil, c1=c1 if c2 else None)
            out = None
            if out_slice:
                wide = torch.full((n, *size, cout + 48), 7.0, dtype=dtype, device=dev)
                out = wide[..., 16:16 + cout]
            elif out_base is not None:
                flat = torch.full((out_base + y_ref.numel() + 8,), 7.0, dtype=dtype, device=dev)
                out = flat[out_base:out_base + y_ref.numel()].view(n, *size, cout)
            if tile_stats and want_stats:
                _poison(n * ops.tiles_per_sample(*size) * cout * 2)
            y, stats = ops.conv3d(xd, wpk, cout, k, dil, bias=bias.to(dev) if with_bias else None, want_stats=want_stats, x2=x2d, out=out)
        torch.cuda.synchronize()
        R.assert_exact(y, y_ref, dtype, what=f"y {c1}+{c2}->{cout} k{k} d{dil}")
        if not want_stats:
            assert stats is None
        elif tile_stats:
            R.assert_tile_stats_exact(stats, y_ref, squares=True, what="tile statistics")
        else:
            R.assert_stats_exact(stats, y_ref, squares=squares, what="tile statistics")
        if out_slice:
            assert float(wide[..., :16].float().min()) == 7.0 and float(wide[..., 16 + cout:].float().max()) == 7.0
            assert float(wide[..., :16].float().max()) == 7.0 and float(wide[..., 16 + cout:].float().min()) == 7.0
        elif out_base is not None:
            assert y.data_ptr() == flat.data_ptr() + out_base * flat.element_size()
            assert bool((flat[:out_base].float() == 7.0).all()) and bool((flat[out_base + y_ref.numel():].float() == 7.0).all())
        outs.append((y, stats))
    return outs


def _dgrad(dtype, cin, cout, n, size, dil=1, k=3, x3=None):
    """The input gradient: the same kernels on weights packed with PACK_DGRAD (transposed, taps flipped)."""
    from brats21_amd import ops
    dy, w, dx_ref = R.dgrad_case(cin, cout, n, size, dil, k)
    with ops.split_precision(x3):
        wpk = ops.pack_weights(w.to(_dev()), dtype, ops.PACK_DGRAD, dil=dil)
        amax = torch.tensor([2.0], device=_dev()) if x3 else None
        dx, _ = ops.conv3d(_dv(dy, dtype), wpk, cin, k, dil, amax=amax)
    torch.cuda.synchronize()
    R.assert_exact(dx, dx_ref, dtype, what=f"dx {cout}->{cin} k{k} d{dil}")


@pytest.mark.parametrize("size,dil", [(SMALL, 1), (SMALL, 2), (MID, 1)])
@pytest.mark.parametrize("cin,cout", _FULL + _PADDED)
@pytest.mark.parametrize("dtype", [BF, FH, F32])
def test_tile_kernel_forward_and_input_gradient(dtype, cin, cout, size, dil):
    """The 4-wave tile kernel (16-bit) and the exact-f32 kernels at the channel shapes of item 1: forward with bias and tile
    statistics, channel-slice input views, and the input gradient through PACK_DGRAD."""
    _fwd(dtype, cin, 0, cout, 2, size, dil, views=(size == SMALL))
    _dgrad(dtype, cin, cout, 2, size, dil)


@pytest.mark.parametrize("dtype", [BF, FH, F32])
def test_padded_first_layer_forward(dtype):
    """4 real channels padded to 8 (zero x and zero weight columns) -> 48 into a channel slice of a wider output buffer: the
    tile kernel (the dense-output first-layer kernel is test_first_layer_and_cout48_kernels)."""
    _fwd(dtype, 8, 0, 48, 2, SMALL, real_cin=4, out_slice=True)
    _fwd(dtype, 8, 0, 48, 2, MID, real_cin=4, out_slice=True)


@pytest.mark.parametrize("kp", [0, 1])
@pytest.mark.parametrize("cin,cin2,cout,dil,size", [
    (384, 0, 384, 1, (16, 16, 16)), (384, 0, 384, 2, (16, 16, 16)), (384, 384, 192, 1, (16, 16, 16)), (192, 0, 96, 1, (10, 12, 20))])
@pytest.mark.parametrize("dtype", [BF, FH])
def test_k_parity_form_forward_and_input_gradient(dtype, cin, cin2, cout, dil, size, kp):
    """The 8-wave K-parity form of the small-grid launches and the 4-wave form of the same launches, each against the exact
    reference (so also bit-equal to each other), forward and -- single-source rows -- input gradient."""
    from brats21_amd import ops
    old = ops.set_kp(kp)
    try:
        _fwd(dtype, cin, cin2, cout, 2, size, dil, chunk=48)
        if not cin2:
            _dgrad(dtype, cin, cout, 2, size, dil)
    finally:
        ops.set_kp(old)


@pytest.mark.parametrize("vs8", [0, 1])
@pytest.mark.parametrize("cin,cin2,cout,n,size", [(48, 0, 48, 2, (32, 32, 32)), (48, 48, 48, 1, (12, 20, 40)), (96, 0, 144, 1, (8, 12, 16))])
@pytest.mark.parametrize("dtype", [BF, FH])
def test_vs8_form_forward_and_input_gradient(dtype, cin, cin2, cout, n, size, vs8):
    """The 4x8x16-tile kernel (24-channel chunks) and the 4x4x16-tile kernel on the same layers."""
    from brats21_amd import ops
    old = ops.set_vs8(vs8)
    try:
        _fwd(dtype, cin, cin2, cout, n, size, 1, chunk=24 if vs8 else None)
        if not cin2:
            _dgrad(dtype, cin, cout, n, size, 1)
    finally:
        ops.set_vs8(old)


@pytest.mark.parametrize("dtype", [BF, FH])
def test_first_layer_and_cout48_kernels(dtype):
    """The persistent first-layer kernel (8 -> 48, dense output) and the same call into a channel slice (the 4x8x16-tile kernel with
    an 8-channel chunk); the Cout = 48 kernels on a two-source ragged volume with the 4x8x16-tile switch on.  2 x (32, 64, 64) is
    1024 tiles, below the 2048 from which the library takes either first-layer kernel by itself: the pair runs with the
    threshold switched to 8, and the launch counters say which form ran (one launch per operand set).  The walk shapes of
    the persistent kernel are the business of tests/test_first_layer_gpu.py."""
    from brats21_amd import ops
    forms = (ops.CONV_FORM_FIRST, ops.CONV_FORM_VS8, ops.CONV_FORM_TILE)

    def count():
        return [ops.conv_form_launches(dtype, f) for f in forms]
    old_min, old_vs8 = ops.set_first_min_tiles(8), ops.set_vs8(1)
    try:
        c0 = count()
        new = _fwd(dtype, 8, 0, 48, 2, (32, 64, 64), real_cin=4)
        c1 = count()
        old = _fwd(dtype, 8, 0, 48, 2, (32, 64, 64), real_cin=4, out_slice=True)
        c2 = count()
    finally:
        ops.set_vs8(old_vs8)
        ops.set_first_min_tiles(old_min)
    assert [b - a for a, b in zip(c0, c1)] == [len(new), 0, 0], "the dense output must take the persistent first-layer kernel"
    assert [b - a for a, b in zip(c1, c2)] == [0, len(old), 0], "the channel slice must take the 4x8x16-tile kernel"
    assert len(new) == len(old) and all(torch.equal(a[0], b[0].contiguous()) for a, b in zip(new, old))
    old = ops.set_vs8(1)
    try:
        _fwd(dtype, 48, 48, 48, 1, (9, 21, 37), chunk=24)
    finally:
        ops.set_vs8(old)


@pytest.mark.parametrize("cin,cout,n,size", [(48, 24, 2, SMALL), (24, 48, 2, SMALL), (48, 24, 2, MID), (384, 96, 1, (8, 8, 16))])
@pytest.mark.parametrize("dtype", [BF, FH, F32])
def test_one_by_one_kernels(dtype, cin, cout, n, size):
    """The 1x1x1 kernels: forward with bias and statistics, and the input gradient."""
    _fwd(dtype, cin, 0, cout, n, size, 1, k=1)
    _dgrad(dtype, cin, cout, n, size, 1, k=1)


@pytest.mark.parametrize("cin,cin2,cout,dil,size", [
    (8, 0, 48, 1, (8, 8, 16)), (24, 0, 24, 1, (8, 12, 16)), (48, 0, 48, 1, (8, 16, 16)), (48, 48, 48, 1, (8, 8, 16)),
    (48, 0, 96, 1, (8, 8, 32)), (96, 0, 96, 2, (8, 8, 16)), (32, 0, 64, 1, (5, 6, 7)), (16, 0, 16, 1, (4, 4, 4))])
@pytest.mark.parametrize("mode", ["x3_f16", "x3_bf16"])
def test_split_precision_forward_and_input_gradient(mode, cin, cin2, cout, dil, size):
    """The x3 forward (f32 tensors, three 16-bit MFMA products; the lo halves are zero here) and its input gradient with the
    power-of-two input scale of a given amax."""
    _fwd(F32, cin, cin2, cout, 2, size, dil, x3=mode)
    if not cin2:
        _dgrad(F32, cin, cout, 2, size, dil, x3=mode)
