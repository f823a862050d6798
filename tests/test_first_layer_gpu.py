"""-m gpu: the two kernels of the networks' first layer (8 -> 48, 3x3x3, 16-bit) at the smallest volumes on which they can go
wrong, bit for bit (integer operands in [-2, 2] against the float64 shifted-GEMM reference of tests/_conv_exact_ref.py; no
tolerance anywhere in this file).

  * conv_first_kernel (csrc/conv_igemm_first.hpp), the persistent kernel of a dense output: its XCD-sliced tile walk with ragged
    slices, unequal trip counts, workgroups with one tile or none, a slice across the sample boundary, and the steady state of
    its halo prefetch;
  * conv_launch_vs8<8, 1, 3> (csrc/conv_igemm_vs8.hpp), the 4x8x16-tile kernel with an 8-channel chunk, which takes every other
    first-layer call: channel-slice outputs, ragged volumes, H = 4 (mod 8), unaligned outputs, no statistics.

By itself the library takes either only from 2048 tiles on (1 M voxels); brats_conv3d_set_first_min_tiles(8) brings them down to
volumes of a few thousand voxels.  What ran is asserted, never assumed: every launch is bracketed by readings of
brats_conv3d_form_launches.  What a volume is in the list for (R.first_walk_properties) is evaluated on a Python mirror of the
walk with the CU count of the device at hand and asserted before the run.

The dense output is a tensor prefilled with 7s (a tile nobody writes keeps them), the statistics are compared per tile
(R.assert_tile_stats_exact: sums in a wrong slot of the right sample fail) in a buffer the allocator was handed full of NaN."""
import contextlib

import pytest
import torch

import _conv_exact_ref as R
from test_conv_exact_gpu import _fwd, _ncu

pytestmark = pytest.mark.gpu

BF, FH = torch.bfloat16, torch.float16
FIRST, VS8, TILE = "first", "vs8", "tile"


@contextlib.contextmanager
def _switches(min_tiles, vs8):
    from brats21_amd import ops
    old_min, old_vs8 = ops.set_first_min_tiles(min_tiles), ops.set_vs8(vs8)
    try:
        yield
    finally:
        ops.set_vs8(old_vs8)
        ops.set_first_min_tiles(old_min)


def _run(dtype, n, size, real_cin, form, **kw):
    """One exact 8 -> 48 forward (_fwd: y, the 7s around it, the per-tile statistics) that must be exactly one launch of `form`."""
    from brats21_amd import ops
    forms = {FIRST: ops.CONV_FORM_FIRST, VS8: ops.CONV_FORM_VS8, TILE: ops.CONV_FORM_TILE}
    before = {k: ops.conv_form_launches(dtype, f) for k, f in forms.items()}
    outs = _fwd(dtype, 8, 0, 48, n, size, real_cin=real_cin, tile_stats=True, chunk=8, **kw)
    delta = {k: ops.conv_form_launches(dtype, f) - before[k] for k, f in forms.items()}
    assert len(outs) == 1
    assert delta == {k: int(k == form) for k in forms}, f"{n} x {size} {kw}: launches per form {delta}, expected one of '{form}'"
    return outs[0][0]


def _require_walk(ntiles, n, size):
    assert R.ntiles_of(n, size) == ntiles
    for what, holds in R.first_walk_properties(ntiles, n, _ncu()):
        assert holds, f"on {_ncu()} CUs the {ntiles}-tile volume no longer exercises: {what}"


@pytest.mark.parametrize("ntiles", sorted(R.FIRST_WALKS))
@pytest.mark.parametrize("real_cin", [4, 8])
@pytest.mark.parametrize("dtype", [BF, FH])
def test_persistent_kernel_walks(dtype, real_cin, ntiles):
    """The dense output on conv_first_kernel (with a bias; 36 and 1170 tiles without one too), then the same call into a channel
    slice on conv_launch_vs8<8, 1, 3> and on the 4x4x16-tile kernel: three kernels, one bit pattern."""
    n, size = R.FIRST_WALKS[ntiles]
    _require_walk(ntiles, n, size)
    for with_bias in (True, False) if ntiles in R.FIRST_NOBIAS else (True,):
        with _switches(8, 1):
            assert R.first_layer_form(n, size, 8) == FIRST and R.first_layer_form(n, size, 8, dense=False) == VS8
            dense = _run(dtype, n, size, real_cin, FIRST, out_base=0, with_bias=with_bias)
            sliced = _run(dtype, n, size, real_cin, VS8, out_slice=True, with_bias=with_bias)
            assert torch.equal(dense, sliced.contiguous())
        with _switches(8, 0):
            sliced = _run(dtype, n, size, real_cin, TILE, out_slice=True, with_bias=with_bias)
            assert torch.equal(dense, sliced.contiguous())


@pytest.mark.parametrize("n,size", R.FIRST_RAGGED)
@pytest.mark.parametrize("real_cin", [4, 8])
@pytest.mark.parametrize("dtype", [BF, FH])
def test_slice_kernel_on_ragged_volumes(dtype, real_cin, n, size):
    """Volumes conv_first_ok refuses (clipped tiles on every axis; H = 20: whole 4-row tiles, half an 8-row tile at the end, the
    y-half statistics of the 4x8x16 tile): conv_launch_vs8<8, 1, 3> is their only first-layer kernel, dense and sliced output."""
    assert (size[0] % 4 or size[1] % 4 or size[2] % 16) and R.ntiles_of(n, size) >= 8
    assert size != (12, 20, 40) or size[1] % 8 == 4
    with _switches(8, 1):
        assert R.first_layer_form(n, size, 8) == VS8
        dense = _run(dtype, n, size, real_cin, VS8, out_base=0)
        sliced = _run(dtype, n, size, real_cin, VS8, out_slice=True)
        assert torch.equal(dense, sliced.contiguous())


@pytest.mark.parametrize("real_cin", [4, 8])
@pytest.mark.parametrize("dtype", [BF, FH])
def test_persistent_kernel_refusals(dtype, real_cin):
    """What conv_first_ok must turn away with the threshold at 8: the persistent kernel's counter stays (asserted by _run: exactly
    one launch, of the named form) and the result is exact.
    7 tiles: below the threshold of 8 the ck == 8 rule leaves the call with the 4x4x16-tile kernel; with the threshold at 1 it is
    the explicit 8-tile term of conv_first_ok alone that keeps the launcher from an empty grid (7 & ~7 = 0), and the rule hands
    the call to the 4x8x16-tile kernel."""
    with _switches(8, 1):
        assert R.ntiles_of(1, (28, 4, 16)) == 7
        _run(dtype, 1, (28, 4, 16), real_cin, TILE, out_base=0)
        _run(dtype, 1, (12, 12, 24), real_cin, VS8, out_base=0)                     # W no multiple of 16
        # y not 16-byte aligned: a dense tensor 4 elements (8 bytes) into its buffer.  8 elements are 16 bytes: still aligned
        y = _run(dtype, 1, (8, 16, 16), real_cin, VS8, out_base=4)
        assert y.data_ptr() % 16 == 8
        y = _run(dtype, 1, (8, 16, 16), real_cin, FIRST, out_base=8)
        assert y.data_ptr() % 16 == 0
        _run(dtype, 1, (8, 16, 16), real_cin, VS8, out_base=0, want_stats=False)    # statistics not requested
    with _switches(1, 1):
        _run(dtype, 1, (28, 4, 16), real_cin, VS8, out_base=0)
    with _switches(1, 0):
        _run(dtype, 1, (28, 4, 16), real_cin, TILE, out_base=0)


@pytest.mark.parametrize("real_cin", [4, 8])
@pytest.mark.parametrize("dtype", [BF, FH])
def test_default_threshold(dtype, real_cin):
    """The library's own rule, the switch at its default: 2295 tiles (odd; four and five tiles per workgroup, a last slice one
    tile short) take the persistent kernel, 1755 tiles do not.  Pins the 2048."""
    from brats21_amd import ops
    (n1, s1), (n0, s0) = R.FIRST_DEFAULT
    assert R.ntiles_of(n0, s0) == 1755 < R.FIRST_MIN_TILES <= 2295
    _require_walk(2295, n1, s1)
    old = ops.set_first_min_tiles(0)
    try:
        assert old == R.FIRST_MIN_TILES, "a test before this one left the threshold switched"
        with _switches(0, 1):
            _run(dtype, n1, s1, real_cin, FIRST, out_base=0)
            _run(dtype, n0, s0, real_cin, TILE, out_base=0)
    finally:
        ops.set_first_min_tiles(old)
