"""-m gpu: the narrow-output 3x3x3 convolution (csrc/conv_narrow.hip, ops.conv3d_narrow / ops.pack_weights_narrow) against the exact
integer-operand references of tests/_conv_exact_ref.py (tests/CONV_EXACT.md): operands are integers in [-2, 2], the reference is
a float64 shifted GEMM per tap, every partial sum is an exact f32 integer under the asserted preconditions, and the f32 result has
to equal the reference bit for bit.

The kernel's tile is 8 x 8 x 16 voxels with four consecutive x per thread and chunks of eight channels; its class tiles are 2, 4,
6, 8, 12, 16.  Volumes: (5, 6, 18) -- ragged and thinner than a tile on z and y, W % 4 != 0 (the scalar epilogue); (16, 16, 64) --
2 x 2 x 4 whole tiles (the 16-byte epilogue); (9, 10, 34) -- several workgroups on every axis with ragged last tiles.  n = 2 with
different samples throughout."""
import pytest
import torch

import _conv_exact_ref as E

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
THIN, WHOLE, RAGGED = (5, 6, 18), (16, 16, 64), (9, 10, 34)
# (C, K, volume, bias, add): every C of {8, 24, 48, 96} and K of {1, 3, 5, 16} on every volume; with / without bias and add
CASES = [
    (8, 1, THIN, True, True),
    (24, 3, THIN, False, True),
    (48, 5, THIN, True, False),
    (96, 16, THIN, True, True),
    (48, 3, WHOLE, True, True),
    (24, 16, WHOLE, False, False),
    (8, 5, WHOLE, True, True),
    (96, 1, WHOLE, True, False),
    (48, 3, RAGGED, True, True),
    (96, 16, RAGGED, False, True),
    (8, 5, RAGGED, True, False),
    (24, 1, RAGGED, False, False),
]


def _name(dt):
    return str(dt)[6:]


def _ids(c):
    return f"c{c[0]}_k{c[1]}_{'x'.join(map(str, c[2]))}{'_bias' if c[3] else ''}{'_add' if c[4] else ''}"


@pytest.fixture(autouse=True)
def _release():
    yield
    torch.cuda.empty_cache()


def _add(n, k, size, seed):
    return E.int_tensor((n, k, *size), 11000 + seed, amax=3)


def _want(y_ref, add):
    """NCDHW float64 from the channels-last reference (+ the residual)"""
    want = y_ref.permute(0, 4, 1, 2, 3).contiguous()
    if add is not None:
        assert float(add.abs().max()) + float(want.abs().max()) < E.EXACT
        want = want + add.double()
    return want


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_forward_exact(case, dtype):
    from brats21_amd import ops
    from brats21_amd._lib import PACK_FWD
    c, k, size, with_bias, with_add = case
    n = 2
    x, _, w, bias, y = E.fwd_case(c, 0, k, n, size, seed=c + k, with_bias=with_bias)
    assert not torch.equal(x[0], x[1])
    add = _add(n, k, size, c + k) if with_add else None
    dev = torch.device("cuda")
    got = ops.conv3d_narrow(x.to(dev, dtype), ops.pack_weights_narrow(w.to(dev), PACK_FWD), k,
                            bias=bias.to(dev) if with_bias else None, add=add.to(dev) if with_add else None)
    assert got.shape == (n, k, *size) and got.dtype == torch.float32
    E.assert_exact(got, _want(y, add), what=f"conv3d_narrow {_ids(case)} {_name(dtype)}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_channel_slice_of_a_wider_buffer(dtype):
    """x = channels [8, 32) of a 48-channel buffer whose other channels are NaN: nothing outside the slice is read."""
    from brats21_amd import ops
    from brats21_amd._lib import PACK_FWD
    c, k, n, size = 24, 3, 2, RAGGED
    x, _, w, bias, y = E.fwd_case(c, 0, k, n, size, seed=77)
    add = _add(n, k, size, 77)
    dev = torch.device("cuda")
    wide = torch.full((n, *size, 48), float("nan"), dtype=dtype, device=dev)
    wide[..., 8:32] = x.to(dev, dtype)
    view = wide[..., 8:32]
    assert not view.is_contiguous()
    got = ops.conv3d_narrow(view, ops.pack_weights_narrow(w.to(dev), PACK_FWD), k, bias=bias.to(dev), add=add.to(dev))
    E.assert_exact(got, _want(y, add), what=f"conv3d_narrow slice {_name(dtype)}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("cout,k,size", [(48, 3, RAGGED), (8, 5, THIN), (96, 16, THIN), (24, 1, WHOLE)],
                         ids=["48to3", "8to5", "96to16", "24to1"])
def test_input_gradient_packing_exact(cout, k, size, dtype):
    """PACK_DGRAD (weights [cout, k, 3, 3, 3] transposed, taps flipped) turns the kernel into the input gradient of a k -> cout
    convolution: against the scatter reference (E.dgrad_ref), with the gradient from elsewhere as `add`."""
    from brats21_amd import ops
    from brats21_amd._lib import PACK_DGRAD
    n = 2
    dy, w, dx = E.dgrad_case(k, cout, n, size, seed=cout + k)
    add = _add(n, k, size, cout)
    dev = torch.device("cuda")
    got = ops.conv3d_narrow(dy.to(dev, dtype), ops.pack_weights_narrow(w.to(dev), PACK_DGRAD), k, add=add.to(dev))
    E.assert_exact(got, _want(dx, add), what=f"conv3d_narrow dgrad {cout}->{k} {_name(dtype)}")


def test_arguments_outside_the_kernel_are_refused():
    from brats21_amd import ops
    from brats21_amd._lib import PACK_FWD, BratsHipError
    dev = torch.device("cuda")
    with pytest.raises(BratsHipError):
        ops.pack_weights_narrow(torch.zeros(17, 8, 3, 3, 3, device=dev), PACK_FWD)   # more than 16 class rows
    with pytest.raises(BratsHipError):
        ops.pack_weights_narrow(torch.zeros(3, 12, 3, 3, 3, device=dev), PACK_FWD)   # channels no multiple of 8
    wp = ops.pack_weights_narrow(torch.zeros(3, 8, 3, 3, 3, device=dev), PACK_FWD)
    with pytest.raises(BratsHipError):
        ops.conv3d_narrow(torch.zeros(1, 4, 4, 4, 16, device=dev), wp, 3)            # weights of another layer
    with pytest.raises(BratsHipError):
        ops.conv3d_narrow(torch.zeros(1, 4, 4, 4, 8, device=dev), wp, 3, add=torch.zeros(1, 3, 4, 4, 5, device=dev))
