"""-m gpu: the nearest-neighbour up-sampling kernels (csrc/nearest.hip; ops.upsample_nearest / upsample_nearest_bwd on NDHWC
activations, ops.planes_nearest / planes_nearest_bwd on f32 NCDHW planes) against torch's own F.interpolate(mode="nearest") and its
float64 autograd gradient.

The forward passes are copies: bit-equal in every storage type.  The adjoints are held to BITS too, on integer-valued gradients in
[-4, 4]: every partial sum of 8 (NDHWC) or up to 8^3 = 512 (planes; |sum| <= 2048 < 2^24) such values is an integer that f32 holds
exactly, and the NDHWC totals (|sum| <= 32) and their sums with an integer addend (|.| <= 36) are exact in bf16 (8 significant
bits: integers up to 256) and fp16 as well -- so the result does not depend on the summation order and equals the float64 gradient
cast to the storage type.  On random f32 gradients the 8-term sum is held to rtol 1e-6 of float64 (7 roundings of 2^-24 each on
the partial sums: 4.2e-7 of the sum of magnitudes; the tolerance is taken against that sum, which cancellation cannot shrink).

Coarse shapes: the smallest where the indexing can go wrong -- one voxel; odd extents with two samples and a channel count that is
no multiple of 16; several workgroups (a 72-voxel row of one channel vector is more than one pass of a 256-lane row in f32) -- the
last once more through a channel-slice view."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from brats21_amd import ops

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8, 1, 1, 1), (2, 24, 3, 5, 7), (1, 8, 6, 10, 72)]  # coarse (N, C, D, H, W)
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
PLANES = [(3, 1, 2, 3), (2, 3, 5, 9)]  # coarse (planes, D, H, W)


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v).split(".")[-1]


def _ints(shape, seed, lo=-4, hi=4):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _ndhwc(t_ncdhw, dtype):
    """[N, C, D, H, W] f32 on the CPU -> NDHWC `dtype` on the GPU (a fresh allocation: canonical strides for extents of 1 too)."""
    n, c, d, h, w = t_ncdhw.shape
    out = torch.empty((n, d, h, w, c), dtype=dtype, device="cuda")
    out.copy_(t_ncdhw.permute(0, 2, 3, 4, 1))
    return out


def _ref_bwd64(dy_ncdhw, scale):
    """float64 autograd gradient of F.interpolate(mode="nearest") for the output gradient dy."""
    n, c, d, h, w = dy_ncdhw.shape
    x = torch.zeros((n, c, d // scale, h // scale, w // scale), dtype=torch.float64, requires_grad=True)
    F.interpolate(x, scale_factor=scale, mode="nearest").backward(dy_ncdhw.double())
    return x.grad


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_forward_is_a_copy(shape, dtype):
    n, c, d, h, w = shape
    x = torch.randn(shape, generator=torch.Generator().manual_seed(1)).to(dtype)  # (the stored values are what is copied)
    want = F.interpolate(x.float(), scale_factor=2, mode="nearest").to(dtype).permute(0, 2, 3, 4, 1).contiguous()
    got = ops.upsample_nearest(_ndhwc(x.float(), dtype), 2)
    assert got.shape == (n, 2 * d, 2 * h, 2 * w, c) and got.dtype == dtype
    assert torch.equal(_bits(got.cpu()), _bits(want))
    assert torch.equal(_bits(ops.upsample_nearest(_ndhwc(x.float(), dtype), 2).cpu()), _bits(got.cpu())), "two runs differ"


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_backward_is_exact_on_integers(shape, dtype):
    n, c, d, h, w = shape
    dy = _ints((n, c, 2 * d, 2 * h, 2 * w), 2)
    add = _ints(shape, 3)
    g64 = _ref_bwd64(dy, 2)
    dyg, addg = _ndhwc(dy, dtype), _ndhwc(add, dtype)
    got = ops.upsample_nearest_bwd(dyg, 2)
    assert got.shape == (n, d, h, w, c) and got.dtype == dtype
    want = g64.to(dtype).permute(0, 2, 3, 4, 1).contiguous()
    assert torch.equal(_bits(got.cpu()), _bits(want))
    got_add = ops.upsample_nearest_bwd(dyg, 2, add=addg)
    want_add = (g64 + add.double()).to(dtype).permute(0, 2, 3, 4, 1).contiguous()
    assert torch.equal(_bits(got_add.cpu()), _bits(want_add))
    assert torch.equal(_bits(got_add), _bits(got + addg)), "add = the plain call followed by an elementwise add"
    assert torch.equal(_bits(ops.upsample_nearest_bwd(dyg, 2, add=addg)), _bits(got_add)), "two runs differ"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=_ids)
def test_backward_add_rounds_the_adjoint_first(dtype):
    """Non-integer values: the adjoint is rounded to the storage type BEFORE the addend is added (what a separate add computes)."""
    shape = SHAPES[1]
    n, c, d, h, w = shape
    g = torch.Generator().manual_seed(4)
    dy = _ndhwc(torch.randn((n, c, 2 * d, 2 * h, 2 * w), generator=g), dtype)
    add = _ndhwc(torch.randn(shape, generator=g), dtype)
    plain = ops.upsample_nearest_bwd(dy, 2)
    assert torch.equal(_bits(ops.upsample_nearest_bwd(dy, 2, add=add)), _bits(plain + add))
    # and the plain call is the f32 sum of the 8 stored children in the order (z, y, x offset), rounded once
    acc = None
    for a in range(2):
        for b in range(2):
            for e in range(2):
                t = dy[:, a::2, b::2, e::2].float()
                acc = t if acc is None else acc + t
    assert torch.equal(_bits(plain), _bits(acc.to(dtype)))


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_backward_random_f32(shape):
    n, c, d, h, w = shape
    dy = torch.randn((n, c, 2 * d, 2 * h, 2 * w), generator=torch.Generator().manual_seed(5))
    got = ops.upsample_nearest_bwd(_ndhwc(dy, torch.float32), 2).cpu().permute(0, 4, 1, 2, 3).double()
    mag = _ref_bwd64(dy.abs(), 2)
    err = float(((got - _ref_bwd64(dy, 2)).abs() / mag).max())
    print(f"  {shape}: max |got - f64| / sum |children| = {err:.2e}")
    assert err <= 1e-6


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_channel_slice_views_leave_their_neighbours_alone(dtype):
    n, c, d, h, w = SHAPES[2]
    vw = 16 // torch.empty((), dtype=dtype).element_size()
    lo, wide = 2 * vw, 5 * vw + c  # (the slice starts and ends on 16-byte vectors, like a concat buffer's parts)
    x = _ints(SHAPES[2], 6)
    dy = _ints((n, c, 2 * d, 2 * h, 2 * w), 7)
    add = _ndhwc(_ints(SHAPES[2], 8), dtype)
    # forward: out is a slice of a wider tensor, and so is the source
    src = torch.full((n, d, h, w, wide), 77.0, dtype=dtype, device="cuda")
    src[..., lo:lo + c] = _ndhwc(x, dtype)
    buf = torch.full((n, 2 * d, 2 * h, 2 * w, wide), -3.0, dtype=dtype, device="cuda")
    out = ops.upsample_nearest(src[..., lo:lo + c], 2, out=buf[..., lo:lo + c])
    assert out.data_ptr() == buf[..., lo:lo + c].data_ptr()
    assert torch.equal(_bits(buf[..., lo:lo + c]), _bits(ops.upsample_nearest(_ndhwc(x, dtype), 2)))
    assert bool((buf[..., :lo] == -3.0).all()) and bool((buf[..., lo + c:] == -3.0).all())
    # backward: dy, add and dx are slices
    dyb = torch.full((n, 2 * d, 2 * h, 2 * w, wide), 9.0, dtype=dtype, device="cuda")
    dyb[..., lo:lo + c] = _ndhwc(dy, dtype)
    addb = torch.full((n, d, h, w, wide), 5.0, dtype=dtype, device="cuda")
    addb[..., lo:lo + c] = add
    want = ops.upsample_nearest_bwd(_ndhwc(dy, dtype), 2, add=add)
    for with_add in (False, True):
        dxb = torch.full((n, d, h, w, wide), -3.0, dtype=dtype, device="cuda")
        ops.upsample_nearest_bwd(dyb[..., lo:lo + c], 2, add=addb[..., lo:lo + c] if with_add else None, out=dxb[..., lo:lo + c])
        ref = want if with_add else ops.upsample_nearest_bwd(_ndhwc(dy, dtype), 2)
        assert torch.equal(_bits(dxb[..., lo:lo + c]), _bits(ref))
        assert bool((dxb[..., :lo] == -3.0).all()) and bool((dxb[..., lo + c:] == -3.0).all())


def test_both_sides_of_the_non_temporal_switch():
    """The NDHWC pair streams its fine tensor with non-temporal accesses from 256 MiB on: 2 x 48 x 112^3 bf16 is 270 MB, one sample
    of it 135 MB.  Integer values, references formed on the GPU by torch (repeat_interleave; the f32 sum of the eight strided
    slices, exact here), and each sample of the large call equals the small call on that sample."""
    g = torch.Generator(device="cuda").manual_seed(18)
    x = torch.randint(-4, 5, (2, 56, 56, 56, 48), device="cuda", generator=g).to(torch.bfloat16)
    y = ops.upsample_nearest(x, 2)
    assert y.numel() * 2 >= (256 << 20) > y[0].numel() * 2
    assert torch.equal(y, x.repeat_interleave(2, 1).repeat_interleave(2, 2).repeat_interleave(2, 3))
    dy = torch.randint(-4, 5, tuple(y.shape), device="cuda", generator=g).to(torch.bfloat16)
    del y
    add = torch.randint(-4, 5, tuple(x.shape), device="cuda", generator=g).to(torch.bfloat16)
    want = sum(dy[:, a::2, b::2, e::2].float() for a in range(2) for b in range(2) for e in range(2))
    dx = ops.upsample_nearest_bwd(dy, 2)
    dxa = ops.upsample_nearest_bwd(dy, 2, add=add)
    assert torch.equal(dx.float(), want) and torch.equal(dxa.float(), want + add.float())
    for i in range(2):
        assert torch.equal(ops.upsample_nearest(x[i:i + 1], 2), ops.upsample_nearest(x, 2)[i:i + 1])
        assert torch.equal(ops.upsample_nearest_bwd(dy[i:i + 1], 2, add=add[i:i + 1]), dxa[i:i + 1])


@pytest.mark.parametrize("scale", [2, 4, 8])
@pytest.mark.parametrize("shape", PLANES, ids=_ids)
def test_planes_pair(shape, scale):
    p, d, h, w = shape
    low = torch.randn((1,) + shape, generator=torch.Generator().manual_seed(9))
    got = ops.planes_nearest(low.cuda(), scale)
    assert got.shape == (1, p, d * scale, h * scale, w * scale) and got.dtype == torch.float32
    assert torch.equal(_bits(got.cpu()), _bits(F.interpolate(low, scale_factor=scale, mode="nearest")))
    assert torch.equal(_bits(ops.planes_nearest(low.cuda(), scale)), _bits(got)), "two runs differ"
    # adjoint, integers: |sum| <= 4 * 8^3 = 2048 < 2^24, every partial sum exact
    dout = _ints(tuple(got.shape), 10)
    g64 = _ref_bwd64(dout, scale)
    back = ops.planes_nearest_bwd(dout.cuda(), scale)
    assert back.shape == low.shape and torch.equal(_bits(back.cpu()), _bits(g64.float()))
    assert torch.equal(_bits(ops.planes_nearest_bwd(dout.cuda(), scale)), _bits(back)), "two runs differ"
    # adjoint, random f32: scale^3 - 1 roundings of 2^-24 each at most, against the sum of magnitudes
    dout = torch.randn(tuple(got.shape), generator=torch.Generator().manual_seed(11))
    back = ops.planes_nearest_bwd(dout.cuda(), scale).cpu().double()
    err = float(((back - _ref_bwd64(dout, scale)).abs() / _ref_bwd64(dout.abs(), scale)).max())
    print(f"  planes {shape} x{scale}: max |got - f64| / sum |block| = {err:.2e}")
    assert err <= (scale ** 3 - 1) * 2.0 ** -24


def test_batched_planes_are_planes():
    """[N, K, ...] is N * K planes: two samples of three classes against torch."""
    low = torch.randn((2, 3, 2, 3, 5), generator=torch.Generator().manual_seed(12))
    assert torch.equal(ops.planes_nearest(low.cuda(), 4).cpu(), F.interpolate(low, scale_factor=4, mode="nearest"))


def test_capture_replays_the_eager_bits():
    n, c, d, h, w = SHAPES[1]
    x = _ndhwc(_ints(SHAPES[1], 13), torch.bfloat16)
    dy = _ndhwc(_ints((n, c, 2 * d, 2 * h, 2 * w), 14), torch.bfloat16)
    add = _ndhwc(_ints(SHAPES[1], 15), torch.bfloat16)
    low = _ints((2, 3, 2, 3, 5), 16).cuda()
    dlow = _ints((2, 3, 8, 12, 20), 17).cuda()

    def run():
        return (ops.upsample_nearest(x, 2), ops.upsample_nearest_bwd(dy, 2, add=add), ops.planes_nearest(low, 4),
                ops.planes_nearest_bwd(dlow, 4))

    eager = [t.clone() for t in run()]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        run()
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    for t in outs:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, outs):
        assert torch.equal(_bits(a), _bits(b))


def test_wrappers_refuse_what_the_kernels_do_not_take():
    from brats21_amd import BratsHipError
    x = torch.zeros((1, 2, 2, 2, 8), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(BratsHipError, match="scale"):
        ops.upsample_nearest(x, 4)
    with pytest.raises(BratsHipError, match="multiple of 8"):
        ops.upsample_nearest(torch.zeros((1, 2, 2, 2, 12), dtype=torch.bfloat16, device="cuda"), 2)
    with pytest.raises(ValueError, match="multiple of the scale"):
        ops.upsample_nearest_bwd(torch.zeros((1, 3, 2, 2, 8), dtype=torch.bfloat16, device="cuda"), 2)
    with pytest.raises(ValueError, match="addend"):
        ops.upsample_nearest_bwd(x, 2, add=torch.zeros((1, 1, 1, 1, 8), dtype=torch.float32, device="cuda"))
    with pytest.raises(BratsHipError, match="scale"):
        ops.planes_nearest(torch.zeros((1, 1, 2, 2, 2), device="cuda"), 3)
    with pytest.raises(ValueError, match="multiple of the scale"):
        ops.planes_nearest_bwd(torch.zeros((1, 1, 6, 8, 8), device="cuda"), 4)
