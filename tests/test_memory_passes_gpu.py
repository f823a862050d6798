"""-m gpu: the up-sampling and deep-supervision-head passes beside the convolutions, bit for bit (torch.equal, no tolerance:
their arithmetic is fixed, only the number of trips through HBM changes).

  * the one-launch x2 trilinear adjoint of 16-bit NDHWC tensors against the three-pass form of the same library
    (brats_upsample_bwd_set_fused), bf16 and fp16, dense and channel-slice destinations, and an extent the tile form
    does not take;
  * the deep heads' x2 / x4 / x8 up-sampling to full size and its adjoint against a torch restatement of their documented
    order evaluated in f32 on the GPU: forward w = (wz * wy) * wx, sum over k = 0..7 (z, y, x bit order) ascending; adjoint
    per axis (D, then H, then W) the sum over ascending fine index l of w(l) * in[l] with w = [i0 == i] w0 + [i1 == i] w1.
    (The restatement was bit-equal to the gather / three-pass kernels these replaced before it was committed.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _rand(shape, seed, dev, dtype=torch.float32):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(shape, generator=g, device=dev, dtype=torch.float32).to(dtype)


# ---- item 1: fused x2 adjoint against the three-pass form --------------------------------------------------------------
def _upsample_bwd_raw(dy, dxbuf, c_off, c, fused):
    """brats_upsample_bwd into the channel slice [c_off, c_off + c) of dxbuf with the fused form forced on / off."""
    from brats21_amd import _lib, ops
    lib = _lib.lib()
    n, do, ho, wo, _ = dy.shape
    d, h, w = do // 2, ho // 2, wo // 2
    code = ops._code(dy.dtype)
    ws = torch.empty(lib.brats_upsample_bwd_ws_bytes(code, n, c, d, h, w, 2), dtype=torch.uint8, device=dy.device)
    dptr, _, dp = ops._desc(dy)
    dx = dxbuf[..., c_off:c_off + c]
    xptr, _, xp = ops._desc(dx)
    old = lib.brats_upsample_bwd_set_fused(fused)
    try:
        _lib.check(lib.brats_upsample_bwd(dptr, dp, xptr, xp, ws.data_ptr(), code, n, c, d, h, w, 2, ops._stream()), "upsample_bwd")
    finally:
        lib.brats_upsample_bwd_set_fused(old)
    torch.cuda.synchronize()
    return dx


def _check_fused(dtype, c, coarse, slice_dst, seed, src_slice=True):
    dev = _dev()
    n = 2
    d, h, w = coarse
    # the gradient is the second half of a concatenated input's gradient in the networks: a channel-slice source
    src = _rand((n, 2 * d, 2 * h, 2 * w, 2 * c if src_slice else c), seed, dev, dtype) * 1e-2
    dy = src[..., c:] if src_slice else src
    pitch, off = (c + 16, 8) if slice_dst else (c, 0)
    out = []
    for fused in (0, 1):
        buf = torch.full((n, d, h, w, pitch), 7.0, dtype=dtype, device=dev)
        _upsample_bwd_raw(dy, buf, off, c, fused)
        out.append(buf)
    assert torch.isfinite(out[0].float()).all()
    assert torch.equal(out[0], out[1]), f"fused x2 adjoint differs from the three-pass form: {dtype} C={c} coarse={coarse}"
    if slice_dst:  # the channels beside the slice are not touched
        assert bool((out[1][..., :off] == 7.0).all()) and bool((out[1][..., off + c:] == 7.0).all())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("edge", [8, 16, 32, 64])
def test_fused_adjoint_c48(dtype, edge):
    _check_fused(dtype, 48, (edge, edge, edge), False, 10 + edge)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("c,edge", [(96, 32), (192, 16), (384, 8), (96, 16), (192, 8)])
def test_fused_adjoint_network_levels(dtype, c, edge):
    _check_fused(dtype, c, (edge, edge, edge), False, 20 + edge + c)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_fused_adjoint_channel_slice_destination(dtype):
    _check_fused(dtype, 48, (16, 16, 16), True, 31)
    _check_fused(dtype, 96, (8, 16, 24), True, 32)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_fused_adjoint_falls_back_where_it_does_not_tile(dtype):
    _check_fused(dtype, 48, (6, 12, 10), False, 41)   # extents that are no multiple of the tile
    _check_fused(dtype, 40, (8, 8, 8), False, 42)     # a channel count that is no multiple of the channel slice


def test_fused_adjoint_is_the_adjoint():
    """<up(x), g> == <x, up^T(g)> in f64 from the bf16 results (a sanity check of the pair, beside the bit-equality above)."""
    from brats21_amd import ops
    dev = _dev()
    x = _rand((2, 16, 16, 16, 48), 51, dev, torch.bfloat16)
    g = _rand((2, 32, 32, 32, 48), 52, dev, torch.bfloat16)
    lhs = (ops.upsample(x, 2).double() * g.double()).sum()
    rhs = (x.double() * ops.upsample_bwd(g, 2).double()).sum()
    assert abs(float(lhs - rhs)) <= 2e-2 * abs(float(lhs)) + 1.0


# ---- items 2 and 3: the deep heads' up-sampling and its adjoint against the documented order ----------------------------
def _coef(out_len, in_len, dev):
    """lerp_coef of the kernels for every output index: f32 scale = (in - 1) / (out - 1), src = scale * o, i0 = (int)src ..."""
    scale = (torch.tensor(float(in_len - 1), dtype=torch.float32) / torch.tensor(float(out_len - 1), dtype=torch.float32)).to(dev)
    o = torch.arange(out_len, device=dev, dtype=torch.float32)
    src = scale * o
    i0 = src.to(torch.int32).clamp(max=in_len - 1)
    i1 = i0 + (i0 < in_len - 1).to(torch.int32)
    w1 = (src - i0.to(torch.float32)).clamp(0.0, 1.0)
    w0 = 1.0 - w1
    return i0.long(), i1.long(), w0, w1


def _up_restated(low, sc):
    """[P, D, H, W] f32 -> [P, D sc, H sc, W sc]: acc = 0; for k in 0..7: acc += ((wz * wy) * wx) * low[z_k, y_k, x_k]."""
    p, d, h, w = low.shape
    dev = low.device
    z0, z1, wz0, wz1 = _coef(d * sc, d, dev)
    y0, y1, wy0, wy1 = _coef(h * sc, h, dev)
    x0, x1, wx0, wx1 = _coef(w * sc, w, dev)
    acc = torch.zeros((p, d * sc, h * sc, w * sc), dtype=torch.float32, device=dev)
    for k in range(8):
        zi, wz = (z1, wz1) if k & 4 else (z0, wz0)
        yi, wy = (y1, wy1) if k & 2 else (y0, wy0)
        xi, wx = (x1, wx1) if k & 1 else (x0, wx0)
        wgt = (wz[:, None, None] * wy[None, :, None]) * wx[None, None, :]
        v = low[:, zi][:, :, yi][:, :, :, xi]
        acc = acc + wgt[None] * v
    return acc


def _adjoint_axis_restated(t, axis, in_len):
    """One axis of the adjoint: out[i] = sum over ascending l of w(l, i) * t[l], w = [i0 == i] w0 + [i1 == i] w1, zero weights skipped."""
    out_len = t.shape[axis]
    i0, i1, w0, w1 = (v.cpu() for v in _coef(out_len, in_len, t.device))
    t = t.movedim(axis, 0)
    acc = torch.zeros((in_len,) + tuple(t.shape[1:]), dtype=torch.float32, device=t.device)
    for l in range(out_len):
        a, b = int(i0[l]), int(i1[l])
        wa, wb = w0[l], w1[l]
        if a == b:
            wsum = (wa + wb).item()
            if wsum != 0.0:
                acc[a] = acc[a] + wsum * t[l]
            continue
        if wa.item() != 0.0:
            acc[a] = acc[a] + wa.item() * t[l]
        if wb.item() != 0.0:
            acc[b] = acc[b] + wb.item() * t[l]
    return acc.movedim(0, axis)


SHAPES = [(2, (16, 16, 16)), (4, (8, 8, 8)), (8, (4, 4, 4)), (2, (8, 12, 20)), (4, (4, 6, 10)), (8, (2, 3, 5)), (8, (16, 16, 16)),
          (4, (32, 32, 32)), (2, (64, 64, 64))]


@pytest.mark.parametrize("sc,low_shape", SHAPES)
def test_head_upsampling_matches_documented_order(sc, low_shape):
    """brats_head_fwd (scale > 1): its low-resolution logits are computed by the head's own 1x1x1 kernel (read back from the
    workspace), the planes up-sampled from them must equal the restated sum bit for bit."""
    from brats21_amd import _lib, ops
    dev = _dev()
    n, k, c = 2, 3, 16
    d, h, w = low_shape
    x = _rand((n, d, h, w, c), 61, dev, torch.bfloat16)
    wt = _rand((k, c), 62, dev).contiguous()
    b = _rand((k,), 63, dev)
    low = torch.empty((n, k, d, h, w), dtype=torch.float32, device=dev)
    out = torch.empty((n, k, d * sc, h * sc, w * sc), dtype=torch.float32, device=dev)
    ptr, _, p = ops._desc(x)
    _lib.check(_lib.lib().brats_head_fwd(ptr, p, wt.data_ptr(), b.data_ptr(), low.data_ptr(), out.data_ptr(), ops._code(x.dtype), n, c, k,
                                         d, h, w, sc, ops._stream()), "head_fwd")
    torch.cuda.synchronize()
    want = _up_restated(low.reshape(n * k, d, h, w), sc).reshape(out.shape)
    assert torch.isfinite(out).all()
    assert torch.equal(out, want), f"x{sc} head up-sampling of {low_shape}: max abs diff {float((out - want).abs().max()):.3e}"


@pytest.mark.parametrize("sc,low_shape", SHAPES)
def test_head_adjoint_matches_documented_order(sc, low_shape):
    """brats_head_bwd (scale > 1): the low-resolution logit gradient it leaves at the start of its workspace must equal the
    restated per-axis adjoint (D, then H, then W; ascending fine index) of dout bit for bit."""
    from brats21_amd import _lib, ops
    dev = _dev()
    n, k, c = 2, 3, 16
    d, h, w = low_shape
    x = _rand((n, d, h, w, c), 71, dev, torch.bfloat16)
    wt = _rand((k, c), 72, dev).contiguous()
    dout = _rand((n, k, d * sc, h * sc, w * sc), 73, dev)
    ws = torch.zeros(_lib.lib().brats_head_bwd_ws_bytes(n, c, k, d, h, w, sc) // 4, dtype=torch.float32, device=dev)
    dx = torch.empty_like(x)
    dw = torch.empty((k, c), dtype=torch.float32, device=dev)
    db = torch.empty(k, dtype=torch.float32, device=dev)
    ptr, _, p = ops._desc(x)
    _lib.check(_lib.lib().brats_head_bwd(ptr, p, wt.data_ptr(), dout.data_ptr(), ws.data_ptr(), dx.data_ptr(), c, dw.data_ptr(),
                                         db.data_ptr(), ops._code(x.dtype), n, c, k, d, h, w, sc, ops._stream()), "head_bwd")
    torch.cuda.synchronize()
    got = ws[:n * k * d * h * w].reshape(n * k, d, h, w)
    t = dout.reshape(n * k, d * sc, h * sc, w * sc)
    for axis, ln in ((1, d), (2, h), (3, w)):
        t = _adjoint_axis_restated(t, axis, ln)
    assert torch.equal(got, t), f"x{sc} head adjoint to {low_shape}: max abs diff {float((got - t).abs().max()):.3e}"
    # ... and what the head makes of it: db = the ordered sum of that gradient is checked against f64 loosely (its own order
    # is pinned by tests/test_ops_gpu.py)
    ref_db = t.reshape(n, k, -1).double().sum((0, 2))
    assert torch.allclose(db.double(), ref_db, rtol=1e-3, atol=1e-3)
