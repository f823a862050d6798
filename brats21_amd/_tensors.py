"""The check layer between PyTorch tensors and the C ABI of libbrats_hip.so: the library indexes memory from raw pointers and a
few integers, so whatever is not checked here is read or written out of bounds on the device.  Every pointer an entry point
receives comes out of one of these helpers, or from a tensor the wrapper allocated itself ("Who guards which pointer")."""
import torch

from . import _lib
from ._lib import BF16, F16, F32, X3_BF16, X3_F16

X3F = "x3_f16"    # operands split into fp16 pairs: f32-class products inside fp16's range (the forward pass)
X3B = "x3_bf16"   # ... into bf16 pairs: 2^-16 per product over f32's whole range (the gradients)


def _code(dtype):
    if dtype == X3F:
        return X3_F16
    if dtype == X3B:
        return X3_BF16
    if dtype == torch.bfloat16:
        return BF16
    if dtype == torch.float32:
        return F32
    if dtype == torch.float16:
        return F16
    raise _lib.BratsHipError(f"unsupported activation dtype {dtype}")


def _w(what):
    """The label of an argument in a message: a string, or (wrapper, argument), which costs a valid call no formatting."""
    return what if isinstance(what, str) else ": ".join(_w(p) for p in what)


class _Act:
    """A checked NDHWC activation (or channel-slice view) as the entry points take it: pointer, channel pitch, dims, dtype code."""
    __slots__ = ("t", "ptr", "pitch", "n", "d", "h", "w", "c", "shape", "vox", "dtype", "code", "device")


_NO_ACT = _Act()  # an absent optional source: null pointer, zero channels and pitch
_NO_ACT.t, _NO_ACT.ptr, _NO_ACT.pitch, _NO_ACT.c = None, None, 0, 0


def _act(t, what="tensor", like=None, shape=None, dtype=None, anyc=False, exc=_lib.BratsHipError):
    """Check t: a CUDA tensor [N, D, H, W, C], NDHWC with a channel pitch, of a storage dtype _code accepts; with like (an _Act):
    on its device, of its shape (anyc: any channel count) and dtype unless shape / dtype name others.  exc: what a shape or dtype
    mismatch raises."""
    if not isinstance(t, torch.Tensor) or t.dim() != 5 or not t.is_cuda:
        raise _lib.BratsHipError((what, "expected a CUDA tensor of shape [N, D, H, W, C]"))
    a = _Act()
    a.shape = n, d, h, w, c = tuple(t.shape)
    s0, s1, s2, p, s4 = t.stride()
    if s4 != 1 or s2 != w * p or s1 != h * w * p or s0 != d * h * w * p:
        raise _lib.BratsHipError(f"{_w(what)} is not NDHWC with a channel pitch: shape {a.shape} strides {t.stride()}")
    a.t, a.ptr, a.pitch, a.n, a.d, a.h, a.w, a.c, a.vox = t, t.data_ptr(), p, n, d, h, w, c, d * h * w
    a.dtype, a.code, a.device = t.dtype, _code(t.dtype), t.device
    if like is not None:
        if a.device != like.device:
            raise _lib.BratsHipError(f"{_w(what)} is on {a.device}, the input on {like.device}")
        shape, dtype = shape or (like.shape[:4] + (c,) if anyc else like.shape), dtype or like.dtype
    if (shape is not None and a.shape != tuple(shape)) or (dtype is not None and a.dtype != dtype):
        raise exc(f"{_w(what)} {a.shape} {a.dtype} does not match {tuple(shape or a.shape)} {dtype or a.dtype}")
    return a


def _act2(t, what, like, **kw):
    """_act of an optional further source; _NO_ACT (null pointer, zero channels and pitch) without one."""
    return _act(t, what, like, **kw) if t is not None else _NO_ACT


def _out(out, shape, like, what, dtype=None, exc=_lib.BratsHipError):
    """The activation a wrapper writes: a fresh tensor of `shape`, or the caller's `out` checked against it (a channel-slice view of
    a wider buffer is fine).  dtype and device are those of like, the wrapper's primary _Act."""
    if out is None:
        out = torch.empty(shape, dtype=dtype or like.dtype, device=like.device)
    return _act(out, what, like, shape=shape, dtype=dtype, exc=exc)


def _desc(t):
    """(data_ptr, C, pitch) of an NDHWC tensor or channel-slice view."""
    a = _act(t)
    return a.ptr, a.c, a.pitch


def _desc2(t):
    """_desc of an optional second source (the virtual concat [x | x2]); (None, 0, 0) without one."""
    return _desc(t) if t is not None else (None, 0, 0)


def _vec(t, numel, what, like, dtype=torch.float32, null=False, at_least=False):
    """Pointer of an operand the kernel indexes flat (the small per-sample vectors of ops.py; outside it also whole targets,
    label maps and fields the size of the logits): a contiguous CUDA tensor of `dtype` on like's device holding exactly (at_least: at least) the
    `numel` elements the kernel indexes (numel None: any).  None passes only where the entry point takes a null pointer."""
    if t is None:
        if null:
            return None
        raise _lib.BratsHipError((what, "missing"))
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_contiguous() or not t.is_cuda:
        raise _lib.BratsHipError(f"{_w(what)}: expected a contiguous CUDA {str(dtype).replace('torch.', '')} tensor")
    if like is not None and t.device != like.device:
        raise _lib.BratsHipError(f"{_w(what)} is on {t.device}, the input on {like.device}")
    if numel is not None and t.numel() != numel and not (at_least and t.numel() > numel):
        raise _lib.BratsHipError(f"{_w(what)} has {t.numel()} elements {tuple(t.shape)}, the kernel reads {numel}")
    return t.data_ptr()


def _f32(t):
    return _vec(t, None, "operand", None, null=True)


def _tile_stats(t, a, c, what):
    """Pointer of per-tile statistics [N, tiles >= 1, c, 2] f32 (the tile count is passed on to the kernel as shape[1])."""
    if not isinstance(t, torch.Tensor) or t.dim() != 4 or tuple(t.shape) != (a.n, max(1, t.shape[1]), c, 2):
        raise _lib.BratsHipError(f"{_w(what)}: expected [N, tiles, C, 2] = {(a.n, '>= 1', c, 2)}, got {tuple(getattr(t, 'shape', ()))}")
    return _vec(t, None, what, a)


def _planes(t, what, like=None, shape=None):
    """A plane tensor [N, K, D, H, W] (logits, their gradient) as contiguous f32; with like: on its device and of `shape`."""
    if not isinstance(t, torch.Tensor) or t.dim() != 5 or not t.is_cuda or not t.is_floating_point():
        raise _lib.BratsHipError((what, "expected a floating-point CUDA tensor of shape [N, K, D, H, W]"))
    if like is not None and (t.device != like.device or tuple(t.shape) != tuple(shape)):
        raise _lib.BratsHipError(f"{_w(what)}: {tuple(t.shape)} on {t.device} does not match {tuple(shape)} on {like.device}")
    return t.contiguous().float()


def _head_weight(weight, a, what):
    """The 1x1x1 head weight [K, C, 1, 1, 1] (or [K, C]) over the activation a's C channels -> (K, [K, C] f32 contiguous)."""
    if (not isinstance(weight, torch.Tensor) or weight.dim() not in (2, 5) or weight.shape[1] != a.c or weight[0, 0].numel() != 1
            or not weight.is_floating_point() or weight.device != a.device):
        raise _lib.BratsHipError(f"{_w(what)}: head weight {tuple(getattr(weight, 'shape', ()))} is no floating-point [K, {a.c}, 1, 1, 1] "
                                 f"tensor on {a.device}")
    k = weight.shape[0]
    return k, weight.detach().reshape(k, a.c).contiguous().float()


_SIZES = {}  # (what, integer arguments) -> the size the library states: a memo of integer-only size queries, filled by the pack_*
# functions from the query they make anyway, so that a check in a steady-state step costs no library call.  The packed sizes
# depend on brats_conv3d_chunk: a setter that changes its answers (today only set_vs8) must clear this memo, as set_vs8 does,
# or valid calls are refused


def _size(key, query):
    v = _SIZES.get(key)
    if v is None:
        v = _SIZES[key] = query()
    return v


def _packed(pw, key, query, what, like, dtype=torch.uint8):
    """Pointer of a packed-weight buffer: on like's device and of exactly the size the library states for the layer `key`
    (what the pack_* functions and PackPlan hand out; a buffer of another size was packed for another layer)."""
    nbytes = _size(key, query)
    if (not isinstance(pw, torch.Tensor) or not pw.is_cuda or pw.device != like.device or pw.dtype != dtype or not pw.is_contiguous()
            or pw.numel() * pw.element_size() != nbytes):
        raise _lib.BratsHipError(f"{_w(what)}: the packed weights are no contiguous {dtype} buffer of {nbytes} bytes on {like.device}")
    return pw.data_ptr()


def _conv_packed(pw, code, ksize, dil, c1, c2, cout, what, like):
    def query():
        ck = _lib.lib().brats_conv3d_chunk(code, ksize, dil, c1, c2, cout)
        return _lib.lib().brats_conv3d_packed_bytes(code, ksize, c1 + c2, cout, ck) if ck > 0 else 0
    return _packed(pw, ("conv", code, ksize, dil, c1, c2, cout), query, what, like)


def _even(a, what):
    if a.d % 2 or a.h % 2 or a.w % 2:
        raise _lib.BratsHipError(f"{_w(what)}: D, H, W = {a.d}, {a.h}, {a.w} must be even")
    return (a.n, a.d // 2, a.h // 2, a.w // 2)


def _groups(c, groups, what):
    if groups < 1 or c % groups:
        raise _lib.BratsHipError(f"{_w(what)}: {c} channels in {groups} groups")


def _finalize_in(stats, n, c, groups, what):
    """The checked inputs of a statistics finaliser: per-tile statistics [n, tiles >= 1, c, 2] -> (pointer, tiles)."""
    _groups(c, groups, what)
    if not isinstance(stats, torch.Tensor) or stats.dim() != 4 or stats.shape[1] < 1 or tuple(stats.shape) != (n, stats.shape[1], c, 2):
        raise _lib.BratsHipError(f"{_w(what)}: stats {tuple(getattr(stats, 'shape', ()))} is not [N, tiles, C, 2] = ({n}, >= 1, {c}, 2)")
    return _vec(stats, None, (what, "stats"), None), stats.shape[1]
