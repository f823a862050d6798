"""Raw (non-autograd) Python entry points over the C ABI of libbrats_hip.so.

Activations are torch CUDA tensors of shape [N, D, H, W, C] (NDHWC) in torch.bfloat16 or
torch.float32; a tensor may be a channel-slice *view* of a wider buffer (pitch = stride(3)), which
is how torch.cat (networks/equiunet2020.py:478-486 of the reference) is removed.  PyTorch is only
the allocator / stream provider here; every arithmetic op is a HIP kernel of the library.
"""
import contextlib
import weakref

import numpy as np
import torch

from . import _lib
from ._lib import ACT_LEAKY, ACT_NONE, ACT_RELU, BF16, F16, F32, PACK_DGRAD, PACK_FWD, X3_BF16, X3_F16  # noqa: F401

ACTS = {"none": ACT_NONE, "relu": ACT_RELU, "leakyrelu": ACT_LEAKY, "elu": _lib.ACT_ELU, "swish": _lib.ACT_SWISH,
        "mish": _lib.ACT_MISH}


class KernelTimer:
    """Optional HIP-event timing of individual library launches on the launch stream (bench.py's
    live roofline measurement).  ops.TIMER = KernelTimer() enables it; None (default) costs nothing."""

    def __init__(self):
        self.records = {}  # key -> list of (start_event, end_event)

    def span(self, key):
        return _Span(self, key)

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for key, evs in self.records.items():
            ms = [a.elapsed_time(b) for a, b in evs]
            out[key] = (len(ms), sum(ms) / len(ms), sum(ms))
        return out


class _Span:
    def __init__(self, timer, key):
        self.timer, self.key = timer, key

    def __enter__(self):
        self.a = torch.cuda.Event(enable_timing=True)
        self.b = torch.cuda.Event(enable_timing=True)
        self.a.record()  # current stream == the stream the library launches on (_stream())

    def __exit__(self, *exc):
        self.b.record()
        self.timer.records.setdefault(self.key, []).append((self.a, self.b))


class _NoSpan:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


TIMER = None
_NOSPAN = _NoSpan()


def _span(*key):
    return TIMER.span(key) if TIMER is not None else _NOSPAN


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_GET_DEVICE = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    """The current HIP stream of the current device as an integer handle.  torch.cuda.current_stream().cuda_stream builds a Python
    Stream object per call (~3 us, ~250 calls per training step: 0.7 ms of host time); the raw accessor is what torch's own
    generated code uses."""
    if _RAW_STREAM is not None and _GET_DEVICE is not None:
        return _RAW_STREAM(_GET_DEVICE())
    return torch.cuda.current_stream().cuda_stream


# ---- split precision ("x3"): f32 tensors, 3x3x3 convolutions on three 16-bit MFMA products (csrc/conv_igemm_x3.hpp) ----
X3F = "x3_f16"    # operands split into fp16 pairs: f32-class products inside fp16's range (the forward pass)
X3B = "x3_bf16"   # ... into bf16 pairs: 2^-16 per product over f32's whole range (the gradients)
_X3 = None        # the split the 3x3x3 convolutions of f32 tensors use inside a split_precision() block; None = exact f32


@contextlib.contextmanager
def split_precision(mode):
    """Inside the block conv3d / conv3d_wgrad / pack_weights run f32 tensors' 3x3x3 convolutions on the split-precision
    kernels (mode = ops.X3F or ops.X3B; None = the exact-f32 MFMA kernels).  The network programs open it around their
    forward (X3F) and backward (X3B) when model.precision = "x3"."""
    global _X3
    if mode not in (None, X3F, X3B):
        raise _lib.BratsHipError(f"split_precision: unknown mode {mode!r}")
    old, _X3 = _X3, mode
    try:
        yield
    finally:
        _X3 = old


def x3_active():
    return _X3 is not None


def x3_mode():
    return _X3


def _conv_dtype(dtype, ksize):
    """The kernel family a convolution of `dtype` tensors runs on: the dtype itself, or the active split mode."""
    if _X3 is not None and dtype == torch.float32 and ksize == 3:
        return _X3
    return dtype


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


def is16(dtype):
    """16-bit storage (bf16 or fp16): the MFMA kernels with f32 accumulation; fp16 is the reference's autocast dtype."""
    return dtype in (torch.bfloat16, torch.float16)


def _fn16(name, dtype):
    """Entry points that move 16-bit data but have no dtype argument exist twice: brats_x (bf16) and brats_x_f16."""
    return getattr(_lib.lib(), name + ("_f16" if dtype == torch.float16 else ""))


def _desc(t):
    """(data_ptr, C, pitch) of an NDHWC tensor or channel-slice view."""
    if t.dim() != 5 or not t.is_cuda:
        raise _lib.BratsHipError("expected a CUDA tensor of shape [N, D, H, W, C]")
    n, d, h, w, c = t.shape
    p = t.stride(3)
    if t.stride(4) != 1 or t.stride(2) != w * p or t.stride(1) != h * w * p or t.stride(0) != d * h * w * p:
        raise _lib.BratsHipError(f"tensor is not NDHWC with a channel pitch: shape {tuple(t.shape)} strides {t.stride()}")
    return t.data_ptr(), c, p


def _desc2(t):
    """_desc of an optional second source (the virtual concat [x | x2]); (None, 0, 0) without one."""
    return _desc(t) if t is not None else (None, 0, 0)


def _f32(t):
    if t is None:
        return None
    if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
        raise _lib.BratsHipError("expected a contiguous CUDA float32 tensor")
    return t.data_ptr()


def new_act(n, d, h, w, c, dtype, device):
    return torch.empty((n, d, h, w, c), dtype=dtype, device=device)


# ------------------------------------------------------------------------------------------ layout
def ncdhw_to_ndhwc(x, dtype, cpad=None):
    """[N,C,D,H,W] f32 -> [N,D,H,W,cpad] dtype (extra channels zero)."""
    n, c, d, h, w = x.shape
    cpad = cpad or c
    x = x.contiguous().float()
    out = new_act(n, d, h, w, cpad, dtype, x.device)
    _lib.check(_lib.lib().brats_ncdhw_to_ndhwc(x.data_ptr(), out.data_ptr(), _code(dtype), n, c, cpad, cpad, d, h, w,
                                               _stream()), "ncdhw_to_ndhwc")
    return out


def ndhwc_to_ncdhw(x):
    ptr, c, p = _desc(x)
    n, d, h, w, _ = x.shape
    out = torch.empty((n, c, d, h, w), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().brats_ndhwc_to_ncdhw(ptr, p, out.data_ptr(), _code(x.dtype), n, c, d, h, w, _stream()),
               "ndhwc_to_ncdhw")
    return out


# ------------------------------------------------------------------------------------------ conv
def conv_chunk(dtype, ksize, dil, c1, c2=0, cout=0):
    """K chunk of the kernel that will run a layer with c1 (+c2) input channels and `cout` GEMM rows."""
    ck = _lib.lib().brats_conv3d_chunk(_code(dtype), ksize, dil, c1, c2, cout)
    if ck <= 0:
        raise _lib.BratsHipError(f"conv3d: no channel chunk for c1={c1} c2={c2} dtype={dtype}")
    return ck


_PACK_CACHE = {}  # inference only: packed weights keyed by (tensor object, layout arguments); validated by the version
# counter, the address AND the generation below (writes through ``p.data`` -- the reference's Ranger2020 updates its
# weights with ``p.data.copy_``, learning/optimizer.py:243,253 -- do not bump a parameter's version counter)
_PACK_GEN = 0
_PACK_KEEP = None  # list collecting every packed buffer handed out while a hipGraph of the forward is being built


def invalidate_packed_weights():
    """Drop every cached packed-weight buffer.  Called by the network modules whenever their weights may have changed
    without a version bump: on every grad-enabled (training) forward and on every train() / eval() transition.  Call it
    yourself after writing weights through ``p.data`` between two no_grad forwards of an eval-mode model."""
    global _PACK_GEN
    _PACK_GEN += 1
    _PACK_CACHE.clear()


def pack_generation():
    return _PACK_GEN


@contextlib.contextmanager
def keep_packed(sink):
    """Every buffer pack_weights() / pack_weights_f8() returns inside the block is appended to ``sink``: a captured
    hipGraph bakes the buffers' addresses in, so its owner must keep them alive (inferers.GraphedPredictor)."""
    global _PACK_KEEP
    old, _PACK_KEEP = _PACK_KEEP, sink
    try:
        yield sink
    finally:
        _PACK_KEEP = old


def _cache_get(key, w):
    hit = _PACK_CACHE.get(key)
    if hit is not None and hit[0]() is w and hit[1] == w._version and hit[2] == w.data_ptr() and hit[4] == _PACK_GEN:
        if _PACK_KEEP is not None:
            _PACK_KEEP.append(hit[3])
        return hit[3]
    return None


def _cache_put(key, w, packed):
    if len(_PACK_CACHE) >= 1024:
        _PACK_CACHE.clear()
    _PACK_CACHE[key] = (weakref.ref(w), w._version, w.data_ptr(), packed, _PACK_GEN)
    if _PACK_KEEP is not None:
        _PACK_KEEP.append(packed)


def _pack_geometry(w, mode, cin_pad=None, cin_off=0, cin_cnt=None, c1=None):
    """Of packing w [Cout, Cin, k, k, k]: (cin_w, cnt, kdim, rows, src) -- the input channels after zero-padding to cin_pad, the
    size of the slice [cin_off, cin_off + cnt) that is packed, the GEMM's K and rows by mode, and src = (c1, c2): the channels of
    the (possibly two-source) input the kernel will read, which decide about its K chunk."""
    cin_w = cin_pad if cin_pad is not None else w.shape[1]
    cnt = cin_w - cin_off if cin_cnt is None else cin_cnt
    kdim, rows = (cnt, w.shape[0]) if mode == PACK_FWD else (w.shape[0], cnt)
    return cin_w, cnt, kdim, rows, ((kdim, 0) if (c1 is None or mode != PACK_FWD) else (c1, kdim - c1))


def _padded(w, cin_w):
    """w detached, contiguous f32, its input channels zero-padded to cin_w."""
    w = w.detach()
    if cin_w != w.shape[1]:
        wp = torch.zeros((w.shape[0], cin_w) + tuple(w.shape[2:]), dtype=torch.float32, device=w.device)
        wp[:, :w.shape[1]] = w
        w = wp
    return w.contiguous().float()


_PACK_JOB = np.dtype([("w", "<u8"), ("out", "<u8"), ("dtype", "<i4"), ("mode", "<i4"), ("taps", "<i4"), ("cin_w", "<i4"),
                      ("cin_real", "<i4"), ("cin_off", "<i4"), ("rows", "<i4"), ("rows16", "<i4"), ("kdim", "<i4"), ("ck", "<i4"),
                      ("ms_n", "<i4"), ("reserved", "<i4"), ("total", "<u8")])  # == brats_pack_job (include/brats_hip.h)


class PackPlan:
    """Every packed-weight buffer a training step needs (each layer: forward and dgrad layout) as views of ONE allocation,
    filled by ONE launch per step (brats_conv3d_pack_weights_multi) instead of one ~9 us launch per layer and layout.

    The first step runs the ordinary per-layer path and records what was asked for; ``run()`` (called by the module at the
    start of a training forward) then builds the tables once and re-packs everything each step.  ``pack_weights`` hands
    out a view only while the parameter is the same object, at the same address, with the version counter ``run()`` saw;
    anything else falls back to the per-layer path (and is added to the plan)."""

    def __init__(self):
        self.recorded = {}   # key -> (weakref(w), args)
        self.entries = None  # key -> [weakref(w), data_ptr, offset, nbytes, version]
        self.dirty = True

    def record(self, key, w, args):
        if isinstance(w, torch.nn.Parameter) and key not in self.recorded:  # (temporaries would never hit again)
            self.recorded[key] = (weakref.ref(w), args)
            self.dirty = True

    def _build(self, device):
        # one job / block table per library flavour: fp16 jobs go to brats_conv3d_pack_weights_multi_f16 (where the job's
        # dtype code BF16 means "the 16-bit type"), everything else to the plain entry point
        jobs, blocks, entries, off = {False: [], True: []}, {False: [], True: []}, {}, 0
        for key, (wref, (dtype, mode, cin_pad, cin_off, cin_cnt, dil, c1)) in self.recorded.items():
            w = wref()
            if w is None or w.dtype != torch.float32 or not w.is_contiguous():
                continue
            cin_real, k = w.shape[1], w.shape[2]
            cin_w, _, kdim, rows, src = _pack_geometry(w, mode, cin_pad, cin_off, cin_cnt, c1)
            ck = conv_chunk(dtype, k, dil, *src, rows)
            code = _code(dtype)
            nbytes = _lib.lib().brats_conv3d_packed_bytes(code, k, kdim, rows, ck)
            rows16 = (rows + 15) // 16
            x3 = code in (X3_BF16, X3_F16)  # (hi and lo fragments side by side)
            ms_n = nbytes // ((kdim // ck) * rows16 * (2048 if x3 else 1024))
            total = nbytes // (4 if code == F32 else 2)
            entries[key] = [wref, w.data_ptr(), off, nbytes, -1]
            fl = code in (F16, X3_F16)
            jobs[fl].append((w.data_ptr(), off, {F16: BF16, X3_F16: X3_BF16}.get(code, code), mode, k ** 3, cin_w, cin_real, cin_off,
                             rows, rows16, kdim, ck, ms_n, 0, total))
            j = len(jobs[fl]) - 1
            blocks[fl].extend((j, b) for b in range(_lib.lib().brats_conv3d_pack_blocks(kdim, ck, rows)))
            off += (nbytes + 255) // 256 * 256
        self.buf = torch.empty(max(off, 256), dtype=torch.uint8, device=device)
        self.tables = []
        for fl in (False, True):
            if not jobs[fl]:
                continue
            rec = np.array(jobs[fl], dtype=_PACK_JOB)
            rec["out"] += self.buf.data_ptr()
            self.tables.append((fl, torch.from_numpy(rec.view(np.uint8).copy()).to(device),
                                torch.tensor(blocks[fl], dtype=torch.int32, device=device).reshape(-1, 2).contiguous()))
        self.entries = entries
        self.dirty = False

    def run(self, device):
        if not self.recorded:
            return
        if self.entries is not None and not self.dirty:
            for e in self.entries.values():  # a parameter that was re-allocated (.to(), load with assign) moves: rebuild
                w = e[0]()
                if w is None or w.data_ptr() != e[1]:
                    self.dirty = True
                    break
        if self.dirty or self.entries is None:
            self._build(device)
        for fl, jobs, blocks in self.tables:
            fn = _lib.lib().brats_conv3d_pack_weights_multi_f16 if fl else _lib.lib().brats_conv3d_pack_weights_multi
            _lib.check(fn(jobs.data_ptr(), blocks.data_ptr(), blocks.shape[0], _stream()), "conv3d_pack_weights_multi")
        for e in self.entries.values():
            e[4] = e[0]()._version

    def lookup(self, key, w):
        e = self.entries.get(key) if self.entries is not None else None
        if e is not None and e[0]() is w and e[1] == w.data_ptr() and e[4] == w._version:
            return self.buf[e[2]:e[2] + e[3]]
        return None


ACTIVE_PLAN = None  # set by the network programs around a training forward / backward
_PLANS = weakref.WeakKeyDictionary()  # module -> PackPlan (kept off the module: deepcopy / state_dict stay plain)


@contextlib.contextmanager
def use_plan(plan):
    global ACTIVE_PLAN
    old, ACTIVE_PLAN = ACTIVE_PLAN, plan
    try:
        yield
    finally:
        ACTIVE_PLAN = old


def plan_for(module, device):
    """Re-pack every recorded weight of `module` (one launch) and return its plan; call at the start of a training forward."""
    plan = _PLANS.get(module)
    if plan is None:
        plan = _PLANS[module] = PackPlan()
    plan.run(device)
    return plan


def pack_weights(w, dtype, mode, cin_pad=None, cin_off=0, cin_cnt=None, dil=1, c1=None):
    """w: torch-layout [Cout, Cin, k, k, k] f32 parameter -> packed MFMA-fragment buffer.
    mode PACK_FWD: GEMM rows = Cout, K = Cin (zero-padded to cin_pad); PACK_DGRAD: rows = Cin slice,
    K = Cout, taps flipped.

    Under ``torch.no_grad()`` (sliding-window / TTA inference: 144 forwards of the same weights per volume) the
    packed buffer is cached.  A hit needs the same tensor object, address, version counter (bumped by in-place updates:
    torch optimizers, brats21_amd.optim.Ranger2020, load_state_dict, SWA averaging) and cache generation
    (``invalidate_packed_weights``: every training forward and train()/eval() switch of the modules -- that covers
    optimizers that write through ``p.data``, like the reference's Ranger2020)."""
    key = None
    dtype = _conv_dtype(dtype, w.shape[2])
    if ACTIVE_PLAN is not None:
        pkey = (id(w), str(dtype), mode, cin_pad, cin_off, cin_cnt, dil, c1)
        v = ACTIVE_PLAN.lookup(pkey, w)
        if v is not None:
            return v
        ACTIVE_PLAN.record(pkey, w, (dtype, mode, cin_pad, cin_off, cin_cnt, dil, c1))
    if not torch.is_grad_enabled():
        # keyed by the tensor OBJECT (weak reference: a new tensor that reuses a freed address must not hit) and its
        # version counter
        key = (id(w), str(dtype), mode, cin_pad, cin_off, cin_cnt, dil, c1)
        hit = _cache_get(key, w)
        if hit is not None:
            return hit
    packed = _pack_weights(w, dtype, mode, cin_pad, cin_off, cin_cnt, dil, c1)
    if key is not None:
        _cache_put(key, w, packed)
    return packed


def _pack_weights(w, dtype, mode, cin_pad, cin_off, cin_cnt, dil, c1):
    cout_w, k = w.shape[0], w.shape[2]
    cin_w, cin_cnt, kdim, rows, src = _pack_geometry(w, mode, cin_pad, cin_off, cin_cnt, c1)
    w = _padded(w, cin_w)
    code = _code(dtype)
    ck = conv_chunk(dtype, k, dil, *src, rows)
    nbytes = _lib.lib().brats_conv3d_packed_bytes(code, k, kdim, rows, ck)
    packed = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    _lib.check(_lib.lib().brats_conv3d_pack_weights(w.data_ptr(), packed.data_ptr(), code, mode, k, cout_w, cin_w,
                                                    cin_off, cin_cnt, ck, _stream()), "conv3d_pack_weights")
    return packed


def set_kp(mode):
    """brats_conv3d_set_kp: 1 / 0 = the 8-wave K-parity form of the small-grid 3x3x3 launches on / off, -1 = default.  The packed
    weights do not depend on it.  Returns the previous setting."""
    return _lib.lib().brats_conv3d_set_kp(mode)


def set_vs8(mode):
    """brats_conv3d_set_vs8 + invalidation of everything packed under the old setting (the switch changes the K chunk, i.e.
    the packed-weight layout of the layers it applies to).  Returns the previous setting."""
    old = _lib.lib().brats_conv3d_set_vs8(mode)
    invalidate_packed_weights()
    for plan in list(_PLANS.values()):
        plan.dirty = True
        plan.entries = None
    return old


def set_x3_wgrad_fused(mode):
    """brats_conv3d_set_x3_wgrad_fused: 1 = the fused split-precision weight gradient where it is built and pays, 2 = for any tile
    count (tests), 0 = the split pass + three 16-bit launches everywhere, -1 = default.  Returns the previous setting."""
    return _lib.lib().brats_conv3d_set_x3_wgrad_fused(mode)


def split_granule(cout):
    return _lib.lib().brats_conv3d_split_granule(cout)


def tiles_per_sample(d, h, w):
    return _lib.lib().brats_conv3d_tiles_per_sample(d, h, w)


class Pending:
    """z = act(y * scale + shift) that has NOT been stored: the raw convolution output `y` of a ConvBnRelu unit plus what
    its consumer needs to apply the normalisation + activation on load (conv3d(pre=...), include/brats_hip.h:
    brats_conv3d_fwd_pre), or to materialise it after all (``materialize()`` = the affine_act pass)."""

    def __init__(self, y, scale_shift, act, slope=0.01):
        self.y, self.scale_shift, self.act, self.slope = y, scale_shift, act, slope
        self.shape, self.dtype, self.device = y.shape, y.dtype, y.device

    def materialize(self):
        return affine_act(self.y, self.scale_shift, self.act, slope=self.slope)


def conv_pre_ok(dtype, ksize, dil, c1, c2, cout):
    """Is the normalise-on-load form of the convolution built for this layer?  (16-bit, 3x3x3, dilation 1, Cout % 48 == 0)"""
    return is16(dtype) and bool(_lib.lib().brats_conv3d_pre_ok(_code(dtype), ksize, dil, c1, c2, cout))


def _conv_outputs(x, cout, out, split, want_stats, what):
    """What a convolution of x writes: -> (y, stats | None, args).  y = `out` (checked), a fresh [N, D, H, W, cout] tensor, or --
    split -- the pair of dense tensors with the output channels [0, split) and [split, cout); stats = [N, tiles, cout, 2];
    args = (y, pitch, y2, c2, split, stats) as the entry points take them."""
    n, d, h, w, _ = x.shape
    y2 = None
    if split is not None:
        out = new_act(n, d, h, w, split, x.dtype, x.device)
        y2 = new_act(n, d, h, w, cout - split, x.dtype, x.device)
    elif out is None:
        out = new_act(n, d, h, w, cout, x.dtype, x.device)
    optr, oc, op = _desc(out)
    if (y2 is None and oc != cout) or out.dtype != x.dtype:
        raise _lib.BratsHipError(f"{what}: bad output tensor")
    stats = torch.empty((n, tiles_per_sample(d, h, w), cout, 2), dtype=torch.float32, device=x.device) if want_stats else None
    args = (optr, op, y2.data_ptr() if y2 is not None else None, (cout - split) if y2 is not None else 0, split or 0,
            stats.data_ptr() if stats is not None else None)
    return ((out, y2) if y2 is not None else out), stats, args


def conv3d(x, packed_w, cout, ksize=3, dil=1, bias=None, out=None, want_stats=False, x2=None, split=None, amax=None):
    if isinstance(x, Pending) or isinstance(x2, Pending):
        return _conv3d_pre(x, packed_w, cout, ksize, dil, bias, out, want_stats, x2)
    return _conv3d(x, packed_w, cout, ksize, dil, bias, out, want_stats, x2, split, amax)


def _conv3d_pre(x, packed_w, cout, ksize, dil, bias, out, want_stats, x2):
    """conv3d whose input(s) are Pending activations: normalise + act applied while the halo tile is staged."""
    p1 = x if isinstance(x, Pending) else None
    p2 = x2 if isinstance(x2, Pending) else None
    xa = p1.y if p1 is not None else x
    xb = p2.y if p2 is not None else x2
    if p1 is not None and p2 is not None and (p1.act != p2.act or p1.slope != p2.slope):
        raise _lib.BratsHipError("conv3d: the two pending inputs carry different activations")
    act, slope = (p1 or p2).act, (p1 or p2).slope
    ptr, c, p = _desc(xa)
    n, d, h, w, _ = xa.shape
    ptr2, c2, pp2 = _desc2(xb)
    out, stats, (optr, op, _, _, _, sptr) = _conv_outputs(xa, cout, out, None, want_stats, "conv3d")
    with _span("conv_igemm", c + c2, cout, ksize, dil, n, d, h, w, str(xa.dtype)):
        _lib.check(_lib.lib().brats_conv3d_fwd_pre(ptr, c, p, p1.scale_shift.data_ptr() if p1 is not None else None, ptr2, c2, pp2,
                                                   p2.scale_shift.data_ptr() if p2 is not None else None, ACTS[act], float(slope),
                                                   packed_w.data_ptr(), _f32(bias), optr, op, sptr, _code(xa.dtype), dil, n, d, h, w,
                                                   cout, _stream()), "conv3d_fwd_pre")
    return out, stats


def _conv3d(x, packed_w, cout, ksize=3, dil=1, bias=None, out=None, want_stats=False, x2=None, split=None, amax=None):
    """y[N,D,H,W,cout] = conv([x | x2]) with weights from pack_weights().  Returns (y, stats|None) where
    stats = [N, tiles, cout, 2] per-tile per-channel (sum, sum of squares) of the f32 result.
    x2: optional second input (virtual concat, no torch.cat).  split: write output channels
    [0, split) and [split, cout) to two dense tensors (returns (y, y2) as y).
    amax (split precision only): 1-element f32 device tensor holding max|x| -- the input is scaled into fp16's range by the
    matching power of two and the result scaled back (brats_conv3d_x3_fwd: the input gradient, whose x = dY is tiny)."""
    ptr, c, p = _desc(x)
    n, d, h, w, _ = x.shape
    ptr2, c2, p2 = _desc2(x2)
    y, stats, oargs = _conv_outputs(x, cout, out, split, want_stats, "conv3d")
    kd = _conv_dtype(x.dtype, ksize)  # (split precision: f32 tensors, weights packed under the same mode)
    with _span("conv_igemm", c + c2, cout, ksize, dil, n, d, h, w, str(kd)):
        if amax is not None and kd in (X3F, X3B):
            _lib.check(_lib.lib().brats_conv3d_x3_fwd(ptr, c, p, ptr2, c2, p2, _f32(amax), packed_w.data_ptr(), _f32(bias), *oargs,
                                                      _code(kd), dil, n, d, h, w, cout, _stream()), "conv3d_x3_fwd")
        else:
            _lib.check(_lib.lib().brats_conv3d_fwd(ptr, c, p, ptr2, c2, p2, packed_w.data_ptr(), _f32(bias), *oargs, _code(kd),
                                                   ksize, dil, n, d, h, w, cout, _stream()), "conv3d_fwd")
    return y, stats


# ------------------------------------------------------------------------------------------ narrow-output conv
def pack_weights_narrow(w, mode):
    """w: torch-layout [Cout, Cin, 3, 3, 3] f32 -> the f32 buffer conv3d_narrow() reads.  PACK_FWD: Cout <= 16 class rows over Cin
    channels; PACK_DGRAD: Cin <= 16 class rows over Cout channels, transposed with the taps flipped (the input gradient as a
    convolution of dy).  The channel count must be a multiple of 8.  Cached under no_grad like pack_weights()."""
    if w.dim() != 5 or tuple(w.shape[2:]) != (3, 3, 3):
        raise _lib.BratsHipError(f"pack_weights_narrow: expected [Cout, Cin, 3, 3, 3], got {tuple(w.shape)}")
    cout_w, cin_w = w.shape[0], w.shape[1]
    c, k = (cin_w, cout_w) if mode == PACK_FWD else (cout_w, cin_w)
    key = None
    if not torch.is_grad_enabled():
        key = (id(w), "narrow", mode)
        hit = _cache_get(key, w)
        if hit is not None:
            return hit
    nbytes = _lib.lib().brats_conv3d_narrow_packed_bytes(c, k)
    if nbytes == 0:
        raise _lib.BratsHipError(f"pack_weights_narrow: {c} channels -> {k} rows is outside the kernel (channels % 8 == 0, rows <= 16)")
    wf = w.detach().contiguous().float()
    packed = torch.empty(nbytes // 4, dtype=torch.float32, device=w.device)
    _lib.check(_lib.lib().brats_conv3d_narrow_pack(wf.data_ptr(), packed.data_ptr(), mode, cout_w, cin_w, _stream()),
               "conv3d_narrow_pack")
    if key is not None:
        _cache_put(key, w, packed)
    return packed


def conv3d_narrow(x, packed_w, k, bias=None, add=None):
    """NCDHW f32 [N, k, D, H, W] = add + bias + conv3x3x3(x) (zero padding, dilation 1) of an NDHWC tensor or channel slice x
    (bf16, fp16 or f32; C a multiple of 8) with weights from pack_weights_narrow(); k <= 16.  bias [k] and add [N, k, D, H, W]
    (f32, never rounded) are optional.  One pass: x is read once per output tile, the result leaves as f32 planes."""
    ptr, c, p = _desc(x)
    n, d, h, w, _ = x.shape
    if packed_w.numel() * 4 != _lib.lib().brats_conv3d_narrow_packed_bytes(c, k):
        raise _lib.BratsHipError(f"conv3d_narrow: the packed weights do not belong to a {c} -> {k} layer")
    if add is not None and tuple(add.shape) != (n, k, d, h, w):
        raise _lib.BratsHipError(f"conv3d_narrow: add has shape {tuple(add.shape)}, expected {(n, k, d, h, w)}")
    if bias is not None and bias.numel() != k:
        raise _lib.BratsHipError(f"conv3d_narrow: bias has {bias.numel()} elements, expected {k}")
    out = torch.empty((n, k, d, h, w), dtype=torch.float32, device=x.device)
    with _span("conv_narrow", c, k, n, d, h, w, str(x.dtype)):
        _lib.check(_lib.lib().brats_conv3d_narrow_fwd(ptr, c, p, packed_w.data_ptr(), _f32(bias), _f32(add), out.data_ptr(),
                                                      _code(x.dtype), k, n, d, h, w, _stream()), "conv3d_narrow_fwd")
    return out


# ------------------------------------------------------------------------------------------ fp8 conv
def absmax(x):
    """max|x| of an NDHWC tensor as a 1-element f32 device tensor (no host sync)."""
    ptr, c, p = _desc(x)
    out = torch.empty(1, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().brats_absmax(ptr, p, _code(x.dtype), x.shape[0] * x.shape[1] * x.shape[2] * x.shape[3], c,
                                       out.data_ptr(), _stream()), "absmax")
    return out


F8_MIN_SIZE = 0  # e4m3 forward convolutions only at levels whose depth is >= this many voxels (0 = every level); set_f8_min_size()


def set_f8_min_size(n):
    """Restrict model.conv_fp8's FORWARD convolutions to the levels with a depth of at least n voxels (64: the 128^3 and 64^3
    levels of a 128^3 patch; 0 = all levels, the default).  An experiment knob for VERDICT r5 item 7 (does e4m3 hold the Dice bar
    when only the large, statistics-rich levels use it?); the backward kernels do not look at it.  Returns the previous value."""
    global F8_MIN_SIZE
    old, F8_MIN_SIZE = F8_MIN_SIZE, int(n)
    return old


def conv_f8_chunk(c1, c2=0):
    """Channel chunk of the fp8 kernel for an input of c1 (+c2) channels; 0 = not supported (use conv3d)."""
    return _lib.lib().brats_conv3d_f8_chunk(c1, c2)


def pack_weights_f8(w, mode, cin_pad=None, cin_off=0, cin_cnt=None, c1=None):
    """e4m3 fragments + per-row power-of-two scales for conv3d_f8 (3x3x3 only); arguments as pack_weights()."""
    key = None
    if not torch.is_grad_enabled():
        key = (id(w), "f8", mode, cin_pad, cin_off, cin_cnt, 0, c1)
        hit = _cache_get(key, w)
        if hit is not None:
            return hit
    w0, cout_w = w, w.shape[0]
    if w.shape[2] != 3:
        raise _lib.BratsHipError("pack_weights_f8: 3x3x3 kernels only")
    cin_w, cin_cnt, kdim, rows, src = _pack_geometry(w, mode, cin_pad, cin_off, cin_cnt, c1)
    w = _padded(w, cin_w)
    ck = conv_f8_chunk(*src)
    if ck <= 0:
        raise _lib.BratsHipError(f"pack_weights_f8: K channels {kdim} (c1={c1}) are not multiples of 16")
    nbytes = _lib.lib().brats_conv3d_f8_packed_bytes(kdim, rows, ck)
    packed = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    _lib.check(_lib.lib().brats_conv3d_f8_pack_weights(w.data_ptr(), packed.data_ptr(), mode, cout_w, cin_w, cin_off,
                                                       cin_cnt, ck, _stream()), "conv3d_f8_pack_weights")
    if key is not None:
        _cache_put(key, w0, packed)
    return packed


def conv3d_f8(x, packed_w, cout, dil=1, bias=None, out=None, want_stats=False, x2=None, split=None, amax=None, amax2=None,
              xscale=None):
    """conv3d() with the e4m3 MFMA kernel (bf16 tensors in and out).  amax / amax2: 1-element f32 tensors holding
    max|x| / max|x2| (from affine_act / gn_act_bwd / absmax); when missing they are computed here (one extra pass)
    unless a static power-of-two ``xscale`` is given."""
    if not is16(x.dtype):
        raise _lib.BratsHipError("conv3d_f8: bf16 activations only")
    ptr, c, p = _desc(x)
    n, d, h, w, _ = x.shape
    ptr2, c2, p2 = _desc2(x2)
    if xscale is None:
        if amax is None:
            amax = absmax(x)
        if x2 is not None and amax2 is None:
            amax2 = absmax(x2)
    else:
        amax = amax2 = None
    y, stats, oargs = _conv_outputs(x, cout, out, split, want_stats, "conv3d_f8")
    with _span("conv_igemm_f8", c + c2, cout, 3, dil, n, d, h, w, "e4m3"):
        _lib.check(_fn16("brats_conv3d_f8_fwd", x.dtype)(ptr, c, p, _f32(amax), ptr2, c2, p2, _f32(amax2),
                                                  float(xscale) if xscale is not None else 0.0, packed_w.data_ptr(),
                                                  _f32(bias), *oargs, dil, n, d, h, w, cout, _stream()), "conv3d_f8_fwd")
    return y, stats


def _grad_out(out, shape, device):
    """The f32 tensor a gradient kernel writes: `out` (e.g. the parameter's slice of a DDP bucket, ddp.GradientBuckets.dest)
    when it is given and fits, otherwise a fresh allocation."""
    if out is not None and out.numel() == int(np.prod(shape)) and out.dtype == torch.float32 and out.is_contiguous():
        return out.view(shape)
    return torch.empty(shape, dtype=torch.float32, device=device)


def conv3d_wgrad(x, dy, ksize=3, dil=1, want_dbias=False, x2=None, out=None, amax_dy=None):
    """dW [cout, cin (+cin2), k,k,k] f32 (and dbias) from the layer input [x | x2] and the output gradient dy.
    amax_dy (split precision only): 1-element f32 device tensor holding max|dy| (see conv3d's amax)."""
    ptr, c, p = _desc(x)
    ptr2, c2, p2 = _desc2(x2)
    dptr, cout, dp = _desc(dy)
    n, d, h, w, _ = x.shape
    kd = _conv_dtype(x.dtype, ksize)
    if kd in (X3F, X3B) and (c % 8 or c2 % 8 or cout % 8):
        kd = x.dtype  # (narrow test widths: the 16-bit kernels behind the split form want multiples of 8 channels)
    code = _code(kd)
    nbytes = _lib.lib().brats_conv3d_wgrad_ws_bytes(code, ksize, n, d, h, w, c, c2, cout)
    ws = torch.empty(max(nbytes, 4) // 4, dtype=torch.float32, device=x.device)
    dw = _grad_out(out, (cout, c + c2, ksize, ksize, ksize), x.device)
    db = torch.empty(cout, dtype=torch.float32, device=x.device) if want_dbias else None
    if amax_dy is not None and kd in (X3F, X3B):
        with _span("conv_wgrad", c + c2, cout, ksize, dil, n, d, h, w, str(kd)):
            _lib.check(_lib.lib().brats_conv3d_x3_wgrad(ptr, c, p, ptr2, c2, p2, dptr, dp, _f32(amax_dy), ws.data_ptr(), dw.data_ptr(),
                                                        db.data_ptr() if db is not None else None, code, dil, n, d, h, w, cout,
                                                        _stream()), "conv3d_x3_wgrad")
        return dw, db
    with _span("conv_wgrad", c + c2, cout, ksize, dil, n, d, h, w, str(kd)):
        _lib.check(_lib.lib().brats_conv3d_wgrad(ptr, c, p, ptr2, c2, p2, dptr, dp, ws.data_ptr(), dw.data_ptr(),
                                                 db.data_ptr() if db is not None else None, code, ksize, dil, n, d, h, w,
                                                 cout, _stream()), "conv3d_wgrad")
    return dw, db


def conv3d_wgrad_f8_ok(x, dy, x2=None):
    """Is the e4m3 weight-gradient kernel built for this layer (3x3x3, dilation 1, 48 x 48 / 64 x 32 channel blocks)?"""
    n, d, h, w, c = x.shape
    return (is16(x.dtype) and dy.dtype == x.dtype and
            _lib.lib().brats_conv3d_wgrad_f8_ws_bytes(n, d, h, w, c, x2.shape[-1] if x2 is not None else 0, dy.shape[-1]) > 0)


def conv3d_wgrad_f8(x, dy, amax, amax_dy, x2=None, amax2=None, out=None):
    """dW [cout, cin (+cin2), 3, 3, 3] f32 of a dilation-1 layer with X and dY rounded to e4m3 on the way into the MFMA
    (v_mfma_scale_f32_16x16x128_f8f6f4).  amax* : 1-element f32 device tensors holding max|x|, max|x2|, max|dy| (recorded
    by the kernels that produced the tensors; absmax() otherwise).  Only where conv3d_wgrad_f8_ok()."""
    ptr, c, p = _desc(x)
    ptr2, c2, p2 = _desc2(x2)
    dptr, cout, dp = _desc(dy)
    n, d, h, w, _ = x.shape
    if not is16(x.dtype) or dy.dtype != x.dtype:
        raise _lib.BratsHipError("conv3d_wgrad_f8: bf16 activations only")
    nbytes = _lib.lib().brats_conv3d_wgrad_f8_ws_bytes(n, d, h, w, c, c2, cout)
    if nbytes == 0:
        raise _lib.BratsHipError(f"conv3d_wgrad_f8: not built for {c}+{c2} -> {cout} channels at {n}x{d}x{h}x{w} (use conv3d_wgrad)")
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    dw = _grad_out(out, (cout, c + c2, 3, 3, 3), x.device)
    with _span("conv_wgrad_f8", c + c2, cout, 3, 1, n, d, h, w, "e4m3"):
        _lib.check(_fn16("brats_conv3d_wgrad_f8", x.dtype)(ptr, c, p, _f32(amax), ptr2, c2, p2, _f32(amax2), dptr, dp, _f32(amax_dy),
                                                    ws.data_ptr(), dw.data_ptr(), n, d, h, w, cout, _stream()), "conv3d_wgrad_f8")
    return dw


# ------------------------------------------------------------------------------------------ GroupNorm + act
def gn_finalize(stats, n, c, groups, voxels, gamma, beta, eps=1e-5):
    mean_rstd = torch.empty((n, groups, 2), dtype=torch.float32, device=stats.device)
    scale_shift = torch.empty((n, c, 2), dtype=torch.float32, device=stats.device)
    chan = torch.empty(_lib.lib().brats_gn_ws_doubles(n, c), dtype=torch.float64, device=stats.device)
    _lib.check(_lib.lib().brats_gn_finalize(stats.data_ptr(), stats.shape[1], n, c, groups, float(voxels), eps,
                                            _f32(gamma), _f32(beta), mean_rstd.data_ptr(), scale_shift.data_ptr(),
                                            chan.data_ptr(), _stream()), "gn_finalize")
    return mean_rstd, scale_shift


def affine_act(y, scale_shift, act="relu", out=None, slope=0.01, amax=None, slope_t=None):
    """amax: optional zero-initialised 1-element f32 tensor that receives max|out| (scale source of conv3d_f8).
    slope_t: 1-element f32 device tensor overriding ``slope`` (nn.PReLU's learnable weight, act = "leakyrelu")."""
    ptr, c, p = _desc(y)
    n, d, h, w, _ = y.shape
    if out is None:
        out = new_act(n, d, h, w, c, y.dtype, y.device)
    optr, oc, op = _desc(out)
    _lib.check(_lib.lib().brats_affine_act_fwd(ptr, p, scale_shift.data_ptr(), optr, op, _code(y.dtype), ACTS[act], slope,
                                               _f32(slope_t), n, d * h * w, c, _f32(amax), _stream()), "affine_act_fwd")
    return out


def affine_act_add(y, scale_shift, add, act="relu", out=None, slope=0.01, slope_t=None):
    """out = add + act(y * scale + shift) in one pass (include/brats_hip.h: brats_affine_act_add_fwd): bit-identical to
    affine_act(y, ...) followed by an elementwise add of the two stored tensors.  add / out may be channel-slice views; out must
    not overlap y or add."""
    ptr, c, p = _desc(y)
    aptr, ac, ap = _desc(add)
    n, d, h, w, _ = y.shape
    if add.shape != y.shape or add.dtype != y.dtype:
        raise _lib.BratsHipError("affine_act_add: add must have y's shape and dtype")
    if out is None:
        out = new_act(n, d, h, w, c, y.dtype, y.device)
    optr, oc, op = _desc(out)
    if out.shape != y.shape or out.dtype != y.dtype:
        raise _lib.BratsHipError("affine_act_add: bad output tensor")
    _lib.check(_lib.lib().brats_affine_act_add_fwd(ptr, p, scale_shift.data_ptr(), aptr, ap, optr, op, _code(y.dtype), ACTS[act], slope,
                                                   _f32(slope_t), n, d * h * w, c, _stream()), "affine_act_add_fwd")
    return out


def grad_sum(*srcs, out=None):
    """out = srcs[0] + srcs[1] (+ srcs[2] (+ srcs[3])) on NDHWC tensors (or channel-slice views) of one shape and storage type:
    f32 accumulation in argument order, one rounding, one launch (include/brats_hip.h: brats_grad_sum) -- the gradient of a
    tensor with several readers.  More than four sources: further launches that take the running sum as their first source.
    Small f32 tensors (weight gradients) go through a [1, 1, 1, rows, C] view.  out must not overlap a source."""
    if len(srcs) < 2:
        raise _lib.BratsHipError("grad_sum: at least two sources")
    first = srcs[0]
    if any(s.shape != first.shape or s.dtype != first.dtype for s in srcs[1:]):
        raise _lib.BratsHipError("grad_sum: the sources must have one shape and dtype")
    if len(srcs) > 4:
        return grad_sum(grad_sum(*srcs[:4]), *srcs[4:], out=out)
    n, d, h, w, c = first.shape
    if out is None:
        out = new_act(n, d, h, w, c, first.dtype, first.device)
    optr, oc, op = _desc(out)
    if out.shape != first.shape or out.dtype != first.dtype:
        raise _lib.BratsHipError("grad_sum: bad output tensor")
    args = []
    for s in srcs:
        ptr, _, p = _desc(s)
        args += [ptr, p]
    args += [None, 0] * (4 - len(srcs))
    _lib.check(_lib.lib().brats_grad_sum(*args, len(srcs), optr, op, _code(first.dtype), n, d * h * w, c, _stream()), "grad_sum")
    return out


def dropout(x, p, state, unit, out=None):
    """nn.Dropout(p) on an NDHWC activation (or, with the same arguments, on the gradient flowing back through it): x * keep /
    (1 - p) with keep a pure function of (state[0] = seed, state[1] = step counter, unit id, element index) -- brats_dropout.
    state: int64[2] DEVICE tensor.  out=x: in place."""
    ptr, c, pitch = _desc(x)
    n, d, h, w, _ = x.shape
    if state.dtype != torch.int64 or state.numel() != 2 or not state.is_cuda:
        raise _lib.BratsHipError("dropout: state must be an int64[2] device tensor (seed, step counter)")
    if out is None:
        out = new_act(n, d, h, w, c, x.dtype, x.device)
    optr, oc, op = _desc(out)
    if oc != c or out.dtype != x.dtype:
        raise _lib.BratsHipError("dropout: bad output tensor")
    _lib.check(_lib.lib().brats_dropout(ptr, pitch, optr, op, _code(x.dtype), n * d * h * w, c, float(p), state.data_ptr(), int(unit),
                                        _stream()), "dropout")
    return out


def affine_act_pool(y, scale_shift, act="relu", slope=0.01, amax=None, slope_t=None, with_avg=False, want_argmax=False):
    """(z, pooled) = (affine_act(y), maxpool2(z)) in one pass (include/brats_hip.h: brats_affine_act_pool_fwd).
    want_argmax: z._pool_argmax = the uint8 window index of every pooled element, which maxpool2_bwd(z, ...) then reads
    instead of the window itself."""
    ptr, c, p = _desc(y)
    n, d, h, w, _ = y.shape
    z = new_act(n, d, h, w, c, y.dtype, y.device)
    pooled = new_act(n, d // 2, h // 2, w // 2, c * (2 if with_avg else 1), y.dtype, y.device)
    idx = torch.empty((n, d // 2, h // 2, w // 2, c), dtype=torch.uint8, device=y.device) if want_argmax else None
    zp, _, zpitch = _desc(z)
    pp, _, ppitch = _desc(pooled)
    _lib.check(_lib.lib().brats_affine_act_pool_fwd(ptr, p, scale_shift.data_ptr(), zp, zpitch, pp, ppitch,
                                                    idx.data_ptr() if idx is not None else None, _code(y.dtype), ACTS[act],
                                                    slope, _f32(slope_t), n, d, h, w, c, int(with_avg), _f32(amax), _stream()),
               "affine_act_pool_fwd")
    if idx is not None:
        z._pool_argmax = idx
    return z, pooled


def _gn_bwd_bufs(y, dy=None):
    """(dy like y, reduction workspace, dgamma [C], dbeta [C]) of the GroupNorm + activation backward entry points."""
    n, c = y.shape[0], y.shape[-1]
    red = torch.empty(_lib.lib().brats_gn_bwd_ws_floats(n, c), dtype=torch.float32, device=y.device)
    dgamma = torch.empty(c, dtype=torch.float32, device=y.device)
    dbeta = torch.empty(c, dtype=torch.float32, device=y.device)
    return (torch.empty(y.shape, dtype=y.dtype, device=y.device) if dy is None else dy), red, dgamma, dbeta


def gn_act_bwd(dz, y, scale_shift, mean_rstd, gamma, groups=8, act="relu", slope=0.01, amax=None, slope_t=None, out=None):
    """Returns (dy, dgamma, dbeta) for z = act(GroupNorm(y)); amax (optional, zero-initialised) receives max|dy|.
    out: the tensor dy is written to (e.g. a slice of a stacked buffer) instead of a fresh one."""
    dzp, c, dzpitch = _desc(dz)
    yp, _, ypitch = _desc(y)
    n, d, h, w, _ = y.shape
    dy, red, dgamma, dbeta = _gn_bwd_bufs(y, out)
    dyp, dyc, dypitch = _desc(dy)
    if dy.shape != y.shape or dy.dtype != y.dtype:
        raise _lib.BratsHipError("gn_act_bwd: bad output tensor")
    _lib.check(_lib.lib().brats_gn_act_bwd(dzp, dzpitch, yp, ypitch, scale_shift.data_ptr(), mean_rstd.data_ptr(),
                                           _f32(gamma), dyp, dypitch, red.data_ptr(), dgamma.data_ptr(),
                                           dbeta.data_ptr(), _code(y.dtype), ACTS[act], slope, _f32(slope_t), n, d * h * w, c,
                                           groups, _f32(amax), _stream()), "gn_act_bwd")
    return dy, dgamma, dbeta


def conv_bstats_ok(dtype, dil, c1, cout, act="relu", slope_t=None):
    """Is the "backward statistics" form of the 3x3x3 convolution (conv3d_bstats) built for this layer?"""
    dtype = _conv_dtype(dtype, 3)  # (f32 tensors inside a split_precision() block: the x3 kernels have the form too)
    if not (is16(dtype) or dtype in (X3F, X3B)) or slope_t is not None or act not in ("relu", "leakyrelu"):
        return False
    return bool(_lib.lib().brats_conv3d_bstats_ok(_code(dtype), 3, dil, c1, cout))


def conv3d_bstats(x, packed_w, cout, dil, fwd_y, scale_shift, act="relu", slope=0.01, amax=None):
    """The input gradient dz = conv(x = dy of a block's second unit, weights packed with PACK_DGRAD) that also leaves
    GroupNorm backward's first pass for the block's FIRST unit (include/brats_hip.h: brats_conv3d_fwd_bstats): per tile and
    channel sum u and sum u * fwd_y, u = dz * act'(fwd_y * scale + shift).  -> (dz, tile_stats) for gn_act_bwd_tiles().
    f32 tensors inside a split_precision() block run brats_conv3d_x3_fwd_bstats; amax = max|x| as for conv3d (fp16 pairs)."""
    ptr, c, p = _desc(x)
    n, d, h, w, _ = x.shape
    fp, fc, fpitch = _desc(fwd_y)
    if fc != cout or fwd_y.dtype != x.dtype or tuple(fwd_y.shape[:4]) != (n, d, h, w):
        raise _lib.BratsHipError("conv3d_bstats: the forward tensor must have the output's shape and dtype")
    out = new_act(n, d, h, w, cout, x.dtype, x.device)
    stats = torch.empty((n, tiles_per_sample(d, h, w), cout, 2), dtype=torch.float32, device=x.device)
    # (a family of its own in the bench's kernel table: these launches carry a GroupNorm-backward pass in their epilogue and
    #  are not the plain implicit GEMM the roofline line is about)
    kd = _conv_dtype(x.dtype, 3)
    if kd in (X3F, X3B):
        with _span("conv_igemm_bst", c, cout, 3, dil, n, d, h, w, str(kd)):
            _lib.check(_lib.lib().brats_conv3d_x3_fwd_bstats(ptr, c, p, _f32(amax), packed_w.data_ptr(), out.data_ptr(), cout, fp, fpitch,
                                                             scale_shift.data_ptr(), ACTS[act], float(slope), stats.data_ptr(),
                                                             _code(kd), dil, n, d, h, w, cout, _stream()), "conv3d_x3_fwd_bstats")
        return out, stats
    with _span("conv_igemm_bst", c, cout, 3, dil, n, d, h, w, str(x.dtype)):
        _lib.check(_lib.lib().brats_conv3d_fwd_bstats(ptr, c, p, packed_w.data_ptr(), out.data_ptr(), cout, fp, fpitch,
                                                      scale_shift.data_ptr(), ACTS[act], float(slope), stats.data_ptr(),
                                                      _code(x.dtype), dil, n, d, h, w, cout, _stream()), "conv3d_fwd_bstats")
    return out, stats


def gn_act_bwd_tiles(tile_stats, dz, y, scale_shift, mean_rstd, gamma, groups=8, act="relu", slope=0.01, amax=None):
    """gn_act_bwd whose first pass was taken by conv3d_bstats (tile_stats): -> (dy, dgamma, dbeta)."""
    dzp, c, dzpitch = _desc(dz)
    yp, _, ypitch = _desc(y)
    n, d, h, w, _ = y.shape
    dy, red, dgamma, dbeta = _gn_bwd_bufs(y)
    _lib.check(_lib.lib().brats_gn_act_bwd_tiles(tile_stats.data_ptr(), tile_stats.shape[1], dzp, dzpitch, yp, ypitch,
                                                 scale_shift.data_ptr(), mean_rstd.data_ptr(), _f32(gamma), dy.data_ptr(), c,
                                                 red.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), _code(y.dtype), ACTS[act],
                                                 float(slope), n, d * h * w, c, groups, _f32(amax), _stream()), "gn_act_bwd_tiles")
    return dy, dgamma, dbeta


def gn_act_bwd_head(dlogits, head_weight, y, scale_shift, mean_rstd, gamma, groups=8, act="relu", slope=0.01, amax=None):
    """GroupNorm + activation backward of the layer under the 1x1x1 output head, the head's backward folded in
    (include/brats_hip.h: brats_gn_act_bwd_head): -> (dy, dgamma, dbeta, dhead_weight [K,C,1,1,1], dhead_bias [K])."""
    yp, c, ypitch = _desc(y)
    n, d, h, w, _ = y.shape
    k = head_weight.shape[0]
    dev = y.device
    hw = head_weight.detach().reshape(k, c).contiguous().float()
    dl = dlogits.contiguous().float()
    dy, red, dgamma, dbeta = _gn_bwd_bufs(y)
    hws = torch.empty(_lib.lib().brats_gn_bwd_head_ws_floats(n, c, k), dtype=torch.float32, device=dev)
    dhw = torch.empty((k, c), dtype=torch.float32, device=dev)
    dhb = torch.empty(k, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().brats_gn_act_bwd_head(dl.data_ptr(), hw.data_ptr(), k, yp, ypitch, scale_shift.data_ptr(),
                                                mean_rstd.data_ptr(), _f32(gamma), dy.data_ptr(), c, red.data_ptr(), hws.data_ptr(),
                                                dgamma.data_ptr(), dbeta.data_ptr(), dhw.data_ptr(), dhb.data_ptr(), _code(y.dtype),
                                                ACTS[act], slope, n, d * h * w, c, groups, _f32(amax), _stream()), "gn_act_bwd_head")
    return dy, dgamma, dbeta, dhw.reshape(k, c, 1, 1, 1), dhb


def gn_act_bwd_pool(dskip, dpool, argmax, y, scale_shift, mean_rstd, gamma, groups=8, act="relu", slope=0.01, amax=None):
    """GroupNorm + activation backward of the layer that ends an encoder level, its output gradient dskip +
    maxpool-backward(dpool) composed inside the two passes (include/brats_hip.h: brats_gn_act_bwd_pool): -> (dy, dgamma, dbeta)."""
    yp, c, ypitch = _desc(y)
    n, d, h, w, _ = y.shape
    sp, _, spitch = _desc(dskip)
    pp, _, ppitch = _desc(dpool)
    dy, red, dgamma, dbeta = _gn_bwd_bufs(y)
    _lib.check(_lib.lib().brats_gn_act_bwd_pool(sp, spitch, pp, ppitch, argmax.data_ptr(), yp, ypitch, scale_shift.data_ptr(),
                                                mean_rstd.data_ptr(), _f32(gamma), dy.data_ptr(), c, red.data_ptr(),
                                                dgamma.data_ptr(), dbeta.data_ptr(), _code(y.dtype), ACTS[act], slope, n, d, h, w, c,
                                                groups, _f32(amax), _stream()), "gn_act_bwd_pool")
    return dy, dgamma, dbeta


def head_fold_ok(head_weight, act, slope_t):
    """brats_gn_act_bwd_head is built for three logit planes and relu / leakyrelu without a learnable slope."""
    return head_weight.shape[0] == 3 and act in ("relu", "leakyrelu") and slope_t is None


def prelu_slope_grad(dz, y, scale_shift):
    """d loss / d slope [1] of z = PReLU(y * scale + shift) with one shared slope (nn.PReLU()): sum dz * min(pre, 0)."""
    dzp, c, dzpitch = _desc(dz)
    yp, _, ypitch = _desc(y)
    n, d, h, w, _ = y.shape
    ws = torch.empty(_lib.lib().brats_prelu_ws_floats(n), dtype=torch.float32, device=y.device)
    out = torch.empty(1, dtype=torch.float32, device=y.device)
    _lib.check(_lib.lib().brats_prelu_slope_grad(dzp, dzpitch, yp, ypitch, scale_shift.data_ptr(), ws.data_ptr(), out.data_ptr(),
                                                 _code(y.dtype), n, d * h * w, c, _stream()), "prelu_slope_grad")
    return out


# ------------------------------------------------------------------------------------------ pool / upsample
def maxpool2(x, with_avg=False, out=None, want_argmax=False):
    """want_argmax (training): x._pool_argmax = the uint8 window index of every pooled element; maxpool2_bwd(x, ...) then
    reads those bytes instead of the eight window voxels of x."""
    ptr, c, p = _desc(x)
    n, d, h, w, _ = x.shape
    co = 2 * c if with_avg else c
    if out is None:
        out = new_act(n, d // 2, h // 2, w // 2, co, x.dtype, x.device)
    optr, oc, op = _desc(out)
    idx = torch.empty((n, d // 2, h // 2, w // 2, c), dtype=torch.uint8, device=x.device) if want_argmax else None
    _lib.check(_lib.lib().brats_maxpool2_fwd(ptr, p, optr, op, idx.data_ptr() if idx is not None else None, _code(x.dtype), n, c, d,
                                             h, w, int(with_avg), _stream()), "maxpool2_fwd")
    if idx is not None:
        x._pool_argmax = idx
    return out


def maxpool2_bwd(x, dy, dx_skip=None, with_avg=False):
    ptr, c, p = _desc(x)
    dptr, _, dp = _desc(dy)
    n, d, h, w, _ = x.shape
    dx = new_act(n, d, h, w, c, x.dtype, x.device)
    sptr, sp = (None, 0)
    if dx_skip is not None:
        sptr, _, sp = _desc(dx_skip)
    idx = getattr(x, "_pool_argmax", None)
    if idx is not None:  # recorded by affine_act_pool: the window voxels of x are not read again
        _lib.check(_lib.lib().brats_maxpool2_bwd_idx(idx.data_ptr(), dptr, dp, sptr, sp, dx.data_ptr(), c, _code(x.dtype), n, c,
                                                     d, h, w, int(with_avg), _stream()), "maxpool2_bwd_idx")
        return dx
    _lib.check(_lib.lib().brats_maxpool2_bwd(ptr, p, None, 0, dptr, dp, sptr, sp, dx.data_ptr(), c, _code(x.dtype), n, c,
                                             d, h, w, int(with_avg), _stream()), "maxpool2_bwd")
    return dx


def upsample(x, scale=2, out=None):
    ptr, c, p = _desc(x)
    n, d, h, w, _ = x.shape
    if out is None:
        out = new_act(n, d * scale, h * scale, w * scale, c, x.dtype, x.device)
    optr, oc, op = _desc(out)
    _lib.check(_lib.lib().brats_upsample_fwd(ptr, p, optr, op, _code(x.dtype), n, c, d, h, w, scale, _stream()),
               "upsample_fwd")
    return out


def set_upsample_bwd_fused(mode):
    """brats_upsample_bwd_set_fused: 1 / 0 = the one-launch x2 adjoint of 16-bit tensors on / off (off: three passes through the
    workspace everywhere), -1 = default (on where it tiles).  Bit-identical results.  Returns the previous setting."""
    return _lib.lib().brats_upsample_bwd_set_fused(mode)


def upsample_bwd(dy, scale=2, add=None, out=None):
    """The adjoint of upsample; add (a tensor of the result's shape and dtype, e.g. the gradient another consumer of the same
    activation produced): the result is upsample_bwd(dy) + add, bit for bit, in the same launches (brats_upsample_bwd_add).
    out: a channel-slice view to write into instead of a new tensor."""
    dptr, c, dp = _desc(dy)
    n, do, ho, wo, _ = dy.shape
    d, h, w = do // scale, ho // scale, wo // scale
    code = _code(dy.dtype)
    ws = torch.empty(_lib.lib().brats_upsample_bwd_ws_bytes(code, n, c, d, h, w, scale), dtype=torch.uint8, device=dy.device)
    dx = new_act(n, d, h, w, c, dy.dtype, dy.device) if out is None else out
    xptr, xc, xp = _desc(dx)
    if tuple(dx.shape) != (n, d, h, w, c) or dx.dtype != dy.dtype:
        raise ValueError(f"upsample_bwd: out {tuple(dx.shape)} {dx.dtype} does not match {(n, d, h, w, c)} {dy.dtype}")
    if add is None:
        _lib.check(_lib.lib().brats_upsample_bwd(dptr, dp, xptr, xp, ws.data_ptr(), code, n, c, d, h, w, scale, _stream()), "upsample_bwd")
        return dx
    if tuple(add.shape) != (n, d, h, w, c) or add.dtype != dy.dtype:
        raise ValueError(f"upsample_bwd: addend {tuple(add.shape)} {add.dtype} does not match {(n, d, h, w, c)} {dy.dtype}")
    aptr, _, ap = _desc(add)
    _lib.check(_lib.lib().brats_upsample_bwd_add(dptr, dp, aptr, ap, xptr, xp, ws.data_ptr(), code, n, c, d, h, w, scale, _stream()),
               "upsample_bwd_add")
    return dx


def upsample_nearest(x, scale=2, out=None):
    """nn.Upsample(scale_factor=2) in its default mode on an NDHWC tensor: out[n][z][y][x] = x[n][z // 2][y // 2][x // 2], a copy.
    out: a channel-slice view to write into instead of a new tensor."""
    ptr, c, p = _desc(x)
    n, d, h, w, _ = x.shape
    if out is None:
        out = new_act(n, d * scale, h * scale, w * scale, c, x.dtype, x.device)
    optr, oc, op = _desc(out)
    if tuple(out.shape) != (n, d * scale, h * scale, w * scale, c) or out.dtype != x.dtype:
        raise ValueError(f"upsample_nearest: out {tuple(out.shape)} {out.dtype} does not match {(n, d * scale, h * scale, w * scale, c)} {x.dtype}")
    _lib.check(_lib.lib().brats_upsample_nearest_fwd(ptr, p, optr, op, _code(x.dtype), n, c, d, h, w, scale, _stream()),
               "upsample_nearest_fwd")
    return out


def upsample_nearest_bwd(dy, scale=2, add=None, out=None):
    """The adjoint of upsample_nearest: every coarse voxel = the f32 sum of its 8 children, in one launch without a workspace.
    add / out: as in upsample_bwd (the result is upsample_nearest_bwd(dy) + add, bit for bit)."""
    dptr, c, dp = _desc(dy)
    n, do, ho, wo, _ = dy.shape
    if do % scale or ho % scale or wo % scale:
        raise ValueError(f"upsample_nearest_bwd: the extent {(do, ho, wo)} is no multiple of the scale {scale}")
    d, h, w = do // scale, ho // scale, wo // scale
    dx = new_act(n, d, h, w, c, dy.dtype, dy.device) if out is None else out
    xptr, xc, xp = _desc(dx)
    if tuple(dx.shape) != (n, d, h, w, c) or dx.dtype != dy.dtype:
        raise ValueError(f"upsample_nearest_bwd: out {tuple(dx.shape)} {dx.dtype} does not match {(n, d, h, w, c)} {dy.dtype}")
    aptr, ap = None, 0
    if add is not None:
        if tuple(add.shape) != (n, d, h, w, c) or add.dtype != dy.dtype:
            raise ValueError(f"upsample_nearest_bwd: addend {tuple(add.shape)} {add.dtype} does not match {(n, d, h, w, c)} {dy.dtype}")
        aptr, _, ap = _desc(add)
    _lib.check(_lib.lib().brats_upsample_nearest_bwd(dptr, dp, aptr, ap, xptr, xp, _code(dy.dtype), n, c, d, h, w, scale, _stream()),
               "upsample_nearest_bwd")
    return dx


def _planes(t, what):
    if t.dim() != 5 or not t.is_cuda:
        raise _lib.BratsHipError(f"{what}: expected a CUDA tensor of shape [N, K, D, H, W]")
    return t.contiguous().float()


def planes_nearest(low, scale):
    """nn.Upsample(scale_factor=scale) in its default mode on f32 NCDHW planes (the deep-head logits), scale 2, 4 or 8."""
    low = _planes(low, "planes_nearest")
    n, k, d, h, w = low.shape
    out = torch.empty((n, k, d * scale, h * scale, w * scale), dtype=torch.float32, device=low.device)
    _lib.check(_lib.lib().brats_planes_nearest_fwd(low.data_ptr(), out.data_ptr(), n * k, d, h, w, scale, _stream()), "planes_nearest_fwd")
    return out


def planes_nearest_bwd(dout, scale):
    """The adjoint of planes_nearest: every coarse element = the f32 sum of its scale^3 block, in one fixed order."""
    dout = _planes(dout, "planes_nearest_bwd")
    n, k, do, ho, wo = dout.shape
    if do % scale or ho % scale or wo % scale:
        raise ValueError(f"planes_nearest_bwd: the extent {(do, ho, wo)} is no multiple of the scale {scale}")
    dlow = torch.empty((n, k, do // scale, ho // scale, wo // scale), dtype=torch.float32, device=dout.device)
    _lib.check(_lib.lib().brats_planes_nearest_bwd(dout.data_ptr(), dlow.data_ptr(), n * k, do // scale, ho // scale, wo // scale, scale,
                                                   _stream()), "planes_nearest_bwd")
    return dlow


# ------------------------------------------------------------------------------------------ heads
def head(x, weight, bias, scale=1):
    """NCDHW f32 logits [N, K, D*s, H*s, W*s] = upsample_s(conv1x1(x)); weight [K, C, 1,1,1]."""
    ptr, c, p = _desc(x)
    n, d, h, w, _ = x.shape
    k = weight.shape[0]
    wf = weight.detach().reshape(k, c).contiguous().float()
    out = torch.empty((n, k, d * scale, h * scale, w * scale), dtype=torch.float32, device=x.device)
    low = torch.empty((n, k, d, h, w), dtype=torch.float32, device=x.device) if scale > 1 else None
    _lib.check(_lib.lib().brats_head_fwd(ptr, p, wf.data_ptr(), _f32(bias.detach()) if bias is not None else None,
                                         low.data_ptr() if low is not None else None, out.data_ptr(), _code(x.dtype), n, c,
                                         k, d, h, w, scale, _stream()), "head_fwd")
    return out


def gn_head(y, scale_shift, weight, bias, act="relu", slope=0.01):
    """NCDHW f32 logits of the output head on act(GroupNorm(y)) without storing that activation
    (include/brats_hip.h: brats_gn_head_fwd); bit-identical to head(affine_act(y, scale_shift, act), weight, bias)."""
    ptr, c, p = _desc(y)
    n, d, h, w, _ = y.shape
    k = weight.shape[0]
    wf = weight.detach().reshape(k, c).contiguous().float()
    out = torch.empty((n, k, d, h, w), dtype=torch.float32, device=y.device)
    _lib.check(_lib.lib().brats_gn_head_fwd(ptr, p, scale_shift.data_ptr(), ACTS[act], slope, wf.data_ptr(),
                                            _f32(bias.detach()) if bias is not None else None, out.data_ptr(), _code(y.dtype), n, c,
                                            k, d * h * w, _stream()), "gn_head_fwd")
    return out


def head_bwd(x, weight, dout, scale=1, want_dx=True):
    """Returns (dx | None, dweight [K,C,1,1,1], dbias [K])."""
    ptr, c, p = _desc(x)
    n, d, h, w, _ = x.shape
    k = weight.shape[0]
    wf = weight.detach().reshape(k, c).contiguous().float()
    dout = dout.contiguous().float()
    nbytes = _lib.lib().brats_head_bwd_ws_bytes(n, c, k, d, h, w, scale)
    ws = torch.empty(max(nbytes, 4) // 4, dtype=torch.float32, device=x.device)
    dx = new_act(n, d, h, w, c, x.dtype, x.device) if want_dx else None
    dw = torch.empty((k, c), dtype=torch.float32, device=x.device)
    db = torch.empty(k, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().brats_head_bwd(ptr, p, wf.data_ptr(), dout.data_ptr(), ws.data_ptr(),
                                         dx.data_ptr() if dx is not None else None, c, dw.data_ptr(), db.data_ptr(),
                                         _code(x.dtype), n, c, k, d, h, w, scale, _stream()), "head_bwd")
    return dx, dw.reshape(k, c, 1, 1, 1), db


# ------------------------------------------------------------------------------------------ EvoNorm-S0 / SE helpers
def evonorm_finalize(stats, n, c, groups, voxels, eps=1e-5):
    """Returns (mean_rstd [N, groups, 2], chan [N, C, 2] f64 per-channel sums kept for the backward)."""
    mean_rstd = torch.empty((n, groups, 2), dtype=torch.float32, device=stats.device)
    chan = torch.empty(_lib.lib().brats_gn_ws_doubles(n, c), dtype=torch.float64, device=stats.device)  # totals first
    _lib.check(_lib.lib().brats_evonorm_finalize(stats.data_ptr(), stats.shape[1], n, c, groups, float(voxels), eps,
                                                 mean_rstd.data_ptr(), chan.data_ptr(), _stream()), "evonorm_finalize")
    return mean_rstd, chan


def evonorm(y, mean_rstd, gamma, beta, groups=8, out=None, want_chansum=False, amax=None):
    """z = y*sigmoid(y) * rstd_g * gamma + beta; optionally also sum_v z per (n, c) (SE's pooling)."""
    ptr, c, p = _desc(y)
    n, d, h, w, _ = y.shape
    if out is None:
        out = new_act(n, d, h, w, c, y.dtype, y.device)
    optr, _, op = _desc(out)
    cs = torch.empty(_lib.lib().brats_chan_ws_floats(n, c, 1), dtype=torch.float32, device=y.device) if want_chansum else None
    _lib.check(_lib.lib().brats_evonorm_fwd(ptr, p, mean_rstd.data_ptr(), _f32(gamma), _f32(beta), optr, op,
                                            cs.data_ptr() if cs is not None else None, _code(y.dtype), n, d * h * w, c,
                                            groups, _f32(amax), _stream()), "evonorm_fwd")
    return out, (cs[:n * c].view(n, c) if cs is not None else None)


def evonorm_bwd(dz, y, mean_rstd, gamma, groups=8, chan=None, amax=None, gscale=None, gadd=None):
    """Returns (dy, dgamma, dbeta, dconvbias|None); dconvbias = sum_v dy needs the forward's `chan` sums.
    gscale / gadd ([N, C] f32): the incoming gradient is read as dz * gscale + gadd (the SE layer's backward folded in)."""
    dzp, c, dzpitch = _desc(dz)
    yp, _, ypitch = _desc(y)
    n, d, h, w, _ = y.shape
    dy = new_act(n, d, h, w, c, y.dtype, y.device)
    red = torch.empty(_lib.lib().brats_chan_ws_floats(n, c, 3), dtype=torch.float32, device=y.device)
    dgamma = torch.empty(c, dtype=torch.float32, device=y.device)
    dbeta = torch.empty(c, dtype=torch.float32, device=y.device)
    dcb = torch.empty(c, dtype=torch.float32, device=y.device) if chan is not None else None
    _lib.check(_lib.lib().brats_evonorm_bwd(dzp, dzpitch, yp, ypitch, mean_rstd.data_ptr(), _f32(gamma), dy.data_ptr(), c,
                                            red.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(),
                                            chan.data_ptr() if chan is not None else None,
                                            dcb.data_ptr() if dcb is not None else None, _code(y.dtype), n,
                                            d * h * w, c, groups, _f32(amax), _f32(gscale.contiguous()) if gscale is not None else None,
                                            _f32(gadd.contiguous()) if gadd is not None else None, _stream()), "evonorm_bwd")
    return dy, dgamma, dbeta, dcb


def evonorm_bwd_tiles(tile_stats, dz, y, mean_rstd, gamma, beta, groups=8, chan=None, amax=None):
    """evonorm_bwd whose first pass was taken by conv3d_bstats(..., fwd_y = z, act="leakyrelu", slope=1.0) -- tile_stats = per tile
    and channel (sum dz, sum dz * z) with z the EvoNorm's stored output (include/brats_hip.h: brats_evonorm_bwd_tiles).
    -> (dy, dgamma, dbeta, dconvbias|None)."""
    dzp, c, dzpitch = _desc(dz)
    yp, _, ypitch = _desc(y)
    n, d, h, w, _ = y.shape
    dy = new_act(n, d, h, w, c, y.dtype, y.device)
    red = torch.empty(_lib.lib().brats_evonorm_bwd_tiles_ws_floats(n, c), dtype=torch.float32, device=y.device)
    dgamma = torch.empty(c, dtype=torch.float32, device=y.device)
    dbeta = torch.empty(c, dtype=torch.float32, device=y.device)
    dcb = torch.empty(c, dtype=torch.float32, device=y.device) if chan is not None else None
    _lib.check(_lib.lib().brats_evonorm_bwd_tiles(tile_stats.data_ptr(), tile_stats.shape[1], dzp, dzpitch, yp, ypitch, mean_rstd.data_ptr(),
                                                  _f32(gamma), _f32(beta), dy.data_ptr(), c, red.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(),
                                                  chan.data_ptr() if chan is not None else None, dcb.data_ptr() if dcb is not None else None,
                                                  _code(y.dtype), n, d * h * w, c, groups, _f32(amax), _stream()), "evonorm_bwd_tiles")
    return dy, dgamma, dbeta, dcb


def channel_dot(a, b=None):
    """[N, C] f32 = sum over voxels of a (* b)."""
    ap, c, apitch = _desc(a)
    bp, bpitch = (None, 0)
    if b is not None:
        bp, _, bpitch = _desc(b)
    n, d, h, w, _ = a.shape
    out = torch.empty(_lib.lib().brats_chan_ws_floats(n, c, 1), dtype=torch.float32, device=a.device)
    _lib.check(_lib.lib().brats_channel_dot(ap, apitch, bp, bpitch, out.data_ptr(), _code(a.dtype), n, d * h * w, c,
                                            _stream()), "channel_dot")
    return out[:n * c].view(n, c)


def channel_scale(a, scale, add=None, out=None, amax=None):
    """out[v][c] = a[v][c] * scale[n][c] (+ add[n][c])."""
    ap, c, apitch = _desc(a)
    n, d, h, w, _ = a.shape
    if out is None:
        out = new_act(n, d, h, w, c, a.dtype, a.device)
    optr, _, op = _desc(out)
    _lib.check(_lib.lib().brats_channel_scale(ap, apitch, _f32(scale.contiguous()), _f32(add.contiguous()) if add is not None else None,
                                              optr, op, _code(a.dtype), n, d * h * w, c, _f32(amax), _stream()), "channel_scale")
    return out


def se_gate(chansum, voxels, w1, b1, w2, b2):
    """ResidualSELayer gate from the channel sums of z: -> (1 + gate [N, C], hidden [N, C/r]) in one launch."""
    n, c = chansum.shape
    ch = w1.shape[0]
    gate1p = torch.empty((n, c), dtype=torch.float32, device=chansum.device)
    hidden = torch.empty((n, ch), dtype=torch.float32, device=chansum.device)
    _lib.check(_lib.lib().brats_se_fwd(_f32(chansum.contiguous()), 1.0 / float(voxels), _f32(w1.detach().contiguous()), _f32(b1.detach()),
                                       _f32(w2.detach().contiguous()), _f32(b2.detach()), gate1p.data_ptr(), hidden.data_ptr(),
                                       n, c, ch, _stream()), "se_fwd")
    return gate1p, hidden


def se_gate_bwd(dgate, chansum, voxels, hidden, gate1p, w1, w2):
    """-> (gadd [N, C] = d loss / d gap / V, dW1, db1, dW2, db2) in one launch."""
    n, c = chansum.shape
    ch = w1.shape[0]
    dev = chansum.device
    gadd = torch.empty((n, c), dtype=torch.float32, device=dev)
    dw1, db1 = torch.empty((ch, c), dtype=torch.float32, device=dev), torch.empty((ch,), dtype=torch.float32, device=dev)
    dw2, db2 = torch.empty((c, ch), dtype=torch.float32, device=dev), torch.empty((c,), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().brats_se_bwd(_f32(dgate.contiguous()), _f32(chansum.contiguous()), 1.0 / float(voxels), _f32(hidden), _f32(gate1p),
                                       _f32(w1.detach().contiguous()), _f32(w2.detach().contiguous()), gadd.data_ptr(), dw1.data_ptr(),
                                       db1.data_ptr(), dw2.data_ptr(), db2.data_ptr(), n, c, ch, _stream()), "se_bwd")
    return gadd, dw1, db1, dw2, db2


def evonorm_se(y, mean_rstd, gamma, beta, w1, b1, w2, b2, groups=8, out=None, amax=None, apply=True):
    """EvoNorm + ResidualSELayer in one call, the EvoNorm output never stored (csrc/se.hpp):
    -> (out = z * (1 + gate), chansum [N, C] = sum_v z, gate1p [N, C], hidden [N, C/r]).
    apply=False: statistics pass + gate only (out = None): the consumer recomputes the output on load (evonorm_head)."""
    ptr, c, p = _desc(y)
    n, d, h, w, _ = y.shape
    ch = w1.shape[0]
    dev = y.device
    if not apply:
        out, optr, op = None, None, 0
    else:
        if out is None:
            out = new_act(n, d, h, w, c, y.dtype, dev)
        optr, _, op = _desc(out)
    ws = torch.empty(_lib.lib().brats_chan_ws_floats(n, c, 1), dtype=torch.float32, device=dev)
    cs = torch.empty((n, c), dtype=torch.float32, device=dev)
    gate1p = torch.empty((n, c), dtype=torch.float32, device=dev)
    hidden = torch.empty((n, ch), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().brats_evonorm_se_fwd(ptr, p, mean_rstd.data_ptr(), _f32(gamma), _f32(beta), _f32(w1.detach().contiguous()),
                                               _f32(b1.detach()), _f32(w2.detach().contiguous()), _f32(b2.detach()), optr, op,
                                               ws.data_ptr(), cs.data_ptr(), gate1p.data_ptr(), hidden.data_ptr(), ch,
                                               _code(y.dtype), n, d * h * w, c, groups, _f32(amax), _stream()), "evonorm_se_fwd")
    return out, cs, gate1p, hidden


def evonorm_head(y, mean_rstd, gamma, beta, gate1p, weight, bias, groups=8):
    """NCDHW f32 logits of the output head on the gated EvoNorm output of y without storing it
    (include/brats_hip.h: brats_evonorm_head_fwd); bit-identical to head(evonorm_se(...)[0], weight, bias)."""
    ptr, c, p = _desc(y)
    n, d, h, w, _ = y.shape
    k = weight.shape[0]
    # the per-(n, channel) constants in the kernel's own order of operations: (rstd * gamma) * gate1p, beta * gate1p
    rstd = mean_rstd[:, :, 1].repeat_interleave(c // groups, dim=1)
    ss = torch.stack(((rstd * gamma.float()) * gate1p, beta.float() * gate1p), -1).contiguous()
    wf = weight.detach().reshape(k, c).contiguous().float()
    out = torch.empty((n, k, d, h, w), dtype=torch.float32, device=y.device)
    _lib.check(_lib.lib().brats_evonorm_head_fwd(ptr, p, ss.data_ptr(), wf.data_ptr(), _f32(bias.detach()) if bias is not None else None,
                                                 out.data_ptr(), _code(y.dtype), n, c, k, d * h * w, _stream()), "evonorm_head_fwd")
    return out


def evonorm_se_bwd(do, y, mean_rstd, gamma, beta, se_chansum, hidden, gate1p, w1, w2, groups=8, chan=None, amax=None, head=None,
                   pool=None):
    """EvoNorm backward of the layer under a ResidualSELayer with the SE backward folded in (csrc/se.hpp): `do` is the
    gradient of the SE block's OUTPUT.  -> (dy, dgamma, dbeta, dconvbias|None, dW1, db1, dW2, db2).
    head = (head_weight [K,C,1,1,1], dlogits [N,K,D,H,W]) instead of `do` (None): the block feeds only the 1x1x1 output head,
    whose backward is folded in too; two more results: dhead_weight [K,C,1,1,1], dhead_bias [K].
    pool = (d_skip, d_pooled, argmax bytes, with_avg) instead of `do` (None): the block ends an encoder level, `do` = d_skip +
    pooling-backward(d_pooled) is composed inside the passes (brats_evonorm_se_bwd_pool)."""
    yp, c, ypitch = _desc(y)
    n, d, h, w, _ = y.shape
    ch = w1.shape[0]
    dev = y.device

    def f32(*shape):
        return torch.empty(shape, dtype=torch.float32, device=dev)

    dy = new_act(n, d, h, w, c, y.dtype, dev)
    ws = f32(_lib.lib().brats_chan_ws_floats(n, c, 5) + n * c * 3)
    dgamma, dbeta, dcb = f32(c), f32(c), (f32(c) if chan is not None else None)
    gadd, dw1, db1, dw2, db2 = f32(n, c), f32(ch, c), f32(ch), f32(c, ch), f32(c)
    # the arguments the two entry points share, in their order
    norm = (yp, ypitch, mean_rstd.data_ptr(), _f32(gamma), _f32(beta), dy.data_ptr(), c, ws.data_ptr(), dgamma.data_ptr(),
            dbeta.data_ptr(), chan.data_ptr() if chan is not None else None, dcb.data_ptr() if dcb is not None else None,
            _f32(se_chansum.contiguous()), _f32(hidden), _f32(gate1p), _f32(w1.detach().contiguous()),
            _f32(w2.detach().contiguous()), gadd.data_ptr(), dw1.data_ptr(), db1.data_ptr(), dw2.data_ptr(), db2.data_ptr(), ch)
    res = (dy, dgamma, dbeta, dcb, dw1, db1, dw2, db2)
    if pool is not None:
        sp, _, spitch = _desc(pool[0])
        pp, _, ppitch = _desc(pool[1])
        _lib.check(_lib.lib().brats_evonorm_se_bwd_pool(sp, spitch, pp, ppitch, pool[2].data_ptr(), int(pool[3]), d, h, w, *norm,
                                                        _code(y.dtype), n, c, groups, _f32(amax), _stream()), "evonorm_se_bwd_pool")
        return res
    if head is None:
        dop, _, dopitch = _desc(do)
        dl = hw = hws = dhw = dhb = None
        k = 0
    else:
        dop, dopitch = None, 0
        k = head[0].shape[0]
        hw = head[0].detach().reshape(k, c).contiguous().float()
        dl = head[1].contiguous().float()
        hws, dhw, dhb = f32(_lib.lib().brats_gn_bwd_head_ws_floats(n, c, k)), f32(k, c), f32(k)
    _lib.check(_lib.lib().brats_evonorm_se_bwd(dop, dopitch, *norm, _f32(dl), _f32(hw), k, _f32(hws), _f32(dhw), _f32(dhb),
                                               _code(y.dtype), n, d * h * w, c, groups, _f32(amax), _stream()), "evonorm_se_bwd")
    return res if head is None else res + (dhw.reshape(k, c, 1, 1, 1), dhb)


_DCONV_JOB = np.dtype([("term", [("x", "<u8"), ("w", "<u8"), ("xpitch", "<i4"), ("cin", "<i4"), ("ksize", "<i4"), ("dil", "<i4")], (4,)),
                       ("nterms", "<i4"), ("rows", "<i4"), ("bias", "<u8"), ("y", "<u8"), ("ypitch", "<i4"), ("reserved", "<i4")])
# == brats_dconv_job (include/brats_hip.h)


def pack_weights_direct(w, dtype, mode, cin_off=0, cin_cnt=None):
    """w [Cout, Cin, k, k, k] f32 -> the fragment order of the direct (gather) convolution, dconv_run().  Cached under
    torch.no_grad() exactly like pack_weights()."""
    key = None
    if not torch.is_grad_enabled():
        key = (id(w), "direct", str(dtype), mode, cin_off, cin_cnt)
        hit = _cache_get(key, w)
        if hit is not None:
            return hit
    cout_w, k = w.shape[0], w.shape[2]
    cin_w, cnt, kdim, rows, _ = _pack_geometry(w, mode, None, cin_off, cin_cnt)
    code = _code(dtype)
    nbytes = _lib.lib().brats_dconv_packed_bytes(code, k, kdim, rows)
    if nbytes == 0:
        raise _lib.BratsHipError(f"pack_weights_direct: K channels {kdim} must be a multiple of {16 if code in (BF16, F16) else 8}")
    wd = _padded(w, cin_w)
    packed = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    _lib.check(_lib.lib().brats_dconv_pack_weights(wd.data_ptr(), packed.data_ptr(), code, mode, k, cout_w, cin_w, cin_off, cnt,
                                                   _stream()), "dconv_pack_weights")
    if key is not None:
        _cache_put(key, w, packed)
    return packed


def dconv_run(jobs, n, d, h, w, dtype):
    """One launch of the direct (gather) convolution.  jobs: up to 4 of (terms, bias | None, out) with terms = up to 4 of
    (x, packed_w, ksize, dil); out[..., :] = bias + sum over the terms of conv(x, w).  x / out: NDHWC tensors or
    channel-slice views of [n, d, h, w, *]."""
    rec = np.zeros(len(jobs), _DCONV_JOB)
    keep = []
    for j, (terms, bias, out) in enumerate(jobs):
        optr, rows, opitch = _desc(out)
        if out.dtype != dtype or tuple(out.shape[:4]) != (n, d, h, w):
            raise _lib.BratsHipError("dconv_run: bad output tensor")
        rec[j]["nterms"], rec[j]["rows"], rec[j]["y"], rec[j]["ypitch"] = len(terms), rows, optr, opitch
        rec[j]["bias"] = _f32(bias) or 0
        for t, (x, wpk, ksize, dil) in enumerate(terms):
            xptr, cin, xpitch = _desc(x)
            if x.dtype != dtype or tuple(x.shape[:4]) != (n, d, h, w):
                raise _lib.BratsHipError("dconv_run: bad input tensor")
            rec[j]["term"][t] = (xptr, wpk.data_ptr(), xpitch, cin, ksize, dil)
            keep.append(wpk)
    buf = rec.tobytes()
    _lib.check(_lib.lib().brats_dconv_run(buf, len(jobs), _code(dtype), n, d, h, w, _stream()), "dconv_run")


def conv3d_wgrad_shift(x, dy, ksize=1, dil=1, want_dbias=False, out=None, amax_dy=None):
    """dW [cout, cin, k, k, k] f32 (and dbias) of a 1x1x1 convolution, or of a 3x3x3 convolution at any dilation
    (shifted-tap form of the weight-gradient kernel: the ASPP branches with dilation 4 / 6).  Inside a split_precision()
    block f32 tensors run the three-product form (amax_dy: the scale source of dy, see conv3d_wgrad)."""
    ptr, c, p = _desc(x)
    dptr, cout, dp = _desc(dy)
    n, d, h, w, _ = x.shape
    kd = x.dtype
    if _X3 is not None and x.dtype == torch.float32 and c % 8 == 0 and cout % 8 == 0:
        kd = _X3  # (1x1x1 too: the voxel GEMM is MFMA-bound in exact f32 -- 3.0 of EquiUnetASSPEvo-48's 44 ms x3 step)
    code = _code(kd)
    nbytes = _lib.lib().brats_conv3d_wgrad_shift_ws_bytes(code, ksize, n, d, h, w, c, cout)
    ws = torch.empty(max(nbytes, 4) // 4, dtype=torch.float32, device=x.device)
    dw = _grad_out(out, (cout, c, ksize, ksize, ksize), x.device)
    db = torch.empty(cout, dtype=torch.float32, device=x.device) if want_dbias else None
    dbp = db.data_ptr() if db is not None else None
    with _span("conv_wgrad", c, cout, ksize, dil, n, d, h, w, str(kd)):
        if amax_dy is not None and kd in (X3F, X3B):
            _lib.check(_lib.lib().brats_conv3d_x3_wgrad_shift(ptr, c, p, dptr, dp, _f32(amax_dy), ws.data_ptr(), dw.data_ptr(), dbp,
                                                              code, ksize, dil, n, d, h, w, cout, _stream()), "conv3d_x3_wgrad_shift")
        else:
            _lib.check(_lib.lib().brats_conv3d_wgrad_shift(ptr, c, p, dptr, dp, ws.data_ptr(), dw.data_ptr(), dbp, code, ksize, dil,
                                                           n, d, h, w, cout, _stream()), "conv3d_wgrad_shift")
    return dw, db


# ------------------------------------------------------------------------------------------ distance transform
MASK_F32, MASK_U8 = 0, 1


def distance_transform_edt(mask, mode=0):
    """scipy.ndimage.distance_transform_edt(mask) with unit sampling over the last three axes of a cuda tensor [..., D, H, W]
    (every leading index is a volume of its own): f32 distance of each foreground voxel (value != 0; f32, uint8 or bool
    masks are read as they are, other dtypes through f32) to the nearest background voxel, 0 on background, bit-equal to
    scipy's f64 result cast to f32 (csrc/edt.hip; a volume without background: the distance to index (-1, 0, 0), as scipy).
    mode=1: the signed boundary map of the reference's one_hot2dist / OneHotToDist instead (transforms.one_hot_to_dist);
    mode=2: the distance truncated to an integer (the predicted field of the reference's HausdorffLoss).
    No host synchronisation: graph-capturable."""
    if not mask.is_cuda:
        raise _lib.BratsHipError("brats21_amd.ops.distance_transform_edt runs on the GPU only (no CPU fallback)")
    if mask.dim() < 3:
        raise ValueError("distance_transform_edt: expected [..., D, H, W]")
    if mask.dtype == torch.bool:
        m, kind = mask.contiguous().view(torch.uint8), MASK_U8
    elif mask.dtype == torch.uint8:
        m, kind = mask.contiguous(), MASK_U8
    else:
        m, kind = mask.contiguous().float(), MASK_F32
    d, h, w = (int(v) for v in m.shape[-3:])
    out = torch.empty(m.shape, dtype=torch.float32, device=m.device)
    planes = m.numel() // max(1, d * h * w)
    if m.numel() == 0:
        return out
    l = _lib.lib()
    with torch.cuda.device(m.device):
        nbytes = l.brats_edt_ws_bytes(planes, d, h, w)
        if nbytes == 0:
            raise ValueError(f"distance_transform_edt: unsupported shape {tuple(m.shape)} (D, H, W <= 2048, at most 65535 volumes)")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=m.device)
        _lib.check(l.brats_edt(m.data_ptr(), kind, planes, d, h, w, int(mode), out.data_ptr(), ws.data_ptr(), _stream()), "edt")
    return out


# ------------------------------------------------------------------------------------------ exclusive classes
def softmax_planes(logits, inplace=False):
    """torch.softmax(logits, 1) of f32 NCDHW logits [N, K, D, H, W], 2 <= K <= 16 (csrc/softmax_loss.hip); inplace overwrites a
    contiguous f32 input."""
    if not logits.is_cuda:
        raise _lib.BratsHipError("brats21_amd.ops.softmax_planes runs on the GPU only (no CPU fallback)")
    x = logits.contiguous().float()
    n, k = x.shape[:2]
    if x.dim() != 5 or not 2 <= k <= 16:
        raise NotImplementedError(f"softmax_planes: logits {tuple(x.shape)}: [N, K, D, H, W] with 2 <= K <= 16 is built")
    out = x if inplace else torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().brats_softmax_planes(x.data_ptr(), out.data_ptr(), n, k, x[0, 0].numel(), _stream()), "softmax_planes")
    return out


def argmax_labels(prob_sum, img=None):
    """uint8 label map [N, 1, D, H, W] = arg-max over the classes of prob_sum [N, K, D, H, W] (ties to the lowest class); with
    img [N, C, D, H, W] a voxel where every image channel is 0 gets label 0 (remove_background_voxels)."""
    if not prob_sum.is_cuda:
        raise _lib.BratsHipError("brats21_amd.ops.argmax_labels runs on the GPU only (no CPU fallback)")
    p = prob_sum.contiguous().float()
    if p.dim() != 5 or not 1 <= p.shape[1] <= 255:
        raise ValueError(f"argmax_labels: expected [N, K, D, H, W] with K <= 255, got {tuple(p.shape)}")
    n, k = p.shape[:2]
    im = None
    if img is not None:
        im = img.contiguous().float()
        if im.dim() != 5 or im.shape[0] != n or tuple(im.shape[2:]) != tuple(p.shape[2:]):
            raise ValueError(f"image {tuple(im.shape)} does not match predictions {tuple(p.shape)}")
    labels = torch.empty((n, 1) + tuple(p.shape[2:]), dtype=torch.uint8, device=p.device)
    with torch.cuda.device(p.device):
        _lib.check(_lib.lib().brats_argmax_labels(p.data_ptr(), im.data_ptr() if im is not None else None, labels.data_ptr(), n, k,
                                                  im.shape[1] if im is not None else 0, p[0, 0].numel(), _stream()), "argmax_labels")
    return labels


# ------------------------------------------------------------------------------------------ STAPLE fusion
STAPLE_MAX_RATERS = 256
STAPLE_CHUNK = 16  # iterations enqueued between two reads of the done flags (scripts/time_staple.py records the time with it)


def _staple_check_shape(shape):
    shape = tuple(int(v) for v in shape)
    if len(shape) != 5 or min(shape) < 1:
        raise ValueError(f"STAPLE works on [N, C, D, H, W] maps, got shape {shape}")
    if shape[2] * shape[3] * shape[4] >= 2 ** 31:
        raise ValueError(f"STAPLE: {shape[2] * shape[3] * shape[4]} voxels per sample (fewer than 2^31 supported)")
    if shape[0] * shape[1] > 65535:
        raise ValueError(f"STAPLE: {shape[0] * shape[1]} (sample, channel) problems (at most 65535 supported)")
    return shape


class StaplePacker:
    """The streaming input of ``staple``: ``add(mask)`` takes one rater's 0 / 1 map [N, C, D, H, W] (cuda; f32, uint8 or bool;
    foreground = value 1) and keeps ONE BIT of it per voxel -- uint32 planes [N * C, ceil(max_raters / 32), voxels] plus the
    rater's foreground count per (sample, channel) -- so an ensemble of 160 passes costs 20 bytes per voxel and channel, not 640.
    The planes are allocated by the first ``add`` (on ``device``, or on the first mask's device when None)."""

    def __init__(self, shape, max_raters, device=None):
        self.shape = _staple_check_shape(shape)
        if isinstance(max_raters, bool) or not isinstance(max_raters, int) or not 1 <= max_raters <= STAPLE_MAX_RATERS:
            raise ValueError(f"StaplePacker: max_raters must be an int in 1 .. {STAPLE_MAX_RATERS}, got {max_raters!r}")
        self.device = None if device is None else torch.device(device)
        if self.device is not None and self.device.type != "cuda":
            raise _lib.BratsHipError("brats21_amd.ops.StaplePacker runs on the GPU only (no CPU fallback)")
        self.max_raters, self.raters = max_raters, 0
        self.words = (max_raters + 31) // 32
        self.problems = self.shape[0] * self.shape[1]
        self.voxels = self.shape[2] * self.shape[3] * self.shape[4]
        self.bits = self.counts = None

    def add(self, mask):
        if not torch.is_tensor(mask):
            raise TypeError(f"StaplePacker.add: expected a torch.Tensor, got {type(mask).__name__}")
        if tuple(mask.shape) != self.shape:
            raise ValueError(f"StaplePacker.add: map of shape {tuple(mask.shape)}, the packer was made for {self.shape}")
        if not mask.is_cuda:
            raise _lib.BratsHipError("brats21_amd.ops.StaplePacker.add runs on the GPU only (no CPU fallback)")
        if self.raters >= self.max_raters:
            raise ValueError(f"StaplePacker.add: the packer was made for {self.max_raters} raters")
        if self.device is None:
            self.device = mask.device
        if mask.device != self.device:
            raise ValueError(f"StaplePacker.add: map on {mask.device}, the packer is on {self.device}")
        if mask.dtype == torch.bool:
            m, kind = mask.contiguous().view(torch.uint8), MASK_U8
        elif mask.dtype == torch.uint8:
            m, kind = mask.contiguous(), MASK_U8
        else:
            m, kind = mask.contiguous().float(), MASK_F32
        with torch.cuda.device(self.device):
            if self.bits is None:
                self.bits = torch.zeros((self.problems, self.words, self.voxels), dtype=torch.int32, device=self.device)
                self.counts = torch.zeros((self.problems, self.max_raters), dtype=torch.int32, device=self.device)
            _lib.check(_lib.lib().brats_staple_pack(m.data_ptr(), kind, self.bits.data_ptr(), self.counts.data_ptr(), self.max_raters,
                                                    self.problems, self.words, self.voxels, self.raters, _stream()), "staple_pack")
        self.raters += 1
        return self


def _staple_check_threshold(threshold, what="threshold"):
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float)) or not 0.0 <= float(threshold) <= 1.0:
        raise ValueError(f"STAPLE: {what} must be a number in [0, 1], got {threshold!r}")
    return float(threshold)


def staple(raters_or_packer, threshold=0.5, max_iterations=10000, return_probability=False, chunk=None):
    """STAPLE fusion (Warfield et al.) of binary maps, ITK's STAPLEImageFilter as restated in DESIGN.md section 6 -- the
    reference's perform_staple_on_brats_multi_channel (utils/transforms.py:650-687) without SimpleITK and without the host:
    every (sample, channel) is a problem of its own (the reference takes batch 1 only).

    raters_or_packer: a list of R 0 / 1 maps [N, C, D, H, W] (cuda), or a StaplePacker they were streamed into.
    -> (seg, info): seg f32 0 / 1 [N, C, D, H, W] = W > threshold (a NaN weight is background: a channel that no rater marks, or
    that every rater fills, comes out empty, as from ITK); info = device tensors p [N, C, R] (sensitivities), q [N, C, R]
    (specificities), prior [N, C], iterations [N, C] (int32; ITK's GetElapsedIterations()), plus ``probability`` (f64 W) with
    return_probability, and the ints ``chunk`` / ``host_reads``.

    The EM loop is data dependent and driven from here: ``chunk`` iterations (default STAPLE_CHUNK) are enqueued at a time and
    the done flags are read once per chunk -- the only host read.  The kernels skip a finished problem, so the result and
    ``iterations`` do not depend on the chunk length; all sums have a fixed order (csrc/staple.hip), so neither do they on the
    run."""
    threshold = _staple_check_threshold(threshold)
    if isinstance(max_iterations, bool) or not isinstance(max_iterations, int) or not 1 <= max_iterations < 2 ** 31:
        raise ValueError(f"staple: max_iterations must be a positive int, got {max_iterations!r}")
    chunk = STAPLE_CHUNK if chunk is None else chunk
    if isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1:
        raise ValueError(f"staple: chunk must be a positive int, got {chunk!r}")
    if isinstance(raters_or_packer, StaplePacker):
        pk = raters_or_packer
        if pk.raters < 1:
            raise ValueError("staple: the packer holds no rater")
    else:
        raters = list(raters_or_packer)
        if not 1 <= len(raters) <= STAPLE_MAX_RATERS:
            raise ValueError(f"staple: {len(raters)} raters (1 .. {STAPLE_MAX_RATERS} supported)")
        for m in raters:
            if not torch.is_tensor(m):
                raise TypeError(f"staple: expected torch.Tensor maps, got {type(m).__name__}")
            if tuple(m.shape) != tuple(raters[0].shape):
                raise ValueError(f"staple: maps of different shapes {tuple(raters[0].shape)} and {tuple(m.shape)}")
        _staple_check_shape(raters[0].shape)
        if not all(m.is_cuda for m in raters):
            raise _lib.BratsHipError("brats21_amd.ops.staple runs on the GPU only (no CPU fallback)")
        pk = StaplePacker(raters[0].shape, len(raters), raters[0].device)
        for m in raters:
            pk.add(m)
    r, nc, vox, dev = pk.raters, pk.problems, pk.voxels, pk.device
    l = _lib.lib()
    with torch.cuda.device(dev):
        words = (r + 31) // 32
        bits = pk.bits if words == pk.words else pk.bits[:, :words].contiguous()  # (a packer made for more raters than it got)
        state = torch.empty((nc, 2 + 4 * r), dtype=torch.float64, device=dev)
        flags = torch.empty((nc, 4), dtype=torch.int32, device=dev)
        partial = torch.empty((nc, l.brats_staple_blocks(vox), r + 1), dtype=torch.float64, device=dev)
        _lib.check(l.brats_staple_init(bits.data_ptr(), pk.counts.data_ptr(), pk.max_raters, state.data_ptr(), flags.data_ptr(), nc,
                                       r, vox, _stream()), "staple_init")
        enqueued = reads = 0
        while enqueued < max_iterations:
            n = min(chunk, max_iterations - enqueued)
            _lib.check(l.brats_staple_iterate(bits.data_ptr(), pk.counts.data_ptr(), pk.max_raters, state.data_ptr(),
                                              flags.data_ptr(), partial.data_ptr(), nc, r, vox, max_iterations, n, _stream()),
                       "staple_iterate")
            enqueued += n
            if enqueued < max_iterations:  # (after max_iterations every problem is done)
                reads += 1
                if bool(flags[:, 1].all()):
                    break
        seg = torch.empty(pk.shape, dtype=torch.float32, device=dev)
        prob = torch.empty(pk.shape, dtype=torch.float64, device=dev) if return_probability else None
        _lib.check(l.brats_staple_apply(bits.data_ptr(), state.data_ptr(), nc, r, vox, threshold, seg.data_ptr(), MASK_F32,
                                        prob.data_ptr() if prob is not None else None, _stream()), "staple_apply")
    n, c = pk.shape[:2]
    info = {"p": state[:, 2:2 + r].reshape(n, c, r), "q": state[:, 2 + r:2 + 2 * r].reshape(n, c, r),
            "prior": state[:, 0].reshape(n, c), "iterations": flags[:, 2].reshape(n, c), "chunk": chunk, "host_reads": reads}
    if prob is not None:
        info["probability"] = prob
    return seg, info


# ------------------------------------------------------------------------------------------ CBAM attention block
CBAM_EPS = 1e-5  # nn.InstanceNorm3d's default


class CbamSaved:
    """What cbam_fwd keeps for cbam_bwd: only small tensors ([N, C] vectors and f32 / uint16 planes of V voxels)."""
    __slots__ = ("scale", "pooled", "hidden", "argvox", "comp", "cidx", "z", "stats", "pidx")


def _cbam_params(w1, b1, w2, b2, wc, gamma, beta):
    ps = [p.detach().contiguous() for p in (w1, b1, w2, b2, wc, gamma, beta)]
    ch, c = ps[0].shape
    if tuple(ps[2].shape) != (c, ch) or ps[1].numel() != ch or ps[3].numel() != c or ps[4].numel() != 686 or ps[5].numel() != 1 \
            or ps[6].numel() != 1:
        raise _lib.BratsHipError("cbam: parameter shapes do not belong to one CBAM block")
    for p in ps:
        _f32(p)
    return ps, c, ch


def _cbam_storage(x, what):
    if x.dtype == torch.float16:
        raise _lib.BratsHipError(f"{what}: fp16 storage is not built for the CBAM block (float32 or bfloat16)")
    return _code(x.dtype)


def cbam_fwd(x, w1, b1, w2, b2, wc, gamma, beta, out=None, save=True, pool=False):
    """CBAM (channel gate, then spatial gate with InstanceNorm3d(1)) on an NDHWC tensor of float32 or bfloat16 storage:
    -> (out, saved).  Three reads of x and one write of out; x * s and the spatial gate are never stored at x size.
    save=False (inference): nothing is kept, saved is None.  w1 [C/r, C], w2 [C, C/r], wc [1, 2, 7, 7, 7].
    pool=True (D, H, W even): -> (out, maxpool2(out), saved), the pooled tensor written by the last pass (brats_cbam_apply_pool);
    with save, saved.pidx holds the pooling's window-index bytes for cbam_bwd(..., d_pooled=)."""
    l = _lib.lib()
    xp, c, xpitch = _desc(x)
    code = _cbam_storage(x, "cbam_fwd")
    (w1, b1, w2, b2, wc, gamma, beta), cw, ch = _cbam_params(w1, b1, w2, b2, wc, gamma, beta)
    if cw != c:
        raise _lib.BratsHipError(f"cbam_fwd: the block is built for {cw} channels, the tensor has {c}")
    n, d, h, w, _ = x.shape
    v, dev, st = d * h * w, x.device, _stream()
    nb, tiles = l.brats_cbam_blocks(code, c, d, h, w), l.brats_cbam_tiles(d, h, w)
    if nb <= 0:
        _lib.check(-2, "cbam_fwd")
    f32 = dict(dtype=torch.float32, device=dev)
    if out is None:
        out = new_act(n, d, h, w, c, x.dtype, dev)
    optr, oc, opitch = _desc(out)
    if oc != c or out.shape != x.shape or out.dtype != x.dtype:
        raise _lib.BratsHipError("cbam_fwd: bad output tensor")
    sv = CbamSaved()
    sv.pooled, sv.scale = torch.empty((n, 2, c), **f32), torch.empty((n, c), **f32)
    sv.hidden, sv.argvox = torch.empty((n, 2, ch), **f32), torch.empty((n, c), dtype=torch.int32, device=dev)
    sv.comp, sv.z, sv.stats = torch.empty((n, 2, v), **f32), torch.empty((n, v), **f32), torch.empty((n, 2), **f32)
    sv.cidx = torch.empty((n, v), dtype=torch.int16, device=dev) if save else None
    sv.pidx = None
    if pool:
        if d % 2 or h % 2 or w % 2:
            raise _lib.BratsHipError(f"cbam_fwd(pool=True): D, H, W = {d}, {h}, {w} must be even")
        pooled = new_act(n, d // 2, h // 2, w // 2, c, x.dtype, dev)
        pp, _, ppitch = _desc(pooled)
        if save:
            sv.pidx = torch.empty((n, d // 2, h // 2, w // 2, c), dtype=torch.uint8, device=dev)
    part = torch.empty(max(3 * nb * n * c, 3 * n * tiles), **f32)
    with _span("cbam_pool", code, n, c, d, h, w):
        _lib.check(l.brats_cbam_pool(xp, xpitch, part.data_ptr(), sv.pooled.data_ptr(), sv.argvox.data_ptr(), code, n, c, d, h, w, st), "cbam_pool")
    with _span("cbam_gate", code, n, c, d, h, w):
        _lib.check(l.brats_cbam_gate(sv.pooled.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), sv.hidden.data_ptr(),
                                     sv.scale.data_ptr(), n, c, ch, st), "cbam_gate")
    with _span("cbam_compress", code, n, c, d, h, w):
        _lib.check(l.brats_cbam_compress(xp, xpitch, sv.scale.data_ptr(), sv.comp.data_ptr(), sv.cidx.data_ptr() if save else None, code, n, c,
                                         d, h, w, st), "cbam_compress")
    with _span("cbam_spatial", code, n, c, d, h, w):
        _lib.check(l.brats_cbam_spatial(sv.comp.data_ptr(), wc.data_ptr(), sv.z.data_ptr(), part.data_ptr(), sv.stats.data_ptr(), CBAM_EPS, n,
                                        d, h, w, st), "cbam_spatial")
    if pool:
        with _span("cbam_apply_pool", code, n, c, d, h, w):
            _lib.check(l.brats_cbam_apply_pool(xp, xpitch, sv.scale.data_ptr(), sv.z.data_ptr(), sv.stats.data_ptr(), gamma.data_ptr(),
                                               beta.data_ptr(), optr, opitch, pp, ppitch, sv.pidx.data_ptr() if save else None, code, n, c,
                                               d, h, w, st), "cbam_apply_pool")
        return out, pooled, (sv if save else None)
    with _span("cbam_apply", code, n, c, d, h, w):
        _lib.check(l.brats_cbam_apply(xp, xpitch, sv.scale.data_ptr(), sv.z.data_ptr(), sv.stats.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                      optr, opitch, code, n, c, d, h, w, st), "cbam_apply")
    return out, (sv if save else None)


def cbam_bwd(dout, x, saved, w1, b1, w2, b2, wc, gamma, beta, d_pooled=None):
    """Backward of cbam_fwd: -> (dx, dW1, db1, dW2, db2, dWc, dgamma, dbeta).  Five x-sized transfers: dout and x are read for the
    gradient of the spatial gate and the sum_v dout * x * g partials, x once more for the rest of ds, and dout is read and dx
    written by the last pass (which also adds davg / V and the one-hot of the voxel arg-max; it does not need x).
    d_pooled (the block was run with pool=True, save=True): the gradient of the pooled tensor; dout is then the gradient that
    arrives at `out` directly (the skip connection) or None, and the two dout-reading passes compose dout + maxpool2_bwd(d_pooled)
    on load (brats_cbam_bwd_reduce_pool / _bwd_apply_pool) -- bit-identical to maxpool2_bwd(out, d_pooled, dx_skip=dout) first."""
    l = _lib.lib()
    xp, c, xpitch = _desc(x)
    dp, dpitch = (None, 0) if dout is None else _desc(dout)[::2]
    code = _cbam_storage(x, "cbam_bwd")
    if dout is None and d_pooled is None:
        raise _lib.BratsHipError("cbam_bwd: no gradient given")
    if (dout is not None and (dout.shape != x.shape or dout.dtype != x.dtype)) or not isinstance(saved, CbamSaved) or saved.cidx is None:
        raise _lib.BratsHipError("cbam_bwd: dout must have x's shape and dtype, saved must come from cbam_fwd(save=True)")
    if d_pooled is not None:
        pooled_shape = (x.shape[0], x.shape[1] // 2, x.shape[2] // 2, x.shape[3] // 2, x.shape[4])
        if saved.pidx is None or tuple(d_pooled.shape) != pooled_shape or d_pooled.dtype != x.dtype:
            raise _lib.BratsHipError("cbam_bwd: d_pooled must have the pooled tensor's shape and x's dtype, saved must come from "
                                     "cbam_fwd(pool=True, save=True)")
        qp, _, qpitch = _desc(d_pooled)
        pooled_src = (dp, dpitch, qp, qpitch, saved.pidx.data_ptr())
    (w1, b1, w2, b2, wc, gamma, beta), cw, ch = _cbam_params(w1, b1, w2, b2, wc, gamma, beta)
    n, d, h, w, _ = x.shape
    if cw != c or tuple(saved.scale.shape) != (n, c) or tuple(saved.z.shape) != (n, d * h * w):
        raise _lib.BratsHipError("cbam_bwd: saved tensors / parameters do not belong to this input")
    v, dev, st, sv = d * h * w, x.device, _stream(), saved
    nb, tiles = l.brats_cbam_blocks(code, c, d, h, w), l.brats_cbam_tiles(d, h, w)
    f32 = dict(dtype=torch.float32, device=dev)
    dzn, dcomp = torch.empty((n, v), **f32), torch.empty((n, 2, v), **f32)
    asum, rsum, s12 = torch.empty((n, c), **f32), torch.empty((n, c), **f32), torch.empty((n, 2), **f32)
    dpool, tmp = torch.empty((n, 2, c), **f32), torch.empty(n * c + 2 * n * ch, **f32)
    part = torch.empty(max(nb * n * (c + 2), n * tiles * 686), **f32)
    dw1, db1_, dw2, db2_ = torch.empty((ch, c), **f32), torch.empty((ch,), **f32), torch.empty((c, ch), **f32), torch.empty((c,), **f32)
    dwc, dgamma, dbeta = torch.empty((1, 2, 7, 7, 7), **f32), torch.empty((1,), **f32), torch.empty((1,), **f32)
    dx = new_act(n, d, h, w, c, x.dtype, dev)
    dxp, _, dxpitch = _desc(dx)
    # (the pooled forms take (d_skip, pitch, d_pooled, pitch, window indices) where the plain ones take (dout, pitch))
    reduce, apply, src = (("cbam_bwd_reduce", "cbam_bwd_apply", (dp, dpitch)) if d_pooled is None else
                          ("cbam_bwd_reduce_pool", "cbam_bwd_apply_pool", pooled_src))
    with _span(reduce, code, n, c, d, h, w):
        _lib.check(getattr(l, "brats_" + reduce)(*src, xp, xpitch, sv.scale.data_ptr(), sv.z.data_ptr(), sv.stats.data_ptr(), gamma.data_ptr(),
                                                 beta.data_ptr(), dzn.data_ptr(), part.data_ptr(), asum.data_ptr(), s12.data_ptr(), code, n,
                                                 c, d, h, w, st), reduce)
    with _span("cbam_bwd_spatial", code, n, c, d, h, w):
        _lib.check(l.brats_cbam_bwd_spatial(dzn.data_ptr(), sv.z.data_ptr(), sv.stats.data_ptr(), s12.data_ptr(), gamma.data_ptr(),
                                            sv.comp.data_ptr(), wc.data_ptr(), dcomp.data_ptr(), part.data_ptr(), dwc.data_ptr(), n, d, h, w, st),
                   "cbam_bwd_spatial")
    with _span("cbam_bwd_chan", code, n, c, d, h, w):
        _lib.check(l.brats_cbam_bwd_chan(xp, xpitch, dcomp.data_ptr(), sv.cidx.data_ptr(), part.data_ptr(), rsum.data_ptr(), code, n, c, d, h, w,
                                         st), "cbam_bwd_chan")
    with _span("cbam_bwd_gate", code, n, c, d, h, w):
        _lib.check(l.brats_cbam_bwd_gate(asum.data_ptr(), rsum.data_ptr(), sv.pooled.data_ptr(), sv.hidden.data_ptr(), w1.data_ptr(),
                                         b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), s12.data_ptr(), tmp.data_ptr(), dpool.data_ptr(), dw1.data_ptr(),
                                         db1_.data_ptr(), dw2.data_ptr(), db2_.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), n, c, ch, st),
                   "cbam_bwd_gate")
    with _span(apply, code, n, c, d, h, w):
        _lib.check(getattr(l, "brats_" + apply)(*src, sv.scale.data_ptr(), sv.z.data_ptr(), sv.stats.data_ptr(), gamma.data_ptr(),
                                                beta.data_ptr(), dcomp.data_ptr(), sv.cidx.data_ptr(), dpool.data_ptr(), sv.argvox.data_ptr(),
                                                dxp, dxpitch, code, n, c, d, h, w, st), apply)
    return dx, dw1, db1_, dw2, db2_, dwc, dgamma, dbeta


# ------------------------------------------------------------------------------------------ recurrent residual block (R2U-Net)
class RrcnnSaved:
    """What rrcnn_fwd keeps for rrcnn_bwd.  Of tensor size: per RecurrentBlock the stacked unit inputs S and raw convolution outputs
    Y, [(t + 1) N, D, H, W, C] each, and the block input(s) x (x2)."""
    __slots__ = ("x", "x2", "S", "Y", "ss", "mr", "groups", "act", "t", "n")


def _rrcnn_params(params):
    ps = [p.detach() for p in params]
    if len(ps) != 10:
        raise _lib.BratsHipError("rrcnn: ten parameters in the block's state-dict order (RCNN.0.conv.0.weight .. Conv_1x1.bias)")
    c = ps[8].shape[0]
    ok = (ps[8].dim() == 5 and tuple(ps[8].shape[2:]) == (1, 1, 1) and ps[9].numel() == c
          and all(tuple(ps[i].shape) == (c, c, 3, 3, 3) for i in (0, 4)) and all(ps[i].numel() == c for i in (1, 2, 3, 5, 6, 7)))
    if not ok:
        raise _lib.BratsHipError("rrcnn: parameter shapes do not belong to one RRCNNblock")
    for p in ps:
        _f32(p.contiguous())
    return [p.contiguous() for p in ps], c, ps[8].shape[1]


def rrcnn_fwd(x, x2, params, groups=8, act="relu", t=2, save=True):
    """RRCNNblock (networks/unet_family.py:60-101 of the reference) on NDHWC tensors: x0 = conv1x1([x | x2]) + bias, two
    RecurrentBlocks -- ONE conv3x3x3 (bias) -> norm -> act unit applied t + 1 times, to xb and then to xb + previous result --,
    out = x0 + result.  -> (out, saved).  params: the block's ten parameters in state-dict order; groups: 8 (GroupNorm) or C
    (InstanceNorm); x2 (or None): the second source of the 1x1x1 convolution (the virtual concat [x | x2]); x may carry zero
    channels beyond the weight's (a narrow input padded to a channel vector).
    Per application: convolution (+ tile statistics), finalize, and ONE normalise pass that writes the next unit input xb + z
    directly (affine_act_add) -- the plain affine_act only for the first block's result; the last pass of the second block adds
    x0 and writes the output.  save=True: the producers write into slices of the stacked buffers S (unit inputs: x0 is S_A[0:N],
    the first block's result S_B[0:N]) and Y (raw convolution outputs) that rrcnn_bwd reads.  save=False: nothing is kept,
    four activation buffers are reused throughout, saved is None."""
    if x3_active():
        raise NotImplementedError("rrcnn_fwd: the split-precision modes are not built for the recurrent block")
    ps, c, cin = _rrcnn_params(params)
    if t < 1:
        raise _lib.BratsHipError(f"rrcnn_fwd: t = {t} (t >= 1)")
    n, d, h, w, c1 = x.shape
    c2 = x2.shape[-1] if x2 is not None else 0
    if (x2 is not None and (c1 + c2 != cin or x2.dtype != x.dtype or x2.shape[:4] != x.shape[:4])) or (x2 is None and c1 < cin):
        raise _lib.BratsHipError(f"rrcnn_fwd: the block is built for {cin} input channels, the tensors have {c1} + {c2}")
    if c % groups:
        raise _lib.BratsHipError(f"rrcnn_fwd: {c} channels in {groups} groups")
    dtype, dev, vox = x.dtype, x.device, d * h * w
    sv = RrcnnSaved()
    sv.x, sv.x2, sv.groups, sv.act, sv.t, sv.n = x, x2, groups, act, t, n
    sv.S, sv.Y, sv.ss, sv.mr = [], [], [[], []], [[], []]
    if save:
        for _ in range(4):
            (sv.S if len(sv.S) < 2 else sv.Y).append(new_act((t + 1) * n, d, h, w, c, dtype, dev))
        x0 = sv.S[0][:n]
    else:
        x0 = new_act(n, d, h, w, c, dtype, dev)
        ybuf, ping = new_act(n, d, h, w, c, dtype, dev), [new_act(n, d, h, w, c, dtype, dev) for _ in range(2)]
    # (the parameter objects themselves go to pack_weights: its no_grad cache is keyed by them)
    wpk = pack_weights(params[8], dtype, PACK_FWD, cin_pad=c1 + c2, c1=c1 if x2 is not None else None)
    conv3d(x, wpk, c, 1, 1, bias=ps[9], out=x0, x2=x2)
    xb = x0
    for b in (0, 1):
        _, bias, gamma, beta = ps[4 * b:4 * b + 4]
        wpk = pack_weights(params[4 * b], dtype, PACK_FWD)
        cur = xb
        for k in range(t + 1):
            yk = sv.Y[b][k * n:(k + 1) * n] if save else ybuf
            _, stats = conv3d(cur, wpk, c, 3, 1, bias=bias, out=yk, want_stats=True)
            mean_rstd, scale_shift = gn_finalize(stats, n, c, groups, vox, gamma, beta)
            if save:
                sv.ss[b].append(scale_shift)
                sv.mr[b].append(mean_rstd)
            if k < t:
                # the next unit input xb + z.  (save=False: block b's unit inputs live in ping[b]; the convolution that read the
                # previous one has run, so the pass may overwrite it -- it is neither its y nor its add)
                nxt = sv.S[b][(k + 1) * n:(k + 2) * n] if save else ping[b]
                cur = affine_act_add(yk, scale_shift, xb, act, out=nxt)
            elif b == 0:
                # the first block's result has no sum in front of it.  (save=False: it takes over ping[0], which the second block
                # only reads)
                xb = affine_act(yk, scale_shift, act, out=sv.S[1][:n] if save else ping[0])
            else:
                out = affine_act_add(yk, scale_shift, x0, act, out=None if save else ping[1])
    return out, (sv if save else None)


def rrcnn_bwd(dout, saved, params, need_dx=True):
    """Backward of rrcnn_fwd: -> (dx, dx2, grads) with grads the ten parameter gradients in state-dict order, each produced exactly
    once as the finished sum over the t + 1 applications of its unit.  Per RecurrentBlock, from the last application down:
    dy_k = gn_act_bwd(dz_k) written into slice k of a stacked DY, ds_k = dgrad(dy_k) = dz_{k-1}; the gradient of the block input
    is ONE grad_sum over ds_0 .. ds_t (+ dout for x0: the residual); the weight gradient is ONE conv3d_wgrad launch over the
    stacked batch (t + 1) N of (S, DY) -- the sum over applications is the kernel's own reduction over the batch --, the bias
    gradient one channel_dot over DY, dgamma / dbeta the sum of the t + 1 [C] vectors.  need_dx=False: dx (dx2) are None."""
    sv = saved
    if not isinstance(sv, RrcnnSaved):
        raise _lib.BratsHipError("rrcnn_bwd: saved must come from rrcnn_fwd(save=True)")
    if x3_active():
        raise NotImplementedError("rrcnn_bwd: the split-precision modes are not built for the recurrent block")
    ps, c, cin = _rrcnn_params(params)
    n, t, x, x2 = sv.n, sv.t, sv.x, sv.x2
    dtype = x.dtype
    if dout.dtype != dtype or tuple(dout.shape) != tuple(sv.S[0][:n].shape):
        raise _lib.BratsHipError("rrcnn_bwd: dout must have the output's shape and the block's storage type")
    grads = [None] * 10
    dz = dout
    for b in (1, 0):
        gamma = ps[4 * b + 2]
        S, Y = sv.S[b], sv.Y[b]
        DY = torch.empty_like(Y)
        wpk = pack_weights(params[4 * b], dtype, PACK_DGRAD)
        ds, small = [None] * (t + 1), []
        for k in range(t, -1, -1):
            sl = slice(k * n, (k + 1) * n)
            _, dgamma, dbeta = gn_act_bwd(dz, Y[sl], sv.ss[b][k], sv.mr[b][k], gamma, sv.groups, sv.act, out=DY[sl])
            small.append((dgamma, dbeta))
            ds[k], _ = conv3d(DY[sl], wpk, c, 3, 1)
            dz = ds[k]
        dz = grad_sum(*(ds + ([dout] if b == 0 else [])))  # every reader of the block input in one pass
        grads[4 * b], _ = conv3d_wgrad(S, DY, 3, 1)
        grads[4 * b + 1] = channel_dot(DY).sum(0)
        gb = torch.stack([g for g, _ in small] + [g for _, g in small]).view(2, t + 1, c).sum(1)  # [C]-sized: dgamma | dbeta
        grads[4 * b + 2], grads[4 * b + 3] = gb[0], gb[1]
    d_x0 = dz
    c1 = x.shape[-1]
    dws = [conv3d_wgrad_shift(s, d_x0, 1)[0] for s in ((x,) if x2 is None else (x, x2))]
    dw1 = dws[0] if x2 is None else torch.cat(dws, 1)  # (weight-sized)
    grads[8] = dw1[:, :cin].contiguous() if dw1.shape[1] != cin else dw1
    grads[9] = channel_dot(d_x0).sum(0)
    if not need_dx:
        return None, None, grads
    wpk = pack_weights(params[8], dtype, PACK_DGRAD, cin_pad=c1 if x2 is None else None)
    if x2 is None:
        dx, _ = conv3d(d_x0, wpk, c1, 1, 1)
        return dx, None, grads
    if c1 % split_granule(cin) == 0:
        (dx, dx2), _ = conv3d(d_x0, wpk, cin, 1, 1, split=c1)  # two dense tensors, one launch
        return dx, dx2, grads
    dx, _ = conv3d(d_x0, wpk, cin, 1, 1)
    return dx[..., :c1], dx[..., c1:], grads


# ------------------------------------------------------------------------------------------ box calibration
def probe_box(device=None, mfma_ms=50.0, stream_bytes=403 << 20, modes=(0, 1)):
    """What THIS box delivers right now on the two resources the rooflines are quoted against (csrc/probe.hip): 16-bit
    MFMA TFLOP/s with every SIMD issuing back to back (two waves per SIMD, like the convolution kernels), and TB/s of a bf16
    read + write stream over `stream_bytes` (the size of a 2 x 128^3 x 48 activation).  ~120 ms of GPU time (shorter bursts read +-3 % with the chip's power control; 50 ms per
    mode repeats to +-0.1 %: scripts/probe_noise.py), HIP-event timed
    on the current stream.
      mfma_TFLOPs       : dense pseudo-random operands -- the matrix rate the chip SUSTAINS (it holds 1.8-2.0 GHz of its
                          nominal 2.4 GHz under this load: sclk_MHz = 16 cycles per MFMA and SIMD); roofline.frac_of_box
                          is quoted against this number;
      mfma_zeros_TFLOPs : every second operand value zero (post-ReLU activations): less switching power, higher clock --
                          the ceiling for kernels fed with such data.
    (modes 2 / 3 of the probe add vector instructions between the matrix groups: scripts/box_calib.py.)"""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    l = _lib.lib()
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    blocks = 2 * ncu  # 8 waves per CU = two per SIMD, like the convolution kernels
    out = torch.empty(blocks, dtype=torch.float32, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]

    def mfma(iters, mode):
        ev[0].record()
        _lib.check(l.brats_probe_mfma(out.data_ptr(), blocks, iters, mode, _stream()), "probe_mfma")
        ev[1].record()
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1])

    res = {}
    for mode in modes:
        mfma(2000, mode)  # warm-up (code object load, clocks)
        t0 = mfma(20000, mode)
        iters = max(20000, int(20000 * mfma_ms / max(t0, 1e-3)))
        ms = mfma(iters, mode)
        tf = blocks * 4.0 * iters * 8 * 16384 / (ms * 1e-3) / 1e12
        res[mode] = (tf, ms, iters)
    src = torch.empty(stream_bytes, dtype=torch.uint8, device=dev)
    src.view(torch.int16).fill_(0x3c00)
    dst = torch.empty_like(src)
    for _ in range(2):
        _lib.check(l.brats_probe_stream(src.data_ptr(), dst.data_ptr(), stream_bytes, _stream()), "probe_stream")
    reps = 8
    ev[2].record()
    for _ in range(reps):
        _lib.check(l.brats_probe_stream(src.data_ptr(), dst.data_ptr(), stream_bytes, _stream()), "probe_stream")
    ev[3].record()
    ev[3].synchronize()
    sms = ev[2].elapsed_time(ev[3]) / reps
    rec = {"stream_TBps": round(2.0 * stream_bytes / (sms * 1e-3) / 1e12, 3)}
    names = {0: "mfma", 1: "mfma_zeros", 2: "mfma_duty_dense", 3: "mfma_duty"}
    for mode, (tf, ms, iters) in res.items():
        rec[names[mode] + "_TFLOPs"] = round(tf, 1)
    if 0 in res:  # two waves per SIMD x iters x 8 MFMAs x 16 cycles
        rec["sclk_MHz"] = round(2.0 * res[0][2] * 8 * 16 / (res[0][1] * 1e-3) / 1e6, 0)
    rec["probe"] = (f"csrc/probe.hip: {blocks} x 4 waves issuing v_mfma_f32_16x16x32_bf16 back to back, ~{mfma_ms:.0f} ms per mode (mfma = dense "
                    f"random operands: the sustained matrix rate, sclk = the clock behind it at 16 cycles per MFMA and SIMD; mfma_zeros = "
                    f"every second value zero); bf16 read + write stream over {stream_bytes >> 20} MiB, {sms * 1e3:.0f} us per pass")
    return rec
