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

from ._tensors import (X3B, X3F, _NO_ACT, _SIZES, _act, _act2, _code, _conv_packed, _desc, _desc2, _even, _f32, _finalize_in,  # noqa: F401
                       _groups, _head_weight, _out, _packed, _planes, _tile_stats, _vec)

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


def is16(dtype):
    """16-bit storage (bf16 or fp16): the MFMA kernels with f32 accumulation; fp16 is the reference's autocast dtype."""
    return dtype in (torch.bfloat16, torch.float16)


def _fn16(name, dtype):
    """Entry points that move 16-bit data but have no dtype argument exist twice: brats_x (bf16) and brats_x_f16."""
    return getattr(_lib.lib(), name + ("_f16" if dtype == torch.float16 else ""))


def new_act(n, d, h, w, c, dtype, device):
    return torch.empty((n, d, h, w, c), dtype=dtype, device=device)


# ------------------------------------------------------------------------------------------ layout
def ncdhw_to_ndhwc(x, dtype, cpad=None):
    """[N,C,D,H,W] f32 -> [N,D,H,W,cpad] dtype (extra channels zero)."""
    if not isinstance(x, torch.Tensor) or x.dim() != 5 or not x.is_cuda:
        raise _lib.BratsHipError("ncdhw_to_ndhwc: expected a CUDA tensor of shape [N, C, D, H, W]")
    x = x.contiguous().float()  # (any dtype: images arrive as integers too)
    n, c, d, h, w = x.shape
    cpad = cpad or c
    if cpad < c:
        raise _lib.BratsHipError(f"ncdhw_to_ndhwc: cpad = {cpad} is below the tensor's {c} channels")
    out = new_act(n, d, h, w, cpad, dtype, x.device)
    _lib.check(_lib.lib().brats_ncdhw_to_ndhwc(x.data_ptr(), out.data_ptr(), _code(dtype), n, c, cpad, cpad, d, h, w,
                                               _stream()), "ncdhw_to_ndhwc")
    return out


def ndhwc_to_ncdhw(x):
    a = _act(x, "ndhwc_to_ncdhw: x")
    out = torch.empty((a.n, a.c, a.d, a.h, a.w), dtype=torch.float32, device=a.device)
    _lib.check(_lib.lib().brats_ndhwc_to_ncdhw(a.ptr, a.pitch, out.data_ptr(), a.code, a.n, a.c, a.d, a.h, a.w, _stream()),
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


def _on(t, device):
    """Is the tensor t on the CUDA device `device` (a torch.device or string; without an index: any CUDA device)?"""
    d = torch.device(device)
    return t.is_cuda and d.type == "cuda" and d.index in (None, t.device.index)


def _weight(w):
    if not isinstance(w, torch.Tensor) or w.dim() != 5 or not w.is_cuda or not w.is_floating_point():
        raise _lib.BratsHipError("pack_weights: expected a floating-point CUDA tensor [Cout, Cin, k, k, k]")


def _padded(w, cin_w):
    """w (checked: a floating-point CUDA tensor [Cout, Cin, k, k, k]) detached, contiguous f32, its input channels zero-padded
    to cin_w."""
    _weight(w)
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
            if w is None or w.dtype != torch.float32 or not w.is_contiguous() or not _on(w, device):
                continue  # (pack_weights finds no entry for it and takes the per-layer path, which checks it)
            cin_real, k = w.shape[1], w.shape[2]
            cin_w, _, kdim, rows, src = _pack_geometry(w, mode, cin_pad, cin_off, cin_cnt, c1)
            ck = conv_chunk(dtype, k, dil, *src, rows)
            code = _code(dtype)
            nbytes = _SIZES[("conv", code, k, dil, *src, rows)] = _lib.lib().brats_conv3d_packed_bytes(code, k, kdim, rows, ck)
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
    nbytes = _SIZES[("conv", code, k, dil, *src, rows)] = _lib.lib().brats_conv3d_packed_bytes(code, k, kdim, rows, ck)
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
    _SIZES.clear()
    for plan in list(_PLANS.values()):
        plan.dirty = True
        plan.entries = None
    return old


def set_first_min_tiles(n):
    """brats_conv3d_set_first_min_tiles: the number of 4x4x16 tiles from which the first layer (one 8-channel chunk, 16-bit, 3x3x3)
    takes its persistent kernel (dense output) or the 4x8x16-tile kernel (any other output); n <= 0 = the default of 2048.  The
    packed weights do not depend on it.  Returns the previous value."""
    return _lib.lib().brats_conv3d_set_first_min_tiles(int(n))


CONV_FORM_FIRST, CONV_FORM_VS8, CONV_FORM_TILE = 0, 1, 2  # BRATS_CONV_FORM_* of include/brats_hip.h


def conv_form_launches(dtype, form):
    """brats_conv3d_form_launches: how many launches the 16-bit 3x3x3 launchers of `dtype`'s build (torch dtype; fp16 counts on
    its own) have made in form CONV_FORM_FIRST / _VS8 / _TILE since the library was loaded.  Never reset: take differences."""
    if form not in (CONV_FORM_FIRST, CONV_FORM_VS8, CONV_FORM_TILE):
        raise _lib.BratsHipError(f"conv_form_launches: unknown form {form}")
    return int(_lib.lib().brats_conv3d_form_launches(_code(dtype), form))


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


def _conv_outputs(a, cout, out, split, want_stats, what):
    """What a convolution of the activation a writes: -> (y, stats | None, args).  y = `out` (checked), a fresh [N, D, H, W, cout]
    tensor, or -- split -- the pair of dense tensors with the output channels [0, split) and [split, cout); stats = [N, tiles, cout, 2];
    args = (y, pitch, y2, c2, split, stats) as the entry points take them."""
    lead, y2 = a.shape[:4], None
    if split is not None:
        if out is not None or not 0 < split < cout:
            raise _lib.BratsHipError(f"{what}: split = {split} of {cout} channels (no out= with it)")
        y2 = torch.empty(lead + (cout - split,), dtype=a.dtype, device=a.device)
    o = _out(out, lead + (split or cout,), a, (what, "out"))
    stats = torch.empty((a.n, tiles_per_sample(a.d, a.h, a.w), cout, 2), dtype=torch.float32, device=a.device) if want_stats else None
    args = (o.ptr, o.pitch, y2.data_ptr() if y2 is not None else None, (cout - split) if y2 is not None else 0, split or 0,
            stats.data_ptr() if stats is not None else None)
    return ((o.t, y2) if y2 is not None else o.t), stats, args


def conv3d(x, packed_w, cout, ksize=3, dil=1, bias=None, out=None, want_stats=False, x2=None, split=None, amax=None):
    if isinstance(x, Pending) or isinstance(x2, Pending):
        return _conv3d_pre(x, packed_w, cout, ksize, dil, bias, out, want_stats, x2)
    return _conv3d(x, packed_w, cout, ksize, dil, bias, out, want_stats, x2, split, amax)


def _conv3d_pre(x, packed_w, cout, ksize, dil, bias, out, want_stats, x2):
    """conv3d whose input(s) are Pending activations: normalise + act applied while the halo tile is staged."""
    p1 = x if isinstance(x, Pending) else None
    p2 = x2 if isinstance(x2, Pending) else None
    if p1 is not None and p2 is not None and (p1.act != p2.act or p1.slope != p2.slope):
        raise _lib.BratsHipError("conv3d: the two pending inputs carry different activations")
    act, slope = (p1 or p2).act, (p1 or p2).slope
    a, b = _conv_sources(p1.y if p1 is not None else x, p2.y if p2 is not None else x2, "conv3d")
    ss1 = _vec(p1.scale_shift, a.n * a.c * 2, "conv3d: x.scale_shift", a) if p1 is not None else None
    ss2 = _vec(p2.scale_shift, a.n * b.c * 2, "conv3d: x2.scale_shift", a) if p2 is not None else None
    wp = _conv_packed(packed_w, a.code, ksize, dil, a.c, b.c, cout, "conv3d", a)
    out, stats, (optr, op, _, _, _, sptr) = _conv_outputs(a, cout, out, None, want_stats, "conv3d")
    with _span("conv_igemm", a.c + b.c, cout, ksize, dil, a.n, a.d, a.h, a.w, str(a.dtype)):
        _lib.check(_lib.lib().brats_conv3d_fwd_pre(a.ptr, a.c, a.pitch, ss1, b.ptr, b.c, b.pitch, ss2, ACTS[act], float(slope), wp,
                                                   _vec(bias, cout, "conv3d: bias", a, null=True), optr, op, sptr, a.code, dil, a.n,
                                                   a.d, a.h, a.w, cout, _stream()), "conv3d_fwd_pre")
    return out, stats


def _conv_sources(x, x2, what):
    """The checked input [x | x2] of a convolution: -> (_Act of x, _Act of x2 or _NO_ACT)."""
    a = _act(x, (what, "x"))
    return a, _act2(x2, (what, "x2"), a, anyc=True)


def _conv3d(x, packed_w, cout, ksize=3, dil=1, bias=None, out=None, want_stats=False, x2=None, split=None, amax=None):
    """y[N,D,H,W,cout] = conv([x | x2]) with weights from pack_weights().  Returns (y, stats|None) where
    stats = [N, tiles, cout, 2] per-tile per-channel (sum, sum of squares) of the f32 result.
    x2: optional second input (virtual concat, no torch.cat).  split: write output channels
    [0, split) and [split, cout) to two dense tensors (returns (y, y2) as y).
    amax (split precision only): 1-element f32 device tensor holding max|x| -- the input is scaled into fp16's range by the
    matching power of two and the result scaled back (brats_conv3d_x3_fwd: the input gradient, whose x = dY is tiny)."""
    a, b = _conv_sources(x, x2, "conv3d")
    kd = _conv_dtype(a.dtype, ksize)  # (split precision: f32 tensors, weights packed under the same mode)
    code = _code(kd)
    wp = _conv_packed(packed_w, code, ksize, dil, a.c, b.c, cout, "conv3d", a)
    bp = _vec(bias, cout, "conv3d: bias", a, null=True)
    y, stats, oargs = _conv_outputs(a, cout, out, split, want_stats, "conv3d")
    with _span("conv_igemm", a.c + b.c, cout, ksize, dil, a.n, a.d, a.h, a.w, str(kd)):
        if amax is not None and kd in (X3F, X3B):
            _lib.check(_lib.lib().brats_conv3d_x3_fwd(a.ptr, a.c, a.pitch, b.ptr, b.c, b.pitch, _vec(amax, 1, "conv3d: amax", a), wp, bp,
                                                      *oargs, code, dil, a.n, a.d, a.h, a.w, cout, _stream()), "conv3d_x3_fwd")
        else:
            _lib.check(_lib.lib().brats_conv3d_fwd(a.ptr, a.c, a.pitch, b.ptr, b.c, b.pitch, wp, bp, *oargs, code, ksize, dil, a.n, a.d,
                                                   a.h, a.w, cout, _stream()), "conv3d_fwd")
    return y, stats


# ------------------------------------------------------------------------------------------ narrow-output conv
def pack_weights_narrow(w, mode):
    """w: torch-layout [Cout, Cin, 3, 3, 3] f32 -> the f32 buffer conv3d_narrow() reads.  PACK_FWD: Cout <= 16 class rows over Cin
    channels; PACK_DGRAD: Cin <= 16 class rows over Cout channels, transposed with the taps flipped (the input gradient as a
    convolution of dy).  The channel count must be a multiple of 8.  Cached under no_grad like pack_weights()."""
    _weight(w)
    if tuple(w.shape[2:]) != (3, 3, 3):
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
    a = _act(x, "conv3d_narrow: x")
    n, d, h, w, c = a.shape
    # (the size query is made per call, as it always was: exact equality, not a lower bound, tells a foreign buffer)
    if packed_w.numel() * 4 != _lib.lib().brats_conv3d_narrow_packed_bytes(c, k):
        raise _lib.BratsHipError(f"conv3d_narrow: the packed weights do not belong to a {c} -> {k} layer")
    if add is not None and tuple(add.shape) != (n, k, d, h, w):
        raise _lib.BratsHipError(f"conv3d_narrow: add has shape {tuple(add.shape)}, expected {(n, k, d, h, w)}")
    wp = _vec(packed_w, None, "conv3d_narrow: packed_w", a)
    out = torch.empty((n, k, d, h, w), dtype=torch.float32, device=a.device)
    with _span("conv_narrow", c, k, n, d, h, w, str(a.dtype)):
        _lib.check(_lib.lib().brats_conv3d_narrow_fwd(a.ptr, c, a.pitch, wp, _vec(bias, k, "conv3d_narrow: bias", a, null=True),
                                                      _vec(add, None, "conv3d_narrow: add", a, null=True), out.data_ptr(), a.code, k,
                                                      n, d, h, w, _stream()), "conv3d_narrow_fwd")
    return out


# ------------------------------------------------------------------------------------------ fp8 conv
def absmax(x):
    """max|x| of an NDHWC tensor as a 1-element f32 device tensor (no host sync)."""
    a = _act(x, "absmax: x")
    out = torch.empty(1, dtype=torch.float32, device=a.device)
    _lib.check(_lib.lib().brats_absmax(a.ptr, a.pitch, a.code, a.n * a.vox, a.c, out.data_ptr(), _stream()), "absmax")
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
    nbytes = _SIZES[("f8", *src, rows)] = _lib.lib().brats_conv3d_f8_packed_bytes(kdim, rows, ck)
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
    a, b = _conv_sources(x, x2, "conv3d_f8")
    if xscale is None:
        if amax is None:
            amax = absmax(x)
        if x2 is not None and amax2 is None:
            amax2 = absmax(x2)
    else:
        amax = amax2 = None
    wp = _packed(packed_w, ("f8", a.c, b.c, cout), lambda: _lib.lib().brats_conv3d_f8_packed_bytes(
        a.c + b.c, cout, max(1, conv_f8_chunk(a.c, b.c))), "conv3d_f8", a)
    y, stats, oargs = _conv_outputs(a, cout, out, split, want_stats, "conv3d_f8")
    with _span("conv_igemm_f8", a.c + b.c, cout, 3, dil, a.n, a.d, a.h, a.w, "e4m3"):
        _lib.check(_fn16("brats_conv3d_f8_fwd", a.dtype)(a.ptr, a.c, a.pitch, _vec(amax, 1, "conv3d_f8: amax", a, null=True), b.ptr, b.c,
                                                  b.pitch, _vec(amax2, 1, "conv3d_f8: amax2", a, null=True),
                                                  float(xscale) if xscale is not None else 0.0, wp,
                                                  _vec(bias, cout, "conv3d_f8: bias", a, null=True), *oargs, dil, a.n, a.d, a.h, a.w,
                                                  cout, _stream()), "conv3d_f8_fwd")
    return y, stats


def _grad_out(out, shape, device):
    """The f32 tensor a gradient kernel writes: `out` (e.g. the parameter's slice of a DDP bucket, ddp.GradientBuckets.dest)
    when it is given and fits, otherwise a fresh allocation."""
    if (out is not None and out.numel() == int(np.prod(shape)) and out.dtype == torch.float32 and out.is_contiguous()
            and out.device == device):
        return out.view(shape)
    return torch.empty(shape, dtype=torch.float32, device=device)


def _wgrad_operands(x, dy, x2, what):
    """The checked operands of a weight gradient: the layer input [x | x2] and the output gradient dy, of x's extent and dtype."""
    a, b = _conv_sources(x, x2, what)
    return a, b, _act(dy, (what, "dy"), a, anyc=True)


def conv3d_wgrad(x, dy, ksize=3, dil=1, want_dbias=False, x2=None, out=None, amax_dy=None):
    """dW [cout, cin (+cin2), k,k,k] f32 (and dbias) from the layer input [x | x2] and the output gradient dy.
    amax_dy (split precision only): 1-element f32 device tensor holding max|dy| (see conv3d's amax)."""
    a, b, g = _wgrad_operands(x, dy, x2, "conv3d_wgrad")
    n, d, h, w, c, c2, cout = a.n, a.d, a.h, a.w, a.c, b.c, g.c
    kd = _conv_dtype(a.dtype, ksize)
    if kd in (X3F, X3B) and (c % 8 or c2 % 8 or cout % 8):
        kd = a.dtype  # (narrow test widths: the 16-bit kernels behind the split form want multiples of 8 channels)
    code = _code(kd)
    nbytes = _lib.lib().brats_conv3d_wgrad_ws_bytes(code, ksize, n, d, h, w, c, c2, cout)
    ws = torch.empty(max(nbytes, 4) // 4, dtype=torch.float32, device=a.device)
    dw = _grad_out(out, (cout, c + c2, ksize, ksize, ksize), a.device)
    db = torch.empty(cout, dtype=torch.float32, device=a.device) if want_dbias else None
    dbp = db.data_ptr() if db is not None else None
    with _span("conv_wgrad", c + c2, cout, ksize, dil, n, d, h, w, str(kd)):
        if amax_dy is not None and kd in (X3F, X3B):
            _lib.check(_lib.lib().brats_conv3d_x3_wgrad(a.ptr, c, a.pitch, b.ptr, c2, b.pitch, g.ptr, g.pitch,
                                                        _vec(amax_dy, 1, "conv3d_wgrad: amax_dy", a), ws.data_ptr(), dw.data_ptr(), dbp,
                                                        code, dil, n, d, h, w, cout, _stream()), "conv3d_x3_wgrad")
        else:
            _lib.check(_lib.lib().brats_conv3d_wgrad(a.ptr, c, a.pitch, b.ptr, c2, b.pitch, g.ptr, g.pitch, ws.data_ptr(), dw.data_ptr(),
                                                     dbp, code, ksize, dil, n, d, h, w, cout, _stream()), "conv3d_wgrad")
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
    if not is16(x.dtype) or dy.dtype != x.dtype:
        raise _lib.BratsHipError("conv3d_wgrad_f8: bf16 activations only")
    a, b, g = _wgrad_operands(x, dy, x2, "conv3d_wgrad_f8")
    n, d, h, w, c, c2, cout = a.n, a.d, a.h, a.w, a.c, b.c, g.c
    nbytes = _lib.lib().brats_conv3d_wgrad_f8_ws_bytes(n, d, h, w, c, c2, cout)
    if nbytes == 0:
        raise _lib.BratsHipError(f"conv3d_wgrad_f8: not built for {c}+{c2} -> {cout} channels at {n}x{d}x{h}x{w} (use conv3d_wgrad)")
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=a.device)
    dw = _grad_out(out, (cout, c + c2, 3, 3, 3), a.device)
    with _span("conv_wgrad_f8", c + c2, cout, 3, 1, n, d, h, w, "e4m3"):
        _lib.check(_fn16("brats_conv3d_wgrad_f8", a.dtype)(a.ptr, c, a.pitch, _vec(amax, 1, "conv3d_wgrad_f8: amax", a), b.ptr, c2, b.pitch,
                                                    _vec(amax2, 1, "conv3d_wgrad_f8: amax2", a, null=b.t is None), g.ptr, g.pitch,
                                                    _vec(amax_dy, 1, "conv3d_wgrad_f8: amax_dy", a), ws.data_ptr(), dw.data_ptr(), n, d,
                                                    h, w, cout, _stream()), "conv3d_wgrad_f8")
    return dw


# ------------------------------------------------------------------------------------------ GroupNorm + act
def gn_finalize(stats, n, c, groups, voxels, gamma, beta, eps=1e-5):
    sp, tiles = _finalize_in(stats, n, c, groups, "gn_finalize")
    mean_rstd = torch.empty((n, groups, 2), dtype=torch.float32, device=stats.device)
    scale_shift = torch.empty((n, c, 2), dtype=torch.float32, device=stats.device)
    chan = torch.empty(_lib.lib().brats_gn_ws_doubles(n, c), dtype=torch.float64, device=stats.device)
    _lib.check(_lib.lib().brats_gn_finalize(sp, tiles, n, c, groups, float(voxels), eps, _vec(gamma, c, "gn_finalize: gamma", stats, null=True),
                                            _vec(beta, c, "gn_finalize: beta", stats, null=True), mean_rstd.data_ptr(),
                                            scale_shift.data_ptr(), chan.data_ptr(), _stream()), "gn_finalize")
    return mean_rstd, scale_shift


def affine_act(y, scale_shift, act="relu", out=None, slope=0.01, amax=None, slope_t=None):
    """amax: optional zero-initialised 1-element f32 tensor that receives max|out| (scale source of conv3d_f8).
    slope_t: 1-element f32 device tensor overriding ``slope`` (nn.PReLU's learnable weight, act = "leakyrelu")."""
    a = _act(y, "affine_act: y")
    o = _out(out, a.shape, a, "affine_act: out")
    _lib.check(_lib.lib().brats_affine_act_fwd(a.ptr, a.pitch, _vec(scale_shift, a.n * a.c * 2, "affine_act: scale_shift", a), o.ptr, o.pitch,
                                               a.code, ACTS[act], slope, _vec(slope_t, 1, "affine_act: slope_t", a, null=True), a.n, a.vox,
                                               a.c, _vec(amax, 1, "affine_act: amax", a, null=True), _stream()), "affine_act_fwd")
    return o.t


def _overlap(a, b):
    """Do two _Acts of one storage type share memory?  Disjoint channel slices of one buffer (same pitch) do not; views whose
    address ranges meet in any other way count as overlapping."""
    es = a.t.element_size()
    alo, blo = a.ptr, b.ptr
    ahi, bhi = (p.ptr + ((p.n * p.vox - 1) * p.pitch + p.c) * es for p in (a, b))
    if not (alo < bhi and blo < ahi):
        return False
    if a.pitch != b.pitch or (blo - alo) % es:
        return True
    d = ((blo - alo) // es) % a.pitch  # b's first channel, counted from a's, inside a voxel of the shared buffer
    return d < a.c or d + b.c > a.pitch


def _pool_fused_ok(a, act):
    """Is brats_affine_act_add_pool_fwd built for the activation a?  relu / leakyrelu, and a pooling pair per block: at most 128
    channel vectors of 16 bytes."""
    return act in ("relu", "leakyrelu") and a.c * a.t.element_size() // 16 <= 128


def affine_act_add(y, scale_shift, add, act="relu", out=None, slope=0.01, slope_t=None, pool=False, want_argmax=False):
    """out = add + act(y * scale + shift) in one pass (include/brats_hip.h: brats_affine_act_add_fwd): bit-identical to
    affine_act(y, ...) followed by an elementwise add of the two stored tensors.  add / out may be channel-slice views; out must
    not overlap y or add.
    pool=True -> (out, pooled) with pooled = maxpool2(out), written by the same pass (brats_affine_act_add_pool_fwd) where that is
    built -- relu / leakyrelu, up to 128 channel vectors -- and by maxpool2 behind the plain pass elsewhere: the same bits.
    want_argmax: out._pool_argmax = the uint8 window index of every pooled element, which maxpool2_bwd(out, ...) reads."""
    a = _act(y, "affine_act_add: y")
    b = _act(add, "affine_act_add: add", a)
    o = _out(out, a.shape, a, "affine_act_add: out")
    ss = _vec(scale_shift, a.n * a.c * 2, "affine_act_add: scale_shift", a)
    sl = _vec(slope_t, 1, "affine_act_add: slope_t", a, null=True)
    if not pool:
        if want_argmax:
            raise _lib.BratsHipError("affine_act_add: want_argmax needs pool=True")
        _lib.check(_lib.lib().brats_affine_act_add_fwd(a.ptr, a.pitch, ss, b.ptr, b.pitch, o.ptr, o.pitch, a.code, ACTS[act], slope, sl,
                                                       a.n, a.vox, a.c, _stream()), "affine_act_add_fwd")
        return o.t
    half = _even(a, "affine_act_add(pool=True)")
    for src, what in ((a, "y"), (b, "add")):
        if _overlap(o, src):
            raise _lib.BratsHipError(f"affine_act_add(pool=True): out overlaps {what}")
    if not _pool_fused_ok(a, act):
        _lib.check(_lib.lib().brats_affine_act_add_fwd(a.ptr, a.pitch, ss, b.ptr, b.pitch, o.ptr, o.pitch, a.code, ACTS[act], slope, sl,
                                                       a.n, a.vox, a.c, _stream()), "affine_act_add_fwd")
        return o.t, maxpool2(o.t, want_argmax=want_argmax)
    pooled = torch.empty(half + (a.c,), dtype=a.dtype, device=a.device)
    idx = torch.empty(half + (a.c,), dtype=torch.uint8, device=a.device) if want_argmax else None
    _lib.check(_lib.lib().brats_affine_act_add_pool_fwd(a.ptr, a.pitch, ss, b.ptr, b.pitch, o.ptr, o.pitch, pooled.data_ptr(), a.c,
                                                        idx.data_ptr() if idx is not None else None, a.code, ACTS[act], slope, sl,
                                                        a.n, a.d, a.h, a.w, a.c, _stream()), "affine_act_add_pool_fwd")
    if idx is not None:
        o.t._pool_argmax = idx
    return o.t, pooled


def grad_sum(*srcs, out=None):
    """out = srcs[0] + srcs[1] (+ srcs[2] (+ srcs[3])) on NDHWC tensors (or channel-slice views) of one shape and storage type:
    f32 accumulation in argument order, one rounding, one launch (include/brats_hip.h: brats_grad_sum) -- the gradient of a
    tensor with several readers.  More than four sources: further launches that take the running sum as their first source.
    Small f32 tensors (weight gradients) go through a [1, 1, 1, rows, C] view.  out must not overlap a source."""
    if len(srcs) < 2:
        raise _lib.BratsHipError("grad_sum: at least two sources")
    if len(srcs) > 4:
        return grad_sum(grad_sum(*srcs[:4]), *srcs[4:], out=out)
    a = _act(srcs[0], "grad_sum: source 0")
    args = [a.ptr, a.pitch]
    for s in srcs[1:]:
        b = _act(s, "grad_sum: source", a)
        args += [b.ptr, b.pitch]
    args += [None, 0] * (4 - len(srcs))
    o = _out(out, a.shape, a, "grad_sum: out")
    _lib.check(_lib.lib().brats_grad_sum(*args, len(srcs), o.ptr, o.pitch, a.code, a.n, a.vox, a.c, _stream()), "grad_sum")
    return o.t


def dropout(x, p, state, unit, out=None):
    """nn.Dropout(p) on an NDHWC activation (or, with the same arguments, on the gradient flowing back through it): x * keep /
    (1 - p) with keep a pure function of (state[0] = seed, state[1] = step counter, unit id, element index) -- brats_dropout.
    state: int64[2] DEVICE tensor.  out=x: in place."""
    a = _act(x, "dropout: x")
    o = _out(out, a.shape, a, "dropout: out")
    _lib.check(_lib.lib().brats_dropout(a.ptr, a.pitch, o.ptr, o.pitch, a.code, a.n * a.vox, a.c, float(p),
                                        _vec(state, 2, "dropout: state (seed, step counter)", a, torch.int64), int(unit), _stream()),
               "dropout")
    return o.t


def affine_act_pool(y, scale_shift, act="relu", slope=0.01, amax=None, slope_t=None, with_avg=False, want_argmax=False):
    """(z, pooled) = (affine_act(y), maxpool2(z)) in one pass (include/brats_hip.h: brats_affine_act_pool_fwd).
    want_argmax: z._pool_argmax = the uint8 window index of every pooled element, which maxpool2_bwd(z, ...) then reads
    instead of the window itself."""
    a = _act(y, "affine_act_pool: y")
    half = _even(a, "affine_act_pool")
    z = torch.empty(a.shape, dtype=a.dtype, device=a.device)
    pooled = torch.empty(half + (a.c * (2 if with_avg else 1),), dtype=a.dtype, device=a.device)
    idx = torch.empty(half + (a.c,), dtype=torch.uint8, device=a.device) if want_argmax else None
    _lib.check(_lib.lib().brats_affine_act_pool_fwd(a.ptr, a.pitch, _vec(scale_shift, a.n * a.c * 2, "affine_act_pool: scale_shift", a),
                                                    z.data_ptr(), a.c, pooled.data_ptr(), pooled.shape[-1],
                                                    idx.data_ptr() if idx is not None else None, a.code, ACTS[act], slope,
                                                    _vec(slope_t, 1, "affine_act_pool: slope_t", a, null=True), a.n, a.d, a.h, a.w, a.c,
                                                    int(with_avg), _vec(amax, 1, "affine_act_pool: amax", a, null=True), _stream()),
               "affine_act_pool_fwd")
    if idx is not None:
        z._pool_argmax = idx
    return z, pooled


def _gn_bwd_args(a, scale_shift, mean_rstd, gamma, groups, what):
    """The checked small operands every GroupNorm + activation backward reads: -> (scale_shift, mean_rstd, gamma) pointers."""
    _groups(a.c, groups, what)
    return (_vec(scale_shift, a.n * a.c * 2, (what, "scale_shift"), a), _vec(mean_rstd, a.n * groups * 2, (what, "mean_rstd"), a),
            _vec(gamma, a.c, (what, "gamma"), a, null=True))


def _norm_bwd_bufs(a, red_floats, what, out=None, chan=False):
    """What a normalisation backward of the activation a writes: (dy like a -- `out`, checked, when given --, reduction workspace,
    dgamma [C], dbeta [C], dconvbias [C] | None, the one asked for with chan (EvoNorm: the forward's per-channel sums are there))."""
    f32 = dict(dtype=torch.float32, device=a.device)
    return (_out(out, a.shape, a, (what, "out")), torch.empty(red_floats, **f32), torch.empty(a.c, **f32), torch.empty(a.c, **f32),
            torch.empty(a.c, **f32) if chan else None)


def _gn_bwd_bufs(a, what, out=None):
    return _norm_bwd_bufs(a, _lib.lib().brats_gn_bwd_ws_floats(a.n, a.c), what, out)[:4]


def gn_act_bwd(dz, y, scale_shift, mean_rstd, gamma, groups=8, act="relu", slope=0.01, amax=None, slope_t=None, out=None):
    """Returns (dy, dgamma, dbeta) for z = act(GroupNorm(y)); amax (optional, zero-initialised) receives max|dy|.
    out: the tensor dy is written to (e.g. a slice of a stacked buffer) instead of a fresh one."""
    a = _act(y, "gn_act_bwd: y")
    g = _act(dz, "gn_act_bwd: dz", a)
    ss, mr, gm = _gn_bwd_args(a, scale_shift, mean_rstd, gamma, groups, "gn_act_bwd")
    dy, red, dgamma, dbeta = _gn_bwd_bufs(a, "gn_act_bwd", out)
    _lib.check(_lib.lib().brats_gn_act_bwd(g.ptr, g.pitch, a.ptr, a.pitch, ss, mr, gm, dy.ptr, dy.pitch, red.data_ptr(), dgamma.data_ptr(),
                                           dbeta.data_ptr(), a.code, ACTS[act], slope, _vec(slope_t, 1, "gn_act_bwd: slope_t", a, null=True),
                                           a.n, a.vox, a.c, groups, _vec(amax, 1, "gn_act_bwd: amax", a, null=True), _stream()), "gn_act_bwd")
    return dy.t, dgamma, dbeta


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
    a = _act(x, "conv3d_bstats: x")
    n, d, h, w, c = a.shape
    f = _act(fwd_y, "conv3d_bstats: the forward tensor", a, shape=(n, d, h, w, cout))
    kd = _conv_dtype(a.dtype, 3)
    code = _code(kd)
    wp = _conv_packed(packed_w, code, 3, dil, c, 0, cout, "conv3d_bstats", a)
    ss = _vec(scale_shift, n * cout * 2, "conv3d_bstats: scale_shift", a)
    out = new_act(n, d, h, w, cout, a.dtype, a.device)
    stats = torch.empty((n, tiles_per_sample(d, h, w), cout, 2), dtype=torch.float32, device=a.device)
    # (a family of its own in the bench's kernel table: these launches carry a GroupNorm-backward pass in their epilogue and
    #  are not the plain implicit GEMM the roofline line is about)
    with _span("conv_igemm_bst", c, cout, 3, dil, n, d, h, w, str(kd)):
        if kd in (X3F, X3B):
            _lib.check(_lib.lib().brats_conv3d_x3_fwd_bstats(a.ptr, c, a.pitch, _vec(amax, 1, "conv3d_bstats: amax", a, null=True), wp,
                                                             out.data_ptr(), cout, f.ptr, f.pitch, ss, ACTS[act], float(slope),
                                                             stats.data_ptr(), code, dil, n, d, h, w, cout, _stream()), "conv3d_x3_fwd_bstats")
        else:
            _lib.check(_lib.lib().brats_conv3d_fwd_bstats(a.ptr, c, a.pitch, wp, out.data_ptr(), cout, f.ptr, f.pitch, ss, ACTS[act],
                                                          float(slope), stats.data_ptr(), code, dil, n, d, h, w, cout, _stream()),
                       "conv3d_fwd_bstats")
    return out, stats


def gn_act_bwd_tiles(tile_stats, dz, y, scale_shift, mean_rstd, gamma, groups=8, act="relu", slope=0.01, amax=None):
    """gn_act_bwd whose first pass was taken by conv3d_bstats (tile_stats): -> (dy, dgamma, dbeta)."""
    a = _act(y, "gn_act_bwd_tiles: y")
    g = _act(dz, "gn_act_bwd_tiles: dz", a)
    ts = _tile_stats(tile_stats, a, a.c, "gn_act_bwd_tiles: tile_stats")
    ss, mr, gm = _gn_bwd_args(a, scale_shift, mean_rstd, gamma, groups, "gn_act_bwd_tiles")
    dy, red, dgamma, dbeta = _gn_bwd_bufs(a, "gn_act_bwd_tiles")
    _lib.check(_lib.lib().brats_gn_act_bwd_tiles(ts, tile_stats.shape[1], g.ptr, g.pitch, a.ptr, a.pitch, ss, mr, gm, dy.ptr, a.c,
                                                 red.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), a.code, ACTS[act], float(slope), a.n,
                                                 a.vox, a.c, groups, _vec(amax, 1, "gn_act_bwd_tiles: amax", a, null=True), _stream()),
               "gn_act_bwd_tiles")
    return dy.t, dgamma, dbeta


def _head_bwd_in(a, head_weight, dlogits, what):
    """The checked inputs and fresh outputs of a folded head backward: -> (K, [K, C] f32 weight, f32 dlogits planes, workspace,
    dweight [K, C], dbias [K])."""
    k, hw = _head_weight(head_weight, a, what)
    dl = _planes(dlogits, (what, "dlogits"), a, (a.n, k, a.d, a.h, a.w))
    f32 = dict(dtype=torch.float32, device=a.device)
    return (k, hw, dl, torch.empty(_lib.lib().brats_gn_bwd_head_ws_floats(a.n, a.c, k), **f32), torch.empty((k, a.c), **f32),
            torch.empty(k, **f32))


def gn_act_bwd_head(dlogits, head_weight, y, scale_shift, mean_rstd, gamma, groups=8, act="relu", slope=0.01, amax=None):
    """GroupNorm + activation backward of the layer under the 1x1x1 output head, the head's backward folded in
    (include/brats_hip.h: brats_gn_act_bwd_head): -> (dy, dgamma, dbeta, dhead_weight [K,C,1,1,1], dhead_bias [K])."""
    a = _act(y, "gn_act_bwd_head: y")
    ss, mr, gm = _gn_bwd_args(a, scale_shift, mean_rstd, gamma, groups, "gn_act_bwd_head")
    dy, red, dgamma, dbeta = _gn_bwd_bufs(a, "gn_act_bwd_head")
    k, hw, dl, hws, dhw, dhb = _head_bwd_in(a, head_weight, dlogits, "gn_act_bwd_head")
    _lib.check(_lib.lib().brats_gn_act_bwd_head(dl.data_ptr(), hw.data_ptr(), k, a.ptr, a.pitch, ss, mr, gm, dy.ptr, a.c, red.data_ptr(),
                                                hws.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), dhw.data_ptr(), dhb.data_ptr(), a.code,
                                                ACTS[act], slope, a.n, a.vox, a.c, groups, _vec(amax, 1, "gn_act_bwd_head: amax", a, null=True),
                                                _stream()), "gn_act_bwd_head")
    return dy.t, dgamma, dbeta, dhw.reshape(k, a.c, 1, 1, 1), dhb


def _pool_grads(a, dskip, dpool, argmax, with_avg, what):
    """The checked gradient sources of a level-ending layer with output a: d_skip like a, d_pooled (even extents, twice the
    channels with_avg) and the uint8 arg-max plane of the pooling -> (_Act, _Act, pointer)."""
    half = _even(a, what)
    return (_act(dskip, (what, "dskip"), a), _act(dpool, (what, "dpool"), a, shape=half + (a.c * (2 if with_avg else 1),)),
            _vec(argmax, a.n * (a.vox // 8) * a.c, (what, "argmax"), a, torch.uint8))


def gn_act_bwd_pool(dskip, dpool, argmax, y, scale_shift, mean_rstd, gamma, groups=8, act="relu", slope=0.01, amax=None):
    """GroupNorm + activation backward of the layer that ends an encoder level, its output gradient dskip +
    maxpool-backward(dpool) composed inside the two passes (include/brats_hip.h: brats_gn_act_bwd_pool): -> (dy, dgamma, dbeta)."""
    a = _act(y, "gn_act_bwd_pool: y")
    s, q, ip = _pool_grads(a, dskip, dpool, argmax, False, "gn_act_bwd_pool")
    ss, mr, gm = _gn_bwd_args(a, scale_shift, mean_rstd, gamma, groups, "gn_act_bwd_pool")
    dy, red, dgamma, dbeta = _gn_bwd_bufs(a, "gn_act_bwd_pool")
    _lib.check(_lib.lib().brats_gn_act_bwd_pool(s.ptr, s.pitch, q.ptr, q.pitch, ip, a.ptr, a.pitch, ss, mr, gm, dy.ptr, a.c, red.data_ptr(),
                                                dgamma.data_ptr(), dbeta.data_ptr(), a.code, ACTS[act], slope, a.n, a.d, a.h, a.w, a.c,
                                                groups, _vec(amax, 1, "gn_act_bwd_pool: amax", a, null=True), _stream()), "gn_act_bwd_pool")
    return dy.t, dgamma, dbeta


def head_fold_ok(head_weight, act, slope_t):
    """brats_gn_act_bwd_head is built for three logit planes and relu / leakyrelu without a learnable slope."""
    return head_weight.shape[0] == 3 and act in ("relu", "leakyrelu") and slope_t is None


def prelu_slope_grad(dz, y, scale_shift):
    """d loss / d slope [1] of z = PReLU(y * scale + shift) with one shared slope (nn.PReLU()): sum dz * min(pre, 0)."""
    a = _act(y, "prelu_slope_grad: y")
    g = _act(dz, "prelu_slope_grad: dz", a)
    ws = torch.empty(_lib.lib().brats_prelu_ws_floats(a.n), dtype=torch.float32, device=a.device)
    out = torch.empty(1, dtype=torch.float32, device=a.device)
    _lib.check(_lib.lib().brats_prelu_slope_grad(g.ptr, g.pitch, a.ptr, a.pitch, _vec(scale_shift, a.n * a.c * 2, "prelu_slope_grad: scale_shift", a),
                                                 ws.data_ptr(), out.data_ptr(), a.code, a.n, a.vox, a.c, _stream()), "prelu_slope_grad")
    return out


# ------------------------------------------------------------------------------------------ pool / upsample
def _argmax_plane(idx, a, what):
    """Pointer of the uint8 window-index plane of a 2x2x2 pooling of the activation a: one byte per pooled element."""
    return _vec(idx, a.n * (a.vox // 8) * a.c, what, a, torch.uint8)


def maxpool2(x, with_avg=False, out=None, want_argmax=False):
    """want_argmax (training): x._pool_argmax = the uint8 window index of every pooled element; maxpool2_bwd(x, ...) then
    reads those bytes instead of the eight window voxels of x."""
    a = _act(x, "maxpool2: x")
    half = _even(a, "maxpool2")
    o = _out(out, half + (2 * a.c if with_avg else a.c,), a, "maxpool2: out")
    idx = torch.empty(half + (a.c,), dtype=torch.uint8, device=a.device) if want_argmax else None
    _lib.check(_lib.lib().brats_maxpool2_fwd(a.ptr, a.pitch, o.ptr, o.pitch, idx.data_ptr() if idx is not None else None, a.code, a.n, a.c,
                                             a.d, a.h, a.w, int(with_avg), _stream()), "maxpool2_fwd")
    if idx is not None:
        x._pool_argmax = idx
    return o.t


def maxpool2_bwd(x, dy, dx_skip=None, with_avg=False):
    a = _act(x, "maxpool2_bwd: x")
    g = _act(dy, "maxpool2_bwd: dy", a, shape=_even(a, "maxpool2_bwd") + (2 * a.c if with_avg else a.c,))
    s = _act2(dx_skip, "maxpool2_bwd: dx_skip", a)
    dx = torch.empty(a.shape, dtype=a.dtype, device=a.device)
    idx = getattr(x, "_pool_argmax", None)
    if idx is not None:  # recorded by affine_act_pool: the window voxels of x are not read again
        _lib.check(_lib.lib().brats_maxpool2_bwd_idx(_argmax_plane(idx, a, "maxpool2_bwd: x._pool_argmax"), g.ptr, g.pitch, s.ptr, s.pitch,
                                                     dx.data_ptr(), a.c, a.code, a.n, a.c, a.d, a.h, a.w, int(with_avg), _stream()),
                   "maxpool2_bwd_idx")
        return dx
    _lib.check(_lib.lib().brats_maxpool2_bwd(a.ptr, a.pitch, None, 0, g.ptr, g.pitch, s.ptr, s.pitch, dx.data_ptr(), a.c, a.code, a.n, a.c,
                                             a.d, a.h, a.w, int(with_avg), _stream()), "maxpool2_bwd")
    return dx


def _scaled(a, scale):
    return (a.n, a.d * scale, a.h * scale, a.w * scale, a.c)


def _coarse(g, scale, what, exc):
    """The shape of the tensor whose up-sampling by `scale` has g's shape."""
    if scale < 1 or g.d % scale or g.h % scale or g.w % scale:
        raise exc(f"{what}: the extent {(g.d, g.h, g.w)} is no multiple of the scale {scale}")
    return (g.n, g.d // scale, g.h // scale, g.w // scale, g.c)


def upsample(x, scale=2, out=None):
    a = _act(x, "upsample: x")
    o = _out(out, _scaled(a, scale), a, "upsample: out")
    _lib.check(_lib.lib().brats_upsample_fwd(a.ptr, a.pitch, o.ptr, o.pitch, a.code, a.n, a.c, a.d, a.h, a.w, scale, _stream()),
               "upsample_fwd")
    return o.t


def set_upsample_bwd_fused(mode):
    """brats_upsample_bwd_set_fused: 1 / 0 = the one-launch x2 adjoint of 16-bit tensors on / off (off: three passes through the
    workspace everywhere), -1 = default (on where it tiles).  Bit-identical results.  Returns the previous setting."""
    return _lib.lib().brats_upsample_bwd_set_fused(mode)


def upsample_bwd(dy, scale=2, add=None, out=None):
    """The adjoint of upsample; add (a tensor of the result's shape and dtype, e.g. the gradient another consumer of the same
    activation produced): the result is upsample_bwd(dy) + add, bit for bit, in the same launches (brats_upsample_bwd_add).
    out: a channel-slice view to write into instead of a new tensor."""
    g = _act(dy, "upsample_bwd: dy")
    n, d, h, w, c = shape = _coarse(g, scale, "upsample_bwd", _lib.BratsHipError)
    ws = torch.empty(_lib.lib().brats_upsample_bwd_ws_bytes(g.code, n, c, d, h, w, scale), dtype=torch.uint8, device=g.device)
    dx = _out(out, shape, g, "upsample_bwd: out", exc=ValueError)
    if add is None:
        _lib.check(_lib.lib().brats_upsample_bwd(g.ptr, g.pitch, dx.ptr, dx.pitch, ws.data_ptr(), g.code, n, c, d, h, w, scale, _stream()),
                   "upsample_bwd")
        return dx.t
    b = _act(add, "upsample_bwd: addend", g, shape=shape, exc=ValueError)
    _lib.check(_lib.lib().brats_upsample_bwd_add(g.ptr, g.pitch, b.ptr, b.pitch, dx.ptr, dx.pitch, ws.data_ptr(), g.code, n, c, d, h, w, scale,
                                                 _stream()), "upsample_bwd_add")
    return dx.t


def upsample_nearest(x, scale=2, out=None):
    """nn.Upsample(scale_factor=2) in its default mode on an NDHWC tensor: out[n][z][y][x] = x[n][z // 2][y // 2][x // 2], a copy.
    out: a channel-slice view to write into instead of a new tensor."""
    a = _act(x, "upsample_nearest: x")
    o = _out(out, _scaled(a, scale), a, "upsample_nearest: out", exc=ValueError)
    _lib.check(_lib.lib().brats_upsample_nearest_fwd(a.ptr, a.pitch, o.ptr, o.pitch, a.code, a.n, a.c, a.d, a.h, a.w, scale, _stream()),
               "upsample_nearest_fwd")
    return o.t


def upsample_nearest_bwd(dy, scale=2, add=None, out=None):
    """The adjoint of upsample_nearest: every coarse voxel = the f32 sum of its 8 children, in one launch without a workspace.
    add / out: as in upsample_bwd (the result is upsample_nearest_bwd(dy) + add, bit for bit)."""
    g = _act(dy, "upsample_nearest_bwd: dy")
    n, d, h, w, c = shape = _coarse(g, scale, "upsample_nearest_bwd", ValueError)
    dx = _out(out, shape, g, "upsample_nearest_bwd: out", exc=ValueError)
    b = _act2(add, "upsample_nearest_bwd: addend", g, shape=shape, exc=ValueError)
    _lib.check(_lib.lib().brats_upsample_nearest_bwd(g.ptr, g.pitch, b.ptr, b.pitch, dx.ptr, dx.pitch, g.code, n, c, d, h, w, scale, _stream()),
               "upsample_nearest_bwd")
    return dx.t


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
def _bias(bias, k, what, a):
    """Pointer of an optional bias parameter of k elements."""
    return _vec(bias.detach() if bias is not None else None, k, what, a, null=True)


def head(x, weight, bias, scale=1):
    """NCDHW f32 logits [N, K, D*s, H*s, W*s] = upsample_s(conv1x1(x)); weight [K, C, 1,1,1]."""
    a = _act(x, "head: x")
    n, d, h, w, c = a.shape
    k, wf = _head_weight(weight, a, "head")
    out = torch.empty((n, k, d * scale, h * scale, w * scale), dtype=torch.float32, device=a.device)
    low = torch.empty((n, k, d, h, w), dtype=torch.float32, device=a.device) if scale > 1 else None
    _lib.check(_lib.lib().brats_head_fwd(a.ptr, a.pitch, wf.data_ptr(), _bias(bias, k, "head: bias", a),
                                         low.data_ptr() if low is not None else None, out.data_ptr(), a.code, n, c, k, d, h, w, scale,
                                         _stream()), "head_fwd")
    return out


def gn_head(y, scale_shift, weight, bias, act="relu", slope=0.01):
    """NCDHW f32 logits of the output head on act(GroupNorm(y)) without storing that activation
    (include/brats_hip.h: brats_gn_head_fwd); bit-identical to head(affine_act(y, scale_shift, act), weight, bias)."""
    a = _act(y, "gn_head: y")
    k, wf = _head_weight(weight, a, "gn_head")
    out = torch.empty((a.n, k, a.d, a.h, a.w), dtype=torch.float32, device=a.device)
    _lib.check(_lib.lib().brats_gn_head_fwd(a.ptr, a.pitch, _vec(scale_shift, a.n * a.c * 2, "gn_head: scale_shift", a), ACTS[act], slope,
                                            wf.data_ptr(), _bias(bias, k, "gn_head: bias", a), out.data_ptr(), a.code, a.n, a.c, k, a.vox,
                                            _stream()), "gn_head_fwd")
    return out


def head_bwd(x, weight, dout, scale=1, want_dx=True):
    """Returns (dx | None, dweight [K,C,1,1,1], dbias [K])."""
    a = _act(x, "head_bwd: x")
    n, d, h, w, c = a.shape
    k, wf = _head_weight(weight, a, "head_bwd")
    dout = _planes(dout, "head_bwd: dout", a, (n, k, d * scale, h * scale, w * scale))
    nbytes = _lib.lib().brats_head_bwd_ws_bytes(n, c, k, d, h, w, scale)
    ws = torch.empty(max(nbytes, 4) // 4, dtype=torch.float32, device=a.device)
    dx = new_act(n, d, h, w, c, a.dtype, a.device) if want_dx else None
    dw = torch.empty((k, c), dtype=torch.float32, device=a.device)
    db = torch.empty(k, dtype=torch.float32, device=a.device)
    _lib.check(_lib.lib().brats_head_bwd(a.ptr, a.pitch, wf.data_ptr(), dout.data_ptr(), ws.data_ptr(),
                                         dx.data_ptr() if dx is not None else None, c, dw.data_ptr(), db.data_ptr(),
                                         a.code, n, c, k, d, h, w, scale, _stream()), "head_bwd")
    return dx, dw.reshape(k, c, 1, 1, 1), db


# ------------------------------------------------------------------------------------------ EvoNorm-S0 / SE helpers
def _chan_sums(chan, a, what):
    """Pointer of the f64 per-channel sums evonorm_finalize keeps for the backward (None: no convolution-bias gradient): the
    kernels read the totals [N, C, 2] at its start (csrc/norm.hip), the finaliser's workspace behind them is not touched again."""
    return _vec(chan, a.n * a.c * 2, what, a, torch.float64, null=True, at_least=True)


def evonorm_finalize(stats, n, c, groups, voxels, eps=1e-5):
    """Returns (mean_rstd [N, groups, 2], chan [N, C, 2] f64 per-channel sums kept for the backward)."""
    sp, tiles = _finalize_in(stats, n, c, groups, "evonorm_finalize")
    mean_rstd = torch.empty((n, groups, 2), dtype=torch.float32, device=stats.device)
    chan = torch.empty(_lib.lib().brats_gn_ws_doubles(n, c), dtype=torch.float64, device=stats.device)  # totals first
    _lib.check(_lib.lib().brats_evonorm_finalize(sp, tiles, n, c, groups, float(voxels), eps, mean_rstd.data_ptr(), chan.data_ptr(),
                                                 _stream()), "evonorm_finalize")
    return mean_rstd, chan


def _evo_args(a, mean_rstd, gamma, beta, groups, what):
    """The checked small operands of the EvoNorm entry points: -> (mean_rstd, gamma, beta) pointers."""
    _groups(a.c, groups, what)
    return (_vec(mean_rstd, a.n * groups * 2, (what, "mean_rstd"), a), _vec(gamma, a.c, (what, "gamma"), a, null=True),
            _vec(beta, a.c, (what, "beta"), a, null=True))


def evonorm(y, mean_rstd, gamma, beta, groups=8, out=None, want_chansum=False, amax=None):
    """z = y*sigmoid(y) * rstd_g * gamma + beta; optionally also sum_v z per (n, c) (SE's pooling)."""
    a = _act(y, "evonorm: y")
    mr, gm, bt = _evo_args(a, mean_rstd, gamma, beta, groups, "evonorm")
    o = _out(out, a.shape, a, "evonorm: out")
    cs = torch.empty(_lib.lib().brats_chan_ws_floats(a.n, a.c, 1), dtype=torch.float32, device=a.device) if want_chansum else None
    _lib.check(_lib.lib().brats_evonorm_fwd(a.ptr, a.pitch, mr, gm, bt, o.ptr, o.pitch, cs.data_ptr() if cs is not None else None, a.code,
                                            a.n, a.vox, a.c, groups, _vec(amax, 1, "evonorm: amax", a, null=True), _stream()), "evonorm_fwd")
    return o.t, (cs[:a.n * a.c].view(a.n, a.c) if cs is not None else None)


def evonorm_bwd(dz, y, mean_rstd, gamma, groups=8, chan=None, amax=None, gscale=None, gadd=None):
    """Returns (dy, dgamma, dbeta, dconvbias|None); dconvbias = sum_v dy needs the forward's `chan` sums.
    gscale / gadd ([N, C] f32): the incoming gradient is read as dz * gscale + gadd (the SE layer's backward folded in)."""
    a = _act(y, "evonorm_bwd: y")
    g = _act(dz, "evonorm_bwd: dz", a)
    mr, gm, _ = _evo_args(a, mean_rstd, gamma, None, groups, "evonorm_bwd")
    dy, red, dgamma, dbeta, dcb = _norm_bwd_bufs(a, _lib.lib().brats_chan_ws_floats(a.n, a.c, 3), "evonorm_bwd", chan=chan is not None)
    _lib.check(_lib.lib().brats_evonorm_bwd(g.ptr, g.pitch, a.ptr, a.pitch, mr, gm, dy.ptr, a.c, red.data_ptr(), dgamma.data_ptr(),
                                            dbeta.data_ptr(), _chan_sums(chan, a, "evonorm_bwd: chan"),
                                            dcb.data_ptr() if dcb is not None else None, a.code, a.n, a.vox, a.c, groups,
                                            _vec(amax, 1, "evonorm_bwd: amax", a, null=True),
                                            _vec(gscale, a.n * a.c, "evonorm_bwd: gscale", a, null=True),
                                            _vec(gadd, a.n * a.c, "evonorm_bwd: gadd", a, null=True), _stream()), "evonorm_bwd")
    return dy.t, dgamma, dbeta, dcb


def evonorm_bwd_tiles(tile_stats, dz, y, mean_rstd, gamma, beta, groups=8, chan=None, amax=None):
    """evonorm_bwd whose first pass was taken by conv3d_bstats(..., fwd_y = z, act="leakyrelu", slope=1.0) -- tile_stats = per tile
    and channel (sum dz, sum dz * z) with z the EvoNorm's stored output (include/brats_hip.h: brats_evonorm_bwd_tiles).
    -> (dy, dgamma, dbeta, dconvbias|None)."""
    a = _act(y, "evonorm_bwd_tiles: y")
    g = _act(dz, "evonorm_bwd_tiles: dz", a)
    ts = _tile_stats(tile_stats, a, a.c, "evonorm_bwd_tiles: tile_stats")
    mr, gm, bt = _evo_args(a, mean_rstd, gamma, beta, groups, "evonorm_bwd_tiles")
    dy, red, dgamma, dbeta, dcb = _norm_bwd_bufs(a, _lib.lib().brats_evonorm_bwd_tiles_ws_floats(a.n, a.c), "evonorm_bwd_tiles",
                                                 chan=chan is not None)
    _lib.check(_lib.lib().brats_evonorm_bwd_tiles(ts, tile_stats.shape[1], g.ptr, g.pitch, a.ptr, a.pitch, mr, gm, bt, dy.ptr, a.c,
                                                  red.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), _chan_sums(chan, a, "evonorm_bwd_tiles: chan"),
                                                  dcb.data_ptr() if dcb is not None else None, a.code, a.n, a.vox, a.c, groups,
                                                  _vec(amax, 1, "evonorm_bwd_tiles: amax", a, null=True), _stream()), "evonorm_bwd_tiles")
    return dy.t, dgamma, dbeta, dcb


def channel_dot(a, b=None):
    """[N, C] f32 = sum over voxels of a (* b)."""
    a = _act(a, "channel_dot: a")
    b = _act2(b, "channel_dot: b", a)
    out = torch.empty(_lib.lib().brats_chan_ws_floats(a.n, a.c, 1), dtype=torch.float32, device=a.device)
    _lib.check(_lib.lib().brats_channel_dot(a.ptr, a.pitch, b.ptr, b.pitch, out.data_ptr(), a.code, a.n, a.vox, a.c, _stream()), "channel_dot")
    return out[:a.n * a.c].view(a.n, a.c)


def channel_scale(a, scale, add=None, out=None, amax=None):
    """out[v][c] = a[v][c] * scale[n][c] (+ add[n][c])."""
    a = _act(a, "channel_scale: a")
    o = _out(out, a.shape, a, "channel_scale: out")
    _lib.check(_lib.lib().brats_channel_scale(a.ptr, a.pitch, _vec(scale, a.n * a.c, "channel_scale: scale", a),
                                              _vec(add, a.n * a.c, "channel_scale: add", a, null=True), o.ptr, o.pitch, a.code, a.n, a.vox,
                                              a.c, _vec(amax, 1, "channel_scale: amax", a, null=True), _stream()), "channel_scale")
    return o.t


def _se_in(chansum, w1, what):
    """The checked channel sums [N, C] an SE gate starts from and its hidden width: -> (n, c, ch, pointer)."""
    if not isinstance(chansum, torch.Tensor) or chansum.dim() != 2 or not isinstance(w1, torch.Tensor) or w1.dim() != 2:
        raise _lib.BratsHipError((what, "chansum must be [N, C] and w1 [C/r, C]"))
    return tuple(chansum.shape) + (w1.shape[0], _vec(chansum, None, (what, "chansum"), None))


def _se_weights(like, c, ch, what, w1, w2, b1=None, b2=None):
    """Pointers of the SE layer's parameters: w1 [ch, c], w2 [c, ch] and, where the entry point reads them, b1 [ch], b2 [c]."""
    return (_vec(w1.detach(), ch * c, (what, "w1"), like), _bias(b1, ch, (what, "b1"), like),
            _vec(w2.detach(), c * ch, (what, "w2"), like), _bias(b2, c, (what, "b2"), like))


def se_gate(chansum, voxels, w1, b1, w2, b2):
    """ResidualSELayer gate from the channel sums of z: -> (1 + gate [N, C], hidden [N, C/r]) in one launch."""
    n, c, ch, cp = _se_in(chansum, w1, "se_gate")
    if b1 is None or b2 is None:
        raise _lib.BratsHipError("se_gate: the SE layer's biases are missing")
    gate1p = torch.empty((n, c), dtype=torch.float32, device=chansum.device)
    hidden = torch.empty((n, ch), dtype=torch.float32, device=chansum.device)
    _lib.check(_lib.lib().brats_se_fwd(cp, 1.0 / float(voxels), *_se_weights(chansum, c, ch, "se_gate", w1, w2, b1, b2), gate1p.data_ptr(),
                                       hidden.data_ptr(), n, c, ch, _stream()), "se_fwd")
    return gate1p, hidden


def _se_saved(like, n, c, ch, what, hidden, gate1p):
    return _vec(hidden, n * ch, (what, "hidden"), like), _vec(gate1p, n * c, (what, "gate1p"), like)


def se_gate_bwd(dgate, chansum, voxels, hidden, gate1p, w1, w2):
    """-> (gadd [N, C] = d loss / d gap / V, dW1, db1, dW2, db2) in one launch."""
    n, c, ch, cp = _se_in(chansum, w1, "se_gate_bwd")
    f32 = dict(dtype=torch.float32, device=chansum.device)
    gadd = torch.empty((n, c), **f32)
    dw1, db1, dw2, db2 = torch.empty((ch, c), **f32), torch.empty((ch,), **f32), torch.empty((c, ch), **f32), torch.empty((c,), **f32)
    wp1, _, wp2, _ = _se_weights(chansum, c, ch, "se_gate_bwd", w1, w2)
    _lib.check(_lib.lib().brats_se_bwd(_vec(dgate, n * c, "se_gate_bwd: dgate", chansum), cp, 1.0 / float(voxels),
                                       *_se_saved(chansum, n, c, ch, "se_gate_bwd", hidden, gate1p), wp1, wp2, gadd.data_ptr(), dw1.data_ptr(),
                                       db1.data_ptr(), dw2.data_ptr(), db2.data_ptr(), n, c, ch, _stream()), "se_bwd")
    return gadd, dw1, db1, dw2, db2


def evonorm_se(y, mean_rstd, gamma, beta, w1, b1, w2, b2, groups=8, out=None, amax=None, apply=True):
    """EvoNorm + ResidualSELayer in one call, the EvoNorm output never stored (csrc/se.hpp):
    -> (out = z * (1 + gate), chansum [N, C] = sum_v z, gate1p [N, C], hidden [N, C/r]).
    apply=False: statistics pass + gate only (out = None): the consumer recomputes the output on load (evonorm_head)."""
    a = _act(y, "evonorm_se: y")
    n, c, ch = a.n, a.c, w1.shape[0]
    if b1 is None or b2 is None:
        raise _lib.BratsHipError("evonorm_se: the SE layer's biases are missing")
    mr, gm, bt = _evo_args(a, mean_rstd, gamma, beta, groups, "evonorm_se")
    o = _out(out, a.shape, a, "evonorm_se: out") if apply else _NO_ACT
    f32 = dict(dtype=torch.float32, device=a.device)
    ws = torch.empty(_lib.lib().brats_chan_ws_floats(n, c, 1), **f32)
    cs, gate1p, hidden = torch.empty((n, c), **f32), torch.empty((n, c), **f32), torch.empty((n, ch), **f32)
    _lib.check(_lib.lib().brats_evonorm_se_fwd(a.ptr, a.pitch, mr, gm, bt, *_se_weights(a, c, ch, "evonorm_se", w1, w2, b1, b2), o.ptr, o.pitch,
                                               ws.data_ptr(), cs.data_ptr(), gate1p.data_ptr(), hidden.data_ptr(), ch, a.code, n, a.vox, c,
                                               groups, _vec(amax, 1, "evonorm_se: amax", a, null=True), _stream()), "evonorm_se_fwd")
    return o.t, cs, gate1p, hidden


def evonorm_head(y, mean_rstd, gamma, beta, gate1p, weight, bias, groups=8):
    """NCDHW f32 logits of the output head on the gated EvoNorm output of y without storing it
    (include/brats_hip.h: brats_evonorm_head_fwd); bit-identical to head(evonorm_se(...)[0], weight, bias)."""
    a = _act(y, "evonorm_head: y")
    n, c = a.n, a.c
    _evo_args(a, mean_rstd, gamma, beta, groups, "evonorm_head")
    _vec(gate1p, n * c, "evonorm_head: gate1p", a)
    k, wf = _head_weight(weight, a, "evonorm_head")
    # the per-(n, channel) constants in the kernel's own order of operations: (rstd * gamma) * gate1p, beta * gate1p
    rstd = mean_rstd.view(n, groups, 2)[:, :, 1].repeat_interleave(c // groups, dim=1)
    ss = torch.stack(((rstd * gamma.float()) * gate1p.view(n, c), beta.float() * gate1p.view(n, c)), -1).contiguous()
    out = torch.empty((n, k, a.d, a.h, a.w), dtype=torch.float32, device=a.device)
    _lib.check(_lib.lib().brats_evonorm_head_fwd(a.ptr, a.pitch, ss.data_ptr(), wf.data_ptr(), _bias(bias, k, "evonorm_head: bias", a),
                                                 out.data_ptr(), a.code, n, c, k, a.vox, _stream()), "evonorm_head_fwd")
    return out


def evonorm_se_bwd(do, y, mean_rstd, gamma, beta, se_chansum, hidden, gate1p, w1, w2, groups=8, chan=None, amax=None, head=None,
                   pool=None):
    """EvoNorm backward of the layer under a ResidualSELayer with the SE backward folded in (csrc/se.hpp): `do` is the
    gradient of the SE block's OUTPUT.  -> (dy, dgamma, dbeta, dconvbias|None, dW1, db1, dW2, db2).
    head = (head_weight [K,C,1,1,1], dlogits [N,K,D,H,W]) instead of `do` (None): the block feeds only the 1x1x1 output head,
    whose backward is folded in too; two more results: dhead_weight [K,C,1,1,1], dhead_bias [K].
    pool = (d_skip, d_pooled, argmax bytes, with_avg) instead of `do` (None): the block ends an encoder level, `do` = d_skip +
    pooling-backward(d_pooled) is composed inside the passes (brats_evonorm_se_bwd_pool)."""
    a = _act(y, "evonorm_se_bwd: y")
    n, c, ch = a.n, a.c, w1.shape[0]
    mr, gm, bt = _evo_args(a, mean_rstd, gamma, beta, groups, "evonorm_se_bwd")

    def f32(*shape):
        return torch.empty(shape, dtype=torch.float32, device=a.device)

    dy, ws, dgamma, dbeta, dcb = _norm_bwd_bufs(a, _lib.lib().brats_chan_ws_floats(n, c, 5) + n * c * 3, "evonorm_se_bwd", chan=chan is not None)
    gadd, dw1, db1, dw2, db2 = f32(n, c), f32(ch, c), f32(ch), f32(c, ch), f32(c)
    wp1, _, wp2, _ = _se_weights(a, c, ch, "evonorm_se_bwd", w1, w2)
    amaxp, st = _vec(amax, 1, "evonorm_se_bwd: amax", a, null=True), _stream()
    # the arguments the two entry points share, in their order
    norm = (a.ptr, a.pitch, mr, gm, bt, dy.ptr, c, ws.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(),
            _chan_sums(chan, a, "evonorm_se_bwd: chan"), dcb.data_ptr() if dcb is not None else None,
            _vec(se_chansum, n * c, "evonorm_se_bwd: se_chansum", a), *_se_saved(a, n, c, ch, "evonorm_se_bwd", hidden, gate1p), wp1, wp2,
            gadd.data_ptr(), dw1.data_ptr(), db1.data_ptr(), dw2.data_ptr(), db2.data_ptr(), ch)
    res = (dy.t, dgamma, dbeta, dcb, dw1, db1, dw2, db2)
    if pool is not None:
        s, q, ip = _pool_grads(a, pool[0], pool[1], pool[2], pool[3], "evonorm_se_bwd(pool=)")
        _lib.check(_lib.lib().brats_evonorm_se_bwd_pool(s.ptr, s.pitch, q.ptr, q.pitch, ip, int(pool[3]), a.d, a.h, a.w, *norm, a.code, n, c,
                                                        groups, amaxp, st), "evonorm_se_bwd_pool")
        return res
    if head is None:
        g = _act(do, "evonorm_se_bwd: do", a)
        dl = hw = hws = dhw = dhb = None
        k = 0
    else:
        g = _NO_ACT
        k, hw, dl, hws, dhw, dhb = _head_bwd_in(a, head[0], head[1], "evonorm_se_bwd(head=)")
    _lib.check(_lib.lib().brats_evonorm_se_bwd(g.ptr, g.pitch, *norm, *(t.data_ptr() if t is not None else None for t in (dl, hw)), k,
                                               *(t.data_ptr() if t is not None else None for t in (hws, dhw, dhb)), a.code, n, a.vox, c,
                                               groups, amaxp, st), "evonorm_se_bwd")
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
    nbytes = _SIZES[("dconv", code, k, kdim, rows)] = _lib.lib().brats_dconv_packed_bytes(code, k, kdim, rows)
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
    if not 1 <= len(jobs) <= 4 or any(not 1 <= len(terms) <= 4 for terms, _, _ in jobs):
        raise _lib.BratsHipError("dconv_run: one to four jobs of one to four terms each")
    rec = np.zeros(len(jobs), _DCONV_JOB)
    code, first = _code(dtype), None
    for j, (terms, bias, out) in enumerate(jobs):
        o = _act(out, "dconv_run: out", first, dtype=dtype, anyc=True)
        first = first or o
        if o.shape[:4] != (n, d, h, w):
            raise _lib.BratsHipError("dconv_run: bad output tensor")
        rec[j]["nterms"], rec[j]["rows"], rec[j]["y"], rec[j]["ypitch"] = len(terms), o.c, o.ptr, o.pitch
        rec[j]["bias"] = _vec(bias, o.c, "dconv_run: bias", o, null=True) or 0
        for t, (x, wpk, ksize, dil) in enumerate(terms):
            a = _act(x, "dconv_run: input", o, anyc=True)
            wp = _packed(wpk, ("dconv", code, ksize, a.c, o.c), lambda: _lib.lib().brats_dconv_packed_bytes(code, ksize, a.c, o.c),
                         "dconv_run", o)
            rec[j]["term"][t] = (a.ptr, wp, a.pitch, a.c, ksize, dil)
    buf = rec.tobytes()
    _lib.check(_lib.lib().brats_dconv_run(buf, len(jobs), code, n, d, h, w, _stream()), "dconv_run")


def conv3d_wgrad_shift(x, dy, ksize=1, dil=1, want_dbias=False, out=None, amax_dy=None):
    """dW [cout, cin, k, k, k] f32 (and dbias) of a 1x1x1 convolution, or of a 3x3x3 convolution at any dilation
    (shifted-tap form of the weight-gradient kernel: the ASPP branches with dilation 4 / 6).  Inside a split_precision()
    block f32 tensors run the three-product form (amax_dy: the scale source of dy, see conv3d_wgrad)."""
    a, _, g = _wgrad_operands(x, dy, None, "conv3d_wgrad_shift")
    n, d, h, w, c, cout = a.n, a.d, a.h, a.w, a.c, g.c
    kd = a.dtype
    if _X3 is not None and a.dtype == torch.float32 and c % 8 == 0 and cout % 8 == 0:
        kd = _X3  # (1x1x1 too: the voxel GEMM is MFMA-bound in exact f32 -- 3.0 of EquiUnetASSPEvo-48's 44 ms x3 step)
    code = _code(kd)
    nbytes = _lib.lib().brats_conv3d_wgrad_shift_ws_bytes(code, ksize, n, d, h, w, c, cout)
    ws = torch.empty(max(nbytes, 4) // 4, dtype=torch.float32, device=a.device)
    dw = _grad_out(out, (cout, c, ksize, ksize, ksize), a.device)
    db = torch.empty(cout, dtype=torch.float32, device=a.device) if want_dbias else None
    dbp = db.data_ptr() if db is not None else None
    with _span("conv_wgrad", c, cout, ksize, dil, n, d, h, w, str(kd)):
        if amax_dy is not None and kd in (X3F, X3B):
            _lib.check(_lib.lib().brats_conv3d_x3_wgrad_shift(a.ptr, c, a.pitch, g.ptr, g.pitch, _vec(amax_dy, 1, "conv3d_wgrad_shift: amax_dy", a),
                                                              ws.data_ptr(), dw.data_ptr(), dbp, code, ksize, dil, n, d, h, w, cout, _stream()),
                       "conv3d_x3_wgrad_shift")
        else:
            _lib.check(_lib.lib().brats_conv3d_wgrad_shift(a.ptr, c, a.pitch, g.ptr, g.pitch, ws.data_ptr(), dw.data_ptr(), dbp, code, ksize, dil,
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
        if img.device != p.device:
            raise _lib.BratsHipError(f"argmax_labels: image on {img.device}, predictions on {p.device}")
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


def _cbam_params(a, w1, b1, w2, b2, wc, gamma, beta, what):
    """The checked parameters of one CBAM block over the activation a's channels: -> (their seven pointers, ch)."""
    if not isinstance(w1, torch.Tensor) or w1.dim() != 2:
        raise _lib.BratsHipError("cbam: parameter shapes do not belong to one CBAM block")
    ch, cw = w1.shape
    if cw != a.c:
        raise _lib.BratsHipError(f"{what}: the block is built for {cw} channels, the tensor has {a.c}")
    sizes = (ch * cw, ch, cw * ch, cw, 686, 1, 1)
    names = ("w1", "b1", "w2", "b2", "wc", "gamma", "beta")
    return [_vec(p.detach(), k, (what, nm), a) for p, k, nm in zip((w1, b1, w2, b2, wc, gamma, beta), sizes, names)], ch


def _cbam_storage(x, what):
    if x.dtype == torch.float16:
        raise _lib.BratsHipError((what, "fp16 storage is not built for the CBAM block (float32 or bfloat16)"))
    return _code(x.dtype)


def _cbam_saved(sv, a, ch, what, pooled=False):
    """Every field of a CbamSaved checked against the input's n, c and voxel count: -> their pointers, in __slots__ order."""
    n, c, v = a.n, a.c, a.vox
    if not isinstance(sv, CbamSaved):
        raise _lib.BratsHipError((what, "saved must come from cbam_fwd(save=True)"))
    return (_vec(sv.scale, n * c, (what, "saved.scale"), a), _vec(sv.pooled, n * 2 * c, (what, "saved.pooled"), a),
            _vec(sv.hidden, n * 2 * ch, (what, "saved.hidden"), a), _vec(sv.argvox, n * c, (what, "saved.argvox"), a, torch.int32),
            _vec(sv.comp, n * 2 * v, (what, "saved.comp"), a), _vec(sv.cidx, n * v, (what, "saved.cidx"), a, torch.int16),
            _vec(sv.z, n * v, (what, "saved.z"), a), _vec(sv.stats, n * 2, (what, "saved.stats"), a),
            _argmax_plane(sv.pidx, a, (what, "saved.pidx")) if pooled else None)


def cbam_fwd(x, w1, b1, w2, b2, wc, gamma, beta, out=None, save=True, pool=False):
    """CBAM (channel gate, then spatial gate with InstanceNorm3d(1)) on an NDHWC tensor of float32 or bfloat16 storage:
    -> (out, saved).  Three reads of x and one write of out; x * s and the spatial gate are never stored at x size.
    save=False (inference): nothing is kept, saved is None.  w1 [C/r, C], w2 [C, C/r], wc [1, 2, 7, 7, 7].
    pool=True (D, H, W even): -> (out, maxpool2(out), saved), the pooled tensor written by the last pass (brats_cbam_apply_pool);
    with save, saved.pidx holds the pooling's window-index bytes for cbam_bwd(..., d_pooled=)."""
    l = _lib.lib()
    a = _act(x, "cbam_fwd: x")
    code = _cbam_storage(x, "cbam_fwd")
    (w1, b1, w2, b2, wc, gamma, beta), ch = _cbam_params(a, w1, b1, w2, b2, wc, gamma, beta, "cbam_fwd")
    n, d, h, w, c = a.shape
    v, dev, st, xp, xpitch = a.vox, a.device, _stream(), a.ptr, a.pitch
    nb, tiles = l.brats_cbam_blocks(code, c, d, h, w), l.brats_cbam_tiles(d, h, w)
    if nb <= 0:
        _lib.check(-2, "cbam_fwd")
    f32 = dict(dtype=torch.float32, device=dev)
    o = _out(out, a.shape, a, "cbam_fwd: out")
    sv = CbamSaved()
    sv.pooled, sv.scale = torch.empty((n, 2, c), **f32), torch.empty((n, c), **f32)
    sv.hidden, sv.argvox = torch.empty((n, 2, ch), **f32), torch.empty((n, c), dtype=torch.int32, device=dev)
    sv.comp, sv.z, sv.stats = torch.empty((n, 2, v), **f32), torch.empty((n, v), **f32), torch.empty((n, 2), **f32)
    sv.cidx = torch.empty((n, v), dtype=torch.int16, device=dev) if save else None
    sv.pidx = None
    if pool:
        half = _even(a, "cbam_fwd(pool=True)")
        pooled = torch.empty(half + (c,), dtype=a.dtype, device=dev)
        if save:
            sv.pidx = torch.empty(half + (c,), dtype=torch.uint8, device=dev)
    part = torch.empty(max(3 * nb * n * c, 3 * n * tiles), **f32)
    with _span("cbam_pool", code, n, c, d, h, w):
        _lib.check(l.brats_cbam_pool(xp, xpitch, part.data_ptr(), sv.pooled.data_ptr(), sv.argvox.data_ptr(), code, n, c, d, h, w, st), "cbam_pool")
    with _span("cbam_gate", code, n, c, d, h, w):
        _lib.check(l.brats_cbam_gate(sv.pooled.data_ptr(), w1, b1, w2, b2, sv.hidden.data_ptr(), sv.scale.data_ptr(), n, c, ch, st), "cbam_gate")
    with _span("cbam_compress", code, n, c, d, h, w):
        _lib.check(l.brats_cbam_compress(xp, xpitch, sv.scale.data_ptr(), sv.comp.data_ptr(), sv.cidx.data_ptr() if save else None, code, n, c,
                                         d, h, w, st), "cbam_compress")
    with _span("cbam_spatial", code, n, c, d, h, w):
        _lib.check(l.brats_cbam_spatial(sv.comp.data_ptr(), wc, sv.z.data_ptr(), part.data_ptr(), sv.stats.data_ptr(), CBAM_EPS, n,
                                        d, h, w, st), "cbam_spatial")
    if pool:
        with _span("cbam_apply_pool", code, n, c, d, h, w):
            _lib.check(l.brats_cbam_apply_pool(xp, xpitch, sv.scale.data_ptr(), sv.z.data_ptr(), sv.stats.data_ptr(), gamma, beta, o.ptr, o.pitch,
                                               pooled.data_ptr(), c, sv.pidx.data_ptr() if save else None, code, n, c, d, h, w, st),
                       "cbam_apply_pool")
        return o.t, pooled, (sv if save else None)
    with _span("cbam_apply", code, n, c, d, h, w):
        _lib.check(l.brats_cbam_apply(xp, xpitch, sv.scale.data_ptr(), sv.z.data_ptr(), sv.stats.data_ptr(), gamma, beta, o.ptr, o.pitch, code,
                                      n, c, d, h, w, st), "cbam_apply")
    return o.t, (sv if save else None)


def cbam_bwd(dout, x, saved, w1, b1, w2, b2, wc, gamma, beta, d_pooled=None):
    """Backward of cbam_fwd: -> (dx, dW1, db1, dW2, db2, dWc, dgamma, dbeta).  Five x-sized transfers: dout and x are read for the
    gradient of the spatial gate and the sum_v dout * x * g partials, x once more for the rest of ds, and dout is read and dx
    written by the last pass (which also adds davg / V and the one-hot of the voxel arg-max; it does not need x).
    d_pooled (the block was run with pool=True, save=True): the gradient of the pooled tensor; dout is then the gradient that
    arrives at `out` directly (the skip connection) or None, and the two dout-reading passes compose dout + maxpool2_bwd(d_pooled)
    on load (brats_cbam_bwd_reduce_pool / _bwd_apply_pool) -- bit-identical to maxpool2_bwd(out, d_pooled, dx_skip=dout) first."""
    l = _lib.lib()
    a = _act(x, "cbam_bwd: x")
    code = _cbam_storage(x, "cbam_bwd")
    if dout is None and d_pooled is None:
        raise _lib.BratsHipError("cbam_bwd: no gradient given")
    if not isinstance(saved, CbamSaved) or saved.cidx is None:
        raise _lib.BratsHipError("cbam_bwd: dout must have x's shape and dtype, saved must come from cbam_fwd(save=True)")
    g = _act2(dout, "cbam_bwd: dout", a)
    if d_pooled is not None and saved.pidx is None:
        raise _lib.BratsHipError("cbam_bwd: d_pooled must have the pooled tensor's shape and x's dtype, saved must come from "
                                 "cbam_fwd(pool=True, save=True)")
    (w1, b1, w2, b2, wc, gamma, beta), ch = _cbam_params(a, w1, b1, w2, b2, wc, gamma, beta, "cbam_bwd")
    scale, pooled, hidden, argvox, comp, cidx, z, stats, pidx = _cbam_saved(saved, a, ch, "cbam_bwd", d_pooled is not None)
    src = (g.ptr, g.pitch)
    if d_pooled is not None:
        q = _act(d_pooled, "cbam_bwd: d_pooled", a, shape=_even(a, "cbam_bwd(d_pooled=)") + (a.c,))
        src += (q.ptr, q.pitch, pidx)
    n, d, h, w, c = a.shape
    v, dev, st, xp, xpitch = a.vox, a.device, _stream(), a.ptr, a.pitch
    nb, tiles = l.brats_cbam_blocks(code, c, d, h, w), l.brats_cbam_tiles(d, h, w)
    f32 = dict(dtype=torch.float32, device=dev)
    dzn, dcomp = torch.empty((n, v), **f32), torch.empty((n, 2, v), **f32)
    asum, rsum, s12 = torch.empty((n, c), **f32), torch.empty((n, c), **f32), torch.empty((n, 2), **f32)
    dpool, tmp = torch.empty((n, 2, c), **f32), torch.empty(n * c + 2 * n * ch, **f32)
    part = torch.empty(max(nb * n * (c + 2), n * tiles * 686), **f32)
    dw1, db1_, dw2, db2_ = torch.empty((ch, c), **f32), torch.empty((ch,), **f32), torch.empty((c, ch), **f32), torch.empty((c,), **f32)
    dwc, dgamma, dbeta = torch.empty((1, 2, 7, 7, 7), **f32), torch.empty((1,), **f32), torch.empty((1,), **f32)
    dx = new_act(n, d, h, w, c, a.dtype, dev)
    # (the pooled forms take (d_skip, pitch, d_pooled, pitch, window indices) where the plain ones take (dout, pitch))
    reduce, apply = ("cbam_bwd_reduce", "cbam_bwd_apply") if d_pooled is None else ("cbam_bwd_reduce_pool", "cbam_bwd_apply_pool")
    with _span(reduce, code, n, c, d, h, w):
        _lib.check(getattr(l, "brats_" + reduce)(*src, xp, xpitch, scale, z, stats, gamma, beta, dzn.data_ptr(), part.data_ptr(), asum.data_ptr(),
                                                 s12.data_ptr(), code, n, c, d, h, w, st), reduce)
    with _span("cbam_bwd_spatial", code, n, c, d, h, w):
        _lib.check(l.brats_cbam_bwd_spatial(dzn.data_ptr(), z, stats, s12.data_ptr(), gamma, comp, wc, dcomp.data_ptr(), part.data_ptr(),
                                            dwc.data_ptr(), n, d, h, w, st), "cbam_bwd_spatial")
    with _span("cbam_bwd_chan", code, n, c, d, h, w):
        _lib.check(l.brats_cbam_bwd_chan(xp, xpitch, dcomp.data_ptr(), cidx, part.data_ptr(), rsum.data_ptr(), code, n, c, d, h, w, st),
                   "cbam_bwd_chan")
    with _span("cbam_bwd_gate", code, n, c, d, h, w):
        _lib.check(l.brats_cbam_bwd_gate(asum.data_ptr(), rsum.data_ptr(), pooled, hidden, w1, b1, w2, b2, s12.data_ptr(), tmp.data_ptr(),
                                         dpool.data_ptr(), dw1.data_ptr(), db1_.data_ptr(), dw2.data_ptr(), db2_.data_ptr(), dgamma.data_ptr(),
                                         dbeta.data_ptr(), n, c, ch, st), "cbam_bwd_gate")
    with _span(apply, code, n, c, d, h, w):
        _lib.check(getattr(l, "brats_" + apply)(*src, scale, z, stats, gamma, beta, dcomp.data_ptr(), cidx, dpool.data_ptr(), argvox,
                                                dx.data_ptr(), c, code, n, c, d, h, w, st), apply)
    return dx, dw1, db1_, dw2, db2_, dwc, dgamma, dbeta


# ------------------------------------------------------------------------------------------ recurrent residual block (R2U-Net)
class RrcnnSaved:
    """What rrcnn_fwd keeps for rrcnn_bwd.  Of tensor size: per RecurrentBlock the stacked unit inputs S and raw convolution outputs
    Y, [(t + 1) N, D, H, W, C] each, and the block input(s) x (x2)."""
    __slots__ = ("x", "x2", "S", "Y", "ss", "mr", "groups", "act", "t", "n")


def _rrcnn_params(params, like):
    ps = [p.detach() for p in params]
    if len(ps) != 10:
        raise _lib.BratsHipError("rrcnn: ten parameters in the block's state-dict order (RCNN.0.conv.0.weight .. Conv_1x1.bias)")
    c = ps[8].shape[0]
    ok = (ps[8].dim() == 5 and tuple(ps[8].shape[2:]) == (1, 1, 1) and ps[9].numel() == c
          and all(tuple(ps[i].shape) == (c, c, 3, 3, 3) for i in (0, 4)) and all(ps[i].numel() == c for i in (1, 2, 3, 5, 6, 7)))
    if not ok:
        raise _lib.BratsHipError("rrcnn: parameter shapes do not belong to one RRCNNblock")
    for p in ps:
        _vec(p, None, "rrcnn: parameter", like)
    return ps, c, ps[8].shape[1]


def _rrcnn_saved(sv, c, cin, dout):
    """Every field of an RrcnnSaved checked against the block input's n and extent, the block's c, cin and t: -> the _Act of dout."""
    if not isinstance(sv, RrcnnSaved) or not sv.S:
        raise _lib.BratsHipError("rrcnn_bwd: saved must come from rrcnn_fwd(save=True)")
    a = _act(sv.x, "rrcnn_bwd: saved.x")
    a2 = _act2(sv.x2, "rrcnn_bwd: saved.x2", a, anyc=True)
    n, t = a.n, sv.t
    if ((a.c + a2.c != cin if a2.t is not None else a.c < cin) or sv.n != n or t < 1 or c % sv.groups
            or [len(v) for v in (sv.S, sv.Y, sv.ss, sv.mr)] != [2] * 4):
        raise _lib.BratsHipError("rrcnn_bwd: saved does not belong to this block")
    g = _act(dout, "rrcnn_bwd: dout", a, shape=a.shape[:4] + (c,))
    for b in (0, 1):
        for buf in (sv.S[b], sv.Y[b]):
            _act(buf, "rrcnn_bwd: saved.S / saved.Y", a, shape=((t + 1) * n,) + a.shape[1:4] + (c,))
        if len(sv.ss[b]) != t + 1 or len(sv.mr[b]) != t + 1:
            raise _lib.BratsHipError("rrcnn_bwd: saved holds other than t + 1 applications")
        for ss, mr in zip(sv.ss[b], sv.mr[b]):
            _vec(ss, n * c * 2, "rrcnn_bwd: saved.ss", a)
            _vec(mr, n * sv.groups * 2, "rrcnn_bwd: saved.mr", a)
    return g


# Size of the block output from which rrcnn_fwd(pool=True) takes the one-pass form: tensors beyond the Infinity Cache, _cgr_fwd's rule
# for affine_act_pool.  Measured at R2Unet-48's encoder shapes, bf16 (profiles/r2unet_time.json): 0.253 against 0.313 ms at
# 2 x 48 x 128^3 (403 MB); at 2 x 96 x 64^3 (101 MB) the two forms are equal within their spread and at 2 x 192 x 32^3 the pooling
# kernel re-reads the output from the cache and the two passes are faster (0.029 against 0.037 ms).  The bits are the same.
POOL_FUSED_MIN_BYTES = 256 << 20


def rrcnn_fwd(x, x2, params, groups=8, act="relu", t=2, save=True, pool=False):
    """RRCNNblock (networks/unet_family.py:60-101 of the reference) on NDHWC tensors: x0 = conv1x1([x | x2]) + bias, two
    RecurrentBlocks -- ONE conv3x3x3 (bias) -> norm -> act unit applied t + 1 times, to xb and then to xb + previous result --,
    out = x0 + result.  -> (out, saved).  params: the block's ten parameters in state-dict order; groups: 8 (GroupNorm) or C
    (InstanceNorm); x2 (or None): the second source of the 1x1x1 convolution (the virtual concat [x | x2]); x may carry zero
    channels beyond the weight's (a narrow input padded to a channel vector).
    Per application: convolution (+ tile statistics), finalize, and ONE normalise pass that writes the next unit input xb + z
    directly (affine_act_add) -- the plain affine_act only for the first block's result; the last pass of the second block adds
    x0 and writes the output.  save=True: the producers write into slices of the stacked buffers S (unit inputs: x0 is S_A[0:N],
    the first block's result S_B[0:N]) and Y (raw convolution outputs) that rrcnn_bwd reads.  save=False: nothing is kept,
    four activation buffers are reused throughout, saved is None.
    pool=True (the block ends an encoder level of R2U-Net): -> ((out, maxpool2(out)), saved); the last pass writes both
    (affine_act_add(pool=True)), with save=True also out._pool_argmax for maxpool2_bwd(out, d_pooled, dx_skip=d_skip), whose
    result is the dout of rrcnn_bwd."""
    if x3_active():
        raise NotImplementedError("rrcnn_fwd: the split-precision modes are not built for the recurrent block")
    a, a2 = _conv_sources(x, x2, "rrcnn_fwd")
    ps, c, cin = _rrcnn_params(params, a)
    if t < 1:
        raise _lib.BratsHipError(f"rrcnn_fwd: t = {t} (t >= 1)")
    if pool:
        _even(a, "rrcnn_fwd(pool=True)")
    (n, d, h, w, c1), c2 = a.shape, a2.c
    if (x2 is not None and c1 + c2 != cin) or (x2 is None and c1 < cin):
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
            elif not pool:
                out = affine_act_add(yk, scale_shift, x0, act, out=None if save else ping[1])
            elif yk.numel() * yk.element_size() >= POOL_FUSED_MIN_BYTES:
                # the block ends an encoder level: the output and its 2x2x2 max pool from one pass (save: + the arg-max bytes)
                out = affine_act_add(yk, scale_shift, x0, act, out=None if save else ping[1], pool=True, want_argmax=save)
            else:
                out = affine_act_add(yk, scale_shift, x0, act, out=None if save else ping[1])
                out = out, maxpool2(out, want_argmax=save)
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
    ps, c, cin = _rrcnn_params(params, sv.x)
    _rrcnn_saved(sv, c, cin, dout)
    n, t, x, x2 = sv.n, sv.t, sv.x, sv.x2
    dtype = x.dtype
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


# ------------------------------------------------------------------------------------------ additive attention gate
# (defined in a module of its own, which imports this one: the import stands last)
from ._attgate import AttGatePending, AttGateSaved, attgate_bwd, attgate_fwd  # noqa: E402,F401
