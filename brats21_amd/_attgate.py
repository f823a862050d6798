"""The additive attention gate of the reference's AttUnet / R2AttUnet (AttentionBlock, networks/unet_family.py:104-131) over the C
ABI of csrc/attgate.hip; re-exported by brats21_amd.ops as attgate_fwd / attgate_bwd / AttGateSaved.

    g1 = BN_g(W_g g + b_g),  x1 = BN_x(W_x x + b_x),  p = act(g1 + x1),  q = w_psi . p + b_psi,  out = x * sigmoid(BN_1(q))

The two f_int-wide 1x1x1 convolutions, their input and weight gradients are ops.conv3d / ops.conv3d_wgrad_shift; the batch
statistics of BN_g / BN_x come from the convolutions' tile statistics through ops.gn_finalize on the batch viewed as one sample.
Those kernels want a multiple of 8 output channels, so f_int is zero-padded to one where the weights are packed (zero rows, gamma =
beta = 0, zero w_psi entry: act(0) = 0 for every activation built, a padded channel contributes nothing) and the gradients are
sliced back where they leave."""
import torch

from . import _lib, ops
from ._lib import PACK_DGRAD, PACK_FWD
from ._tensors import _act, _code, _out, _vec

BN_EPS = 1e-5  # nn.BatchNorm3d's default
_NAMES = ("W_g.0.weight", "W_g.0.bias", "W_g.1.weight", "W_g.1.bias", "W_x.0.weight", "W_x.0.bias", "W_x.1.weight", "W_x.1.bias",
          "psi.0.weight", "psi.0.bias", "psi.1.weight", "psi.1.bias")
_RUNNING = ("W_g.1.running_mean", "W_g.1.running_var", "W_x.1.running_mean", "W_x.1.running_var", "psi.1.running_mean",
            "psi.1.running_var")


class AttGateSaved:
    """What attgate_fwd keeps for attgate_bwd.  Of tensor size: the inputs g and x and the raw convolution outputs g1raw / x1raw
    ([N, D, H, W, f_int padded]); q is one f32 plane of N * V voxels; the rest are [f_int]-sized tables."""
    __slots__ = ("g", "x", "g1raw", "x1raw", "q", "ss_g", "ss_x", "mr_g", "mr_x", "st1", "act", "training")


def _params(params, a_g, a_x, what):
    """The twelve parameters in state-dict order, checked at exact sizes against the channels of g and x: -> (detached list, f_int)."""
    if len(params) != 12 or not isinstance(params[0], torch.Tensor) or params[0].dim() != 5:
        raise _lib.BratsHipError(f"{what}: twelve parameters in the block's state-dict order (W_g.0.weight .. psi.1.bias)")
    fi = params[0].shape[0]
    sizes = (fi * a_g.c, fi, fi, fi, fi * a_x.c, fi, fi, fi, fi, 1, 1, 1)
    ps = [p.detach() if isinstance(p, torch.Tensor) else p for p in params]
    for p, k, nm in zip(ps, sizes, _NAMES):
        _vec(p, k, (what, nm), a_x)
    return ps, fi


def _pad(t, ci):
    """t [f_int, ...] zero-padded along its first axis to ci entries (t itself where nothing is to pad: a parameter stays the object
    the packed-weight caches know)."""
    if t.shape[0] == ci:
        return t
    out = torch.zeros((ci,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    out[:t.shape[0]] = t.detach()
    return out


def _storage(a, what):
    if ops.x3_active():
        raise NotImplementedError(f"{what}: the split-precision modes are not built for the attention gate")
    return _code(a.dtype)


def _blocks(code, c, a, what):
    nb = _lib.lib().brats_attgate_blocks(code, c, a.n, a.vox)
    if nb <= 0:
        _lib.check(nb, what)
    return nb


def _eval_tables(gamma, beta, mean, var, ci):
    """(scale_shift, mean_rstd) [1, ci, 2] of a BatchNorm in eval mode: a constant affine map from the running buffers."""
    rstd = torch.rsqrt(var.float() + BN_EPS)
    scale = gamma * rstd
    ss = torch.stack([scale, beta - mean * scale], -1)
    mr = torch.stack([mean.float(), rstd], -1)
    return _pad(ss, ci).reshape(1, ci, 2).contiguous(), _pad(mr, ci).reshape(1, ci, 2).contiguous()


def attgate_fwd(g, x, params, act="relu", training=True, out=None, save=True, running=None):
    """The attention gate on NDHWC tensors g [N, D, H, W, f_g] and x [N, D, H, W, f_l] (or channel-slice views) of float32,
    bfloat16 or float16 storage: -> (out, saved | None, stats).  params: the block's twelve parameters in state-dict order.
    training=True: batch statistics (biased variance in the normalisation); stats = ((mean, var) of BN_g, of BN_x, of BN_1) as
    device tensors -- psi's mean includes b_psi -- for the running buffers.  training=False: running = the six running_mean /
    running_var buffers in state-dict order make the three norms constant affine maps; stats is None.
    Passes: the two convolutions (+ tile statistics), their finalisers, brats_attgate_psi_fwd (reads g1raw and x1raw, writes the f32
    plane q; act(g1 + x1) is never stored), BN_1's finaliser, brats_attgate_apply_fwd (reads x and q, writes out -- into out= if
    given, leaving the neighbouring channels of a wider buffer alone).  save=False keeps nothing."""
    what = "attgate_fwd"
    a_x = _act(x, (what, "x"))
    a_g = _act(g, (what, "g"), a_x, anyc=True)
    code = _storage(a_x, what)
    ps, fi = _params(params, a_g, a_x, what)
    if act not in ops.ACTS or act == "none":
        raise _lib.BratsHipError(f"{what}: unknown activation {act!r}")
    if training:
        run = None
    else:
        if running is None or len(running) != 6:
            raise _lib.BratsHipError(f"{what}: training=False needs running = the six running_mean / running_var buffers")
        run = list(running)
        for t, k, nm in zip(run, (fi, fi, fi, fi, 1, 1), _RUNNING):
            _vec(t, k, (what, nm), a_x)
    o = _out(out, a_x.shape, a_x, (what, "out"))
    ci = (fi + 7) // 8 * 8
    n, vox, dev, l, st = a_x.n, a_x.vox, a_x.device, _lib.lib(), ops._stream
    nb = _blocks(code, ci, a_x, what)
    _blocks(code, a_x.c, a_x, what)
    count = float(n * vox)
    f32 = dict(dtype=torch.float32, device=dev)
    sv = AttGateSaved()
    sv.g, sv.x, sv.act, sv.training = g, x, act, bool(training)
    raw, tables = [], []
    for src, k in ((g, 0), (x, 4)):
        w = params[k] if fi == ci else _pad(ps[k], ci)  # (the parameter object itself where it can be: pack_weights' caches are keyed by it)
        wpk = ops.pack_weights(w, a_x.dtype, PACK_FWD)
        y, stats = ops.conv3d(src, wpk, ci, 1, 1, bias=_pad(ps[k + 1], ci), want_stats=training)
        raw.append(y)
        if training:
            mr, ss = ops.gn_finalize(stats.view(1, -1, ci, 2), 1, ci, ci, count, _pad(ps[k + 2], ci), _pad(ps[k + 3], ci), BN_EPS)
        else:
            ss, mr = _eval_tables(ps[k + 2], ps[k + 3], run[k // 2], run[k // 2 + 1], ci)
        tables.append((ss, mr))
    sv.g1raw, sv.x1raw = raw
    (sv.ss_g, sv.mr_g), (sv.ss_x, sv.mr_x) = tables
    sv.q, sv.st1 = torch.empty(n * vox, **f32), torch.empty(8, **f32)
    part = torch.empty(2 * nb, dtype=torch.float64, device=dev) if training else None
    wpsi = _pad(ps[8].reshape(fi), ci)
    with ops._span("attgate_psi_fwd", code, n, ci, vox):
        _lib.check(l.brats_attgate_psi_fwd(sv.g1raw.data_ptr(), ci, sv.x1raw.data_ptr(), ci, sv.ss_g.data_ptr(), sv.ss_x.data_ptr(),
                                           wpsi.data_ptr(), sv.q.data_ptr(), part.data_ptr() if training else None, code, ops.ACTS[act],
                                           0.01, n, vox, ci, st()), "attgate_psi_fwd")
    _lib.check(l.brats_attgate_bn1(part.data_ptr() if training else None, nb, count, ps[10].data_ptr(), ps[11].data_ptr(),
                                   ps[9].data_ptr(), run[4].data_ptr() if run else None, run[5].data_ptr() if run else None, BN_EPS,
                                   sv.st1.data_ptr(), st()), "attgate_bn1")
    with ops._span("attgate_apply_fwd", code, n, a_x.c, vox):
        _lib.check(l.brats_attgate_apply_fwd(a_x.ptr, a_x.pitch, sv.q.data_ptr(), sv.st1.data_ptr(), o.ptr, o.pitch, code, n, vox, a_x.c,
                                             st()), "attgate_apply_fwd")
    stats = None
    if training:
        def mean_var(mr):  # (the finaliser keeps rstd: var = 1 / rstd^2 - eps, _bn_fwd_tail's rule)
            return mr[0, :fi, 0], (1.0 / mr[0, :fi, 1].double() ** 2 - BN_EPS).clamp_min(0).float()
        stats = (mean_var(sv.mr_g), mean_var(sv.mr_x), (sv.st1[0:1], sv.st1[1:2]))
    return o.t, (sv if save else None), stats


def _saved(sv, params, dout, what):
    """Every field of an AttGateSaved checked against the inputs' extent and the block's f_int: -> (_Acts of x, g, dout, ps, fi, ci)."""
    if not isinstance(sv, AttGateSaved):
        raise _lib.BratsHipError(f"{what}: saved must come from attgate_fwd(save=True)")
    a_x = _act(sv.x, (what, "saved.x"))
    a_g = _act(sv.g, (what, "saved.g"), a_x, anyc=True)
    d = _act(dout, (what, "dout"), a_x)
    ps, fi = _params(params, a_g, a_x, what)
    ci = (fi + 7) // 8 * 8
    for t, nm in ((sv.g1raw, "saved.g1raw"), (sv.x1raw, "saved.x1raw")):
        r = _act(t, (what, nm), a_x, shape=a_x.shape[:4] + (ci,))
        if r.pitch != ci:
            raise _lib.BratsHipError(f"{what}: {nm} must be dense")
    _vec(sv.q, a_x.n * a_x.vox, (what, "saved.q"), a_x)
    for t, nm in ((sv.ss_g, "saved.ss_g"), (sv.ss_x, "saved.ss_x"), (sv.mr_g, "saved.mr_g"), (sv.mr_x, "saved.mr_x")):
        _vec(t, 2 * ci, (what, nm), a_x)
    _vec(sv.st1, 8, (what, "saved.st1"), a_x)
    if sv.act not in ops.ACTS:
        raise _lib.BratsHipError(f"{what}: unknown activation {sv.act!r}")
    return a_x, a_g, d, ps, fi, ci


# The fused dx + un-pooling pass (brats_attgate_dx_unpool) is taken from this many bytes of the skip tensor on; below, finish() runs
# its two parents.  0: always -- at the three sizes of DESIGN.md's table the fused pass is never slower than the pair
DX_UNPOOL_MIN_BYTES = 0


class AttGatePending:
    """The last pass of attgate_bwd, deferred (attgate_bwd(defer_dx=True) returns one in place of dx): dx = dout * alpha + t with
    alpha = sigmoid(a q + b) from the plane q [N * V] and the table st1 [8] of the forward, t = W_x^T dx1raw.  Holds dout and t (each
    of x's size) until finish()."""
    __slots__ = ("dout", "t", "q", "st1")

    def __init__(self, dout, t, q, st1):
        self.dout, self.t, self.q, self.st1 = dout, t, q, st1

    def finish(self, skip=None, d_pooled=None, out=None):
        """-> dx; with skip (the gate's input x, which a 2x2x2 max pool reads too) and d_pooled (that pool's output gradient): the
        skip tensor's whole gradient maxpool2_bwd(skip, d_pooled, dx_skip=dx).  Where skip carries a recorded arg-max plane
        (skip._pool_argmax) that is ONE pass, brats_attgate_dx_unpool, and dx is never stored; otherwise brats_attgate_dx followed
        by the pooling backward: the same bits.  out: where to write (a channel-slice view is fine; it must not overlap dout or t).
        The pending object is spent afterwards."""
        what = "attgate_bwd: finish"
        d = _act(self.dout, (what, "dout"))
        t = _act(self.t, (what, "t"), d)
        code = _storage(d, what)
        q, st1 = _vec(self.q, d.n * d.vox, (what, "q"), d), _vec(self.st1, 8, (what, "st1"), d)
        _blocks(code, d.c, d, what)
        o = _out(out, d.shape, d, (what, "out"))
        for src, nm in ((d, "dout"), (t, "t")):
            if out is not None and ops._overlap(o, src):
                raise _lib.BratsHipError(f"{what}: out overlaps {nm}")
        if (skip is None) != (d_pooled is None):
            raise _lib.BratsHipError(f"{what}: skip and d_pooled come together")
        l, st = _lib.lib(), ops._stream
        idx = None
        if skip is not None:
            a = _act(skip, (what, "skip"), d)
            g = _act(d_pooled, (what, "d_pooled"), d, shape=ops._even(d, what) + (d.c,))
            idx = getattr(skip, "_pool_argmax", None)
            if idx is not None:
                idx = ops._argmax_plane(idx, d, (what, "skip._pool_argmax"))
                if d.n > 65535:
                    raise _lib.BratsHipError(f"{what}: N = {d.n} is beyond 65535 samples")
        vw = 16 // d.t.element_size()
        for p, nm in ((d, "dout"), (t, "t"), (o, "out")) + (((g, "d_pooled"),) if skip is not None else ()):
            if p.pitch % vw or p.ptr % 16:  # (the kernels move 16-byte channel vectors)
                raise _lib.BratsHipError(f"{what}: {nm} is not made of aligned 16-byte channel vectors (pitch {p.pitch}, offset {p.ptr % 16})")
        self.dout = self.t = self.q = self.st1 = None
        if idx is not None and d.n * d.vox * d.c * d.t.element_size() >= DX_UNPOOL_MIN_BYTES:
            with ops._span("attgate_dx_unpool", code, d.n, d.c, d.vox):
                _lib.check(l.brats_attgate_dx_unpool(d.ptr, d.pitch, t.ptr, t.pitch, q, st1, idx, g.ptr, g.pitch, o.ptr, o.pitch, code, d.n,
                                                     d.c, d.d, d.h, d.w, st()), "attgate_dx_unpool")
            return o.t
        dx = o if skip is None else _out(None, d.shape, d, (what, "dx"))
        with ops._span("attgate_dx", code, d.n, d.c, d.vox):
            _lib.check(l.brats_attgate_dx(d.ptr, d.pitch, t.ptr, t.pitch, q, st1, dx.ptr, dx.pitch, code, d.n, d.vox, d.c, st()), "attgate_dx")
        if skip is None:
            return dx.t
        if out is None:
            return ops.maxpool2_bwd(skip, d_pooled, dx_skip=dx.t)
        # (ops.maxpool2_bwd's two forms, into the caller's tensor)
        if idx is not None:
            _lib.check(l.brats_maxpool2_bwd_idx(idx, g.ptr, g.pitch, dx.ptr, dx.pitch, o.ptr, o.pitch, code, d.n, d.c, d.d, d.h, d.w, 0, st()),
                       "maxpool2_bwd_idx")
        else:
            _lib.check(l.brats_maxpool2_bwd(a.ptr, a.pitch, None, 0, g.ptr, g.pitch, dx.ptr, dx.pitch, o.ptr, o.pitch, code, d.n, d.c, d.d, d.h,
                                            d.w, 0, st()), "maxpool2_bwd")
        return o.t


def attgate_bwd(dout, saved, params, need_dg=True, need_dx=True, defer_dx=False):
    """Backward of attgate_fwd: -> (dg, dx, grads) with grads the twelve parameter gradients in state-dict order, each a finished
    sum.  Passes: brats_attgate_apply_bwd (reads dout and x: the plane dqn and the sums that are psi.1's gradients and BN_1's
    backward means), brats_attgate_psi_bwd_stats (reads g1raw, x1raw and the planes, recomputes s and p: the per-channel sums that
    are the BN and psi.0 gradients and the means of BN_g / BN_x's backward), brats_attgate_psi_bwd_apply (the same reads: writes
    dg1raw and dx1raw), the 1x1x1 weight-gradient convolutions (their bias gradients: ops.channel_dot) and input-gradient convolutions, and brats_attgate_dx (dx = dout * alpha + W_x^T
    dx1raw; dout * alpha is never stored).  A forward in eval mode (frozen statistics) runs the same passes with the batch-mean terms
    off.  need_dg / need_dx = False skip that input gradient (None).  defer_dx: every pass but the last runs, and dx comes back as an
    AttGatePending whose finish() writes it -- alone, or summed with the un-pooled gradient of a pooling that read x too."""
    what = "attgate_bwd"
    sv = saved
    a_x, a_g, d, ps, fi, ci = _saved(sv, params, dout, what)
    code = _storage(a_x, what)
    n, vox, dev, l, st = a_x.n, a_x.vox, a_x.device, _lib.lib(), ops._stream
    nbx, nbi = _blocks(code, a_x.c, a_x, what), _blocks(code, ci, a_x, what)
    count, training, act = float(n * vox), int(sv.training), ops.ACTS[sv.act]
    f32 = dict(dtype=torch.float32, device=dev)
    dqn, bw1 = torch.empty(n * vox, **f32), torch.empty(4, **f32)
    part1 = torch.empty(2 * nbx, dtype=torch.float64, device=dev)
    part2, sums, coef = torch.empty(nbi * (4 * ci + 4), **f32), torch.empty(4 * ci + 1, **f32), torch.empty(3 * ci, **f32)
    dg1, dx1 = torch.empty_like(sv.g1raw), torch.empty_like(sv.x1raw)
    wpsi = _pad(ps[8].reshape(fi), ci)
    q, st1 = sv.q.data_ptr(), sv.st1.data_ptr()
    tabs = (sv.ss_g.data_ptr(), sv.ss_x.data_ptr(), sv.mr_g.data_ptr(), sv.mr_x.data_ptr(), wpsi.data_ptr(), st1, bw1.data_ptr())
    raws = (sv.g1raw.data_ptr(), ci, sv.x1raw.data_ptr(), ci, q, dqn.data_ptr())
    with ops._span("attgate_apply_bwd", code, n, a_x.c, vox):
        _lib.check(l.brats_attgate_apply_bwd(d.ptr, d.pitch, a_x.ptr, a_x.pitch, q, st1, dqn.data_ptr(), part1.data_ptr(), code, n, vox,
                                             a_x.c, st()), "attgate_apply_bwd")
    _lib.check(l.brats_attgate_bn1_bwd(part1.data_ptr(), nbx, count, training, bw1.data_ptr(), st()), "attgate_bn1_bwd")
    with ops._span("attgate_psi_bwd_stats", code, n, ci, vox):
        _lib.check(l.brats_attgate_psi_bwd_stats(*raws, *tabs, part2.data_ptr(), code, act, 0.01, n, vox, ci, st()), "attgate_psi_bwd_stats")
    _lib.check(l.brats_attgate_psi_bwd_finalize(part2.data_ptr(), nbi, ci, count, training, sums.data_ptr(), coef.data_ptr(), st()),
               "attgate_psi_bwd_finalize")
    with ops._span("attgate_psi_bwd_apply", code, n, ci, vox):
        _lib.check(l.brats_attgate_psi_bwd_apply(*raws, *tabs, coef.data_ptr(), dg1.data_ptr(), ci, dx1.data_ptr(), ci, code, act, 0.01, n,
                                                 vox, ci, st()), "attgate_psi_bwd_apply")
    grads = [None] * 12
    for src, dy, k in ((sv.g, dg1, 0), (sv.x, dx1, 4)):
        # (the bias gradient: ops.channel_dot streams dy once; the weight-gradient entry's own dbias pass is one workgroup per channel,
        #  6.5 ms of a 6.6 ms launch at 2 x 128^3 x 24 -- scripts/time_attgate.py)
        dw, _ = ops.conv3d_wgrad_shift(src, dy, 1)
        db = ops.channel_dot(dy).sum(0)
        grads[k], grads[k + 1] = (dw, db) if fi == ci else (dw[:fi].contiguous(), db[:fi].contiguous())
    grads[2], grads[3] = sums[ci:ci + fi], sums[:fi]
    grads[6], grads[7] = sums[2 * ci:2 * ci + fi], sums[:fi].clone()  # (one sum, two parameters: each gets memory of its own)
    grads[8], grads[9] = sums[3 * ci:3 * ci + fi].view(1, fi, 1, 1, 1), sums[4 * ci:4 * ci + 1]
    grads[10], grads[11] = bw1[0:1], bw1[1:2]
    dg = dx = None
    if need_dg:
        w = params[0] if fi == ci else _pad(ps[0], ci)
        dg, _ = ops.conv3d(dg1, ops.pack_weights(w, a_x.dtype, PACK_DGRAD), a_g.c, 1, 1)
    if need_dx:
        w = params[4] if fi == ci else _pad(ps[4], ci)
        t, _ = ops.conv3d(dx1, ops.pack_weights(w, a_x.dtype, PACK_DGRAD), a_x.c, 1, 1)
        dx = AttGatePending(dout, t, sv.q, sv.st1)
        if not defer_dx:
            dx = dx.finish()
    return dg, dx, grads
