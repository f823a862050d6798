"""Bad calls are refused before anything is launched.

libbrats_hip.so takes raw pointers plus a few integers; what brats21_amd.ops does not check is read or written out of bounds
on the device.  Here the loaded library is swapped for a stand-in: an entry point without a brats_stream_t parameter (size,
_ok, chunk and setter queries: they launch nothing) is passed through, every entry point WITH one is recorded, not called, and
returns 0.  So no corrupt pointer ever reaches a kernel: a missing check shows as a recorded call and a failed assertion.

For every public wrapper the table below holds one valid call -- activations [2, 8, 8, 8, 16] bf16 (two samples: per-sample
sizes matter; 16 channels: two 16-bit vectors, eight groups of two), K = 3 logit planes, t = 1; the e4m3 weight gradient alone
at the smallest shape it is built for -- and the entry points it must record.  Then every tensor argument is corrupted, one
corruption at a time, and each must raise BratsHipError (ValueError where a check from before this file raises that) with
nothing recorded: wrong dtype (one no kernel takes; and, where a call has two or more activations, a storage dtype other than
its partners'); one sample / one channel vector fewer; small operands one element short or non-contiguous; a permuted view
(NDHWC shape, other strides); a CPU tensor; for out= a tensor of the right size and another storage dtype.

Three kinds of corruption are no corruption and are left out, each by a flag on the argument with this meaning:
  * free="sample" / "chan": the wrapper's only sized operand -- one sample (channel vector) fewer is a valid, smaller call;
  * kind "any": the wrapper converts the tensor itself (``.contiguous().float()``): any dtype and any strides are its input by
    design, only the device (and the shape, where a second operand pins it) can be wrong;
  * a one-element operand has no non-contiguous form.
"""
import inspect
import re

import pytest
import torch

from brats21_amd import _lib, ops

pytestmark = pytest.mark.gpu

N, D, C, K, G, CH = 2, 8, 16, 3, 8, 4
V = D * D * D
BF = torch.bfloat16


# ------------------------------------------------------------------------------------------ the stand-in library
def _launching():
    txt = re.sub(r"/\*.*?\*/", " ", open(_lib.HEADER_PATH).read(), flags=re.S)
    return {m.group(1) for m in re.finditer(r"(brats_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", txt) if "brats_stream_t" in m.group(2)}


class _StandIn:
    def __init__(self, real):
        self._real, self._launch, self.calls = real, _launching(), []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in self._launch:
            return fn

        def recorded(*a):
            self.calls.append(name)
            return 0
        return recorded


@pytest.fixture(scope="module")
def standin():
    real = _lib.lib()
    s = _StandIn(real)
    _lib._lib = s
    try:
        yield s
    finally:
        _lib._lib = real
        ops.invalidate_packed_weights()


def test_the_stand_in_splits_the_abi_by_the_stream_parameter():
    launch, every = _launching(), set(_lib.declared_symbols())
    assert launch < every and len(launch) > 50
    assert {"brats_conv3d_fwd", "brats_cbam_pool", "brats_staple_iterate", "brats_dconv_run"} <= launch
    assert not launch & {"brats_conv3d_chunk", "brats_conv3d_packed_bytes", "brats_gn_ws_doubles", "brats_conv3d_set_kp",
                         "brats_conv3d_set_first_min_tiles", "brats_conv3d_form_launches", "brats_conv3d_pre_ok", "brats_abi_version", "brats_last_error"}


# ------------------------------------------------------------------------------------------ arguments and their corruptions
class T:
    """One tensor argument of a valid call: kind = act | out | vec | planes | weight | packed | any."""

    def __init__(self, kind, t, free=()):
        self.kind, self.t, self.free = kind, t, (free,) if isinstance(free, str) else tuple(free)


_OTHER = {torch.float32: torch.int32, torch.float64: torch.float32, torch.uint8: torch.int8, torch.int16: torch.int32,
          torch.int32: torch.int16, torch.int64: torch.int32, torch.bfloat16: torch.float64}


def _strided(t):
    """t's shape and values, the last two axes stored the other way round."""
    return t.transpose(-1, -2).contiguous().transpose(-1, -2)


def corruptions(a, partners=False):
    t, kind = a.t, a.kind
    out = {"cpu": t.cpu()}
    if kind in ("act", "out"):
        out["dtype"] = t.double()
        if partners:  # a dtype the kernels take, but not the one of the call's other activations
            out["other_dtype"] = t.float() if t.dtype != torch.float32 else t.to(BF)
        out["permuted"] = _strided(t)
        out["sample"] = t[:1]
        out["chan"] = t[..., :t.shape[-1] - 8]
        if kind == "out":
            out["out_dtype"] = torch.empty(t.shape, dtype=torch.float32 if t.dtype != torch.float32 else BF, device=t.device)
    elif kind == "vec":
        out["dtype"] = t.to(_OTHER[t.dtype])
        out["short"] = t.flatten()[:-1]
        if t.numel() > 1:
            out["noncontiguous"] = t.flatten().repeat_interleave(2)[::2]
    elif kind == "planes":
        out["dtype"] = t.to(torch.int32)
        out["sample"] = t[:1]
    elif kind == "weight":
        out["dtype"] = t.to(torch.int32)
        out["chan"] = t[:, :t.shape[1] - 8]
    elif kind == "packed":
        out["dtype"] = t.view(torch.int8) if t.dtype == torch.uint8 else t.view(torch.int32)
        out["short"] = t[:-1]
        out["noncontiguous"] = t[::2]
    elif kind == "any":
        if "sample" not in a.free:
            out["sample"] = t[:1]
    return {k: v for k, v in out.items() if k not in a.free}


# ------------------------------------------------------------------------------------------ the table
def _act(c=C, d=D, n=N, dtype=BF):
    return torch.zeros((n, d, d, d, c), dtype=dtype, device="cuda")


def _f(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype, device="cuda")


def _table():
    """name -> (call(**tensors), {label: T}, expected entry points).  Built under the stand-in: the pack_* calls it makes
    are recorded and not run, the buffers have their sizes."""
    P = ops.PACK_FWD
    tiles = ops.tiles_per_sample(D, D, D)
    w3, w1 = _f(C, C, 3, 3, 3), _f(C, C, 1, 1, 1)
    pk3 = ops._pack_weights(w3, BF, P, None, 0, None, 1, None)
    pkf8 = ops.pack_weights_f8(w3, P)
    pkd = ops.pack_weights_direct(w3, BF, P)
    wn = _f(K, C, 3, 3, 3)
    pkn = ops.pack_weights_narrow(wn, P)
    ss, mr, gm, bt = _f(N, C, 2), _f(N, G, 2), _f(C), _f(C)
    norm = dict(scale_shift=T("vec", ss), mean_rstd=T("vec", mr), gamma=T("vec", gm))
    evo = dict(mean_rstd=T("vec", mr), gamma=T("vec", gm), beta=T("vec", bt))
    hw, dl = _f(K, C, 1, 1, 1), _f(N, K, D, D, D)
    half, idx = _act(d=D // 2), _f(N, D // 2, D // 2, D // 2, C, dtype=torch.uint8)
    chan = _f(N, C, 2, dtype=torch.float64)  # (the totals the backward kernels index; evonorm_finalize's buffer is longer)
    se = dict(w1=T("vec", _f(CH, C)), w2=T("vec", _f(C, CH)))
    seb = dict(b1=T("vec", _f(CH)), b2=T("vec", _f(C)))
    nc = T("vec", _f(N, C))
    tb = {}

    def case(name, call, expect, **args):
        tb[name] = (call, args, expect if isinstance(expect, list) else [expect])

    x = T("act", _act(), free="sample")
    x1 = T("act", _act(), free=("sample", "chan"))
    case("ncdhw_to_ndhwc", lambda x: ops.ncdhw_to_ndhwc(x, BF, 8), "brats_ncdhw_to_ndhwc", x=T("any", _f(N, 4, D, D, D), free="sample"))
    case("ndhwc_to_ncdhw", ops.ndhwc_to_ncdhw, "brats_ndhwc_to_ncdhw", x=x1)
    wany = T("any", w3, free="sample")
    case("pack_weights", lambda w: ops.pack_weights(w, BF, P), "brats_conv3d_pack_weights", w=wany)
    case("pack_weights_f8", lambda w: ops.pack_weights_f8(w, P), "brats_conv3d_f8_pack_weights", w=wany)
    case("pack_weights_direct", lambda w: ops.pack_weights_direct(w, BF, P), "brats_dconv_pack_weights", w=wany)
    case("pack_weights_narrow", lambda w: ops.pack_weights_narrow(w, P), "brats_conv3d_narrow_pack", w=T("any", wn, free="sample"))
    case("conv3d", lambda x, pw, bias, out: ops.conv3d(x, pw, C, bias=bias, out=out, want_stats=True), "brats_conv3d_fwd",
         x=T("act", _act()), pw=T("packed", pk3), bias=T("vec", _f(C)), out=T("out", _act()))
    case("Pending", lambda y, ss, pw: ops.conv3d(ops.Pending(y, ss, "relu"), pw, C), "brats_conv3d_fwd_pre",
         y=T("act", _act()), ss=T("vec", ss), pw=T("packed", pk3))
    case("conv3d_narrow", lambda x, pw, bias, add: ops.conv3d_narrow(x, pw, K, bias, add), "brats_conv3d_narrow_fwd",
         x=T("act", _act()), pw=T("packed", pkn), bias=T("vec", _f(K)), add=T("vec", dl))
    case("absmax", ops.absmax, "brats_absmax", x=x1)
    w2s = _f(C, 2 * C, 3, 3, 3)  # two sources of C channels each
    case("conv3d(x2, split)", lambda x, x2, pw: ops.conv3d(x, pw, C, x2=x2, split=8), "brats_conv3d_fwd",
         x=T("act", _act()), x2=T("act", _act()), pw=T("packed", ops._pack_weights(w2s, BF, P, None, 0, None, 1, C)))
    case("conv3d_f8(x2)", lambda x, x2, pw, amax, amax2: ops.conv3d_f8(x, pw, C, x2=x2, amax=amax, amax2=amax2), "brats_conv3d_f8_fwd",
         x=T("act", _act()), x2=T("act", _act()), pw=T("packed", ops.pack_weights_f8(w2s, P, c1=C)), amax=T("vec", _f(1)),
         amax2=T("vec", _f(1)))
    case("conv3d_f8", lambda x, pw, amax, out: ops.conv3d_f8(x, pw, C, amax=amax, out=out), "brats_conv3d_f8_fwd",
         x=T("act", _act()), pw=T("packed", pkf8), amax=T("vec", _f(1)), out=T("out", _act()))
    case("conv3d_wgrad", ops.conv3d_wgrad, "brats_conv3d_wgrad", x=x1, dy=T("act", _act(), free="chan"), x2=T("act", _act(), free="chan"))
    case("conv3d_wgrad_shift", ops.conv3d_wgrad_shift, "brats_conv3d_wgrad_shift", x=x1, dy=T("act", _act(), free="chan"))
    # (the e4m3 weight gradient is built from 96 -> 96 channels at 32^3 on: the one case above the common shape)
    x8 = _act(96, 32)
    assert ops.conv3d_wgrad_f8_ok(x8, x8)
    case("conv3d_wgrad_f8", ops.conv3d_wgrad_f8, "brats_conv3d_wgrad_f8", x=T("act", x8, free=("sample", "chan")),
         dy=T("act", x8, free="chan"), amax=T("vec", _f(1)), amax_dy=T("vec", _f(1)))
    stats = T("vec", _f(N, tiles, C, 2))
    case("gn_finalize", lambda stats, gamma, beta: ops.gn_finalize(stats, N, C, G, V, gamma, beta), "brats_gn_finalize",
         stats=stats, gamma=T("vec", gm), beta=T("vec", bt))
    case("evonorm_finalize", lambda stats: ops.evonorm_finalize(stats, N, C, G, V), "brats_evonorm_finalize", stats=stats)
    one = dict(amax=T("vec", _f(1)), slope_t=T("vec", _f(1)))
    case("affine_act", lambda y, ss, out, amax, slope_t: ops.affine_act(y, ss, "leakyrelu", out, amax=amax, slope_t=slope_t),
         "brats_affine_act_fwd", y=T("act", _act()), ss=T("vec", ss), out=T("out", _act()), **one)
    case("affine_act_add", lambda y, ss, add, out: ops.affine_act_add(y, ss, add, out=out), "brats_affine_act_add_fwd",
         y=T("act", _act()), ss=T("vec", ss), add=T("act", _act()), out=T("out", _act()))
    case("grad_sum", lambda a, b, c, out: ops.grad_sum(a, b, c, out=out), "brats_grad_sum",
         a=T("act", _act()), b=T("act", _act()), c=T("act", _act()), out=T("out", _act()))
    case("dropout", lambda x, state, out: ops.dropout(x, 0.1, state, 0, out), "brats_dropout",
         x=T("act", _act()), state=T("vec", _f(2, dtype=torch.int64)), out=T("out", _act()))
    case("affine_act_pool", lambda y, ss, amax: ops.affine_act_pool(y, ss, amax=amax, want_argmax=True), "brats_affine_act_pool_fwd",
         y=T("act", _act()), ss=T("vec", ss), amax=T("vec", _f(1)))
    case("gn_act_bwd", lambda dz, y, out, **k: ops.gn_act_bwd(dz, y, k["scale_shift"], k["mean_rstd"], k["gamma"], G, out=out),
         "brats_gn_act_bwd", dz=T("act", _act()), y=T("act", _act()), out=T("out", _act()), **norm)
    case("conv3d_bstats", lambda x, pw, fwd_y, ss: ops.conv3d_bstats(x, pw, C, 1, fwd_y, ss), "brats_conv3d_fwd_bstats",
         x=T("act", _act()), pw=T("packed", pk3), fwd_y=T("act", _act()), ss=T("vec", ss))
    case("gn_act_bwd_tiles", lambda ts, dz, y, **k: ops.gn_act_bwd_tiles(ts, dz, y, k["scale_shift"], k["mean_rstd"], k["gamma"], G),
         "brats_gn_act_bwd_tiles", ts=stats, dz=T("act", _act()), y=T("act", _act()), **norm)
    case("gn_act_bwd_head", lambda dl, hw, y, **k: ops.gn_act_bwd_head(dl, hw, y, k["scale_shift"], k["mean_rstd"], k["gamma"], G),
         "brats_gn_act_bwd_head", dl=T("planes", dl), hw=T("weight", hw), y=T("act", _act()), **norm)
    case("gn_act_bwd_pool", lambda dskip, dpool, am, y, **k: ops.gn_act_bwd_pool(dskip, dpool, am, y, k["scale_shift"], k["mean_rstd"],
                                                                                  k["gamma"], G),
         "brats_gn_act_bwd_pool", dskip=T("act", _act()), dpool=T("act", half), am=T("vec", idx), y=T("act", _act()), **norm)
    case("prelu_slope_grad", ops.prelu_slope_grad, "brats_prelu_slope_grad", dz=T("act", _act()), y=T("act", _act()), scale_shift=T("vec", ss))
    case("maxpool2", lambda x, out: ops.maxpool2(x, out=out, want_argmax=True), "brats_maxpool2_fwd", x=T("act", _act()), out=T("out", half))
    def pool_bwd_idx(x, dy, idx):
        x = x[:]  # (a view of its own to hang the recorded plane on)
        x._pool_argmax = idx
        return ops.maxpool2_bwd(x, dy)
    case("maxpool2_bwd(idx)", pool_bwd_idx, "brats_maxpool2_bwd_idx", x=T("act", _act()), dy=T("act", half), idx=T("vec", idx))
    case("maxpool2_bwd", ops.maxpool2_bwd, "brats_maxpool2_bwd", x=T("act", _act()), dy=T("act", half), dx_skip=T("act", _act()))
    case("upsample", lambda x, out: ops.upsample(x, 2, out), "brats_upsample_fwd", x=T("act", half), out=T("out", _act()))
    case("upsample_nearest", lambda x, out: ops.upsample_nearest(x, 2, out), "brats_upsample_nearest_fwd", x=T("act", half), out=T("out", _act()))
    case("upsample_bwd", lambda dy, add, out: ops.upsample_bwd(dy, 2, add, out), "brats_upsample_bwd_add",
         dy=T("act", _act()), add=T("act", half), out=T("out", half))
    case("upsample_nearest_bwd", lambda dy, add, out: ops.upsample_nearest_bwd(dy, 2, add, out), "brats_upsample_nearest_bwd",
         dy=T("act", _act()), add=T("act", half), out=T("out", half))
    pl = T("planes", dl, free="sample")
    case("planes_nearest", lambda low: ops.planes_nearest(low, 2), "brats_planes_nearest_fwd", low=pl)
    case("planes_nearest_bwd", lambda dout: ops.planes_nearest_bwd(dout, 2), "brats_planes_nearest_bwd", dout=pl)
    case("head", lambda x, w, b: ops.head(x, w, b, 2), "brats_head_fwd", x=x, w=T("weight", hw), b=T("vec", _f(K)))
    case("gn_head", ops.gn_head, "brats_gn_head_fwd", y=T("act", _act()), scale_shift=T("vec", ss), weight=T("weight", hw), bias=T("vec", _f(K)))
    case("head_bwd", ops.head_bwd, "brats_head_bwd", x=T("act", _act()), weight=T("weight", hw), dout=T("planes", dl))
    case("evonorm", lambda y, out, amax, **k: ops.evonorm(y, k["mean_rstd"], k["gamma"], k["beta"], G, out, True, amax), "brats_evonorm_fwd",
         y=T("act", _act()), out=T("out", _act()), amax=T("vec", _f(1)), **evo)
    case("evonorm_bwd", lambda dz, y, chan, gscale, gadd, **k: ops.evonorm_bwd(dz, y, k["mean_rstd"], k["gamma"], G, chan, None, gscale, gadd),
         "brats_evonorm_bwd", dz=T("act", _act()), y=T("act", _act()), chan=T("vec", chan), gscale=nc, gadd=nc,
         mean_rstd=T("vec", mr), gamma=T("vec", gm))
    case("evonorm_bwd_tiles", lambda ts, dz, y, chan, **k: ops.evonorm_bwd_tiles(ts, dz, y, k["mean_rstd"], k["gamma"], k["beta"], G, chan),
         "brats_evonorm_bwd_tiles", ts=stats, dz=T("act", _act()), y=T("act", _act()), chan=T("vec", chan), **evo)
    case("channel_dot", ops.channel_dot, "brats_channel_dot", a=T("act", _act()), b=T("act", _act()))
    case("channel_scale", ops.channel_scale, "brats_channel_scale", a=T("act", _act()), scale=nc, add=nc, out=T("out", _act()), amax=T("vec", _f(1)))
    case("se_gate", lambda cs, **k: ops.se_gate(cs, V, k["w1"], k["b1"], k["w2"], k["b2"]), "brats_se_fwd", cs=nc, **se, **seb)
    case("se_gate_bwd", lambda dgate, cs, hidden, gate1p, **k: ops.se_gate_bwd(dgate, cs, V, hidden, gate1p, k["w1"], k["w2"]), "brats_se_bwd",
         dgate=nc, cs=nc, hidden=T("vec", _f(N, CH)), gate1p=nc, **se)
    case("evonorm_se", lambda y, out, **k: ops.evonorm_se(y, k["mean_rstd"], k["gamma"], k["beta"], k["w1"], k["b1"], k["w2"], k["b2"], G, out),
         "brats_evonorm_se_fwd", y=T("act", _act()), out=T("out", _act()), **evo, **se, **seb)
    case("evonorm_head", lambda y, gate1p, weight, bias, **k: ops.evonorm_head(y, k["mean_rstd"], k["gamma"], k["beta"], gate1p, weight, bias, G),
         "brats_evonorm_head_fwd", y=T("act", _act()), gate1p=nc, weight=T("weight", hw), bias=T("vec", _f(K)), **evo)
    sebwd = dict(y=T("act", _act()), cs=nc, hidden=T("vec", _f(N, CH)), gate1p=nc, chan=T("vec", chan), **evo, **se)

    def se_bwd(do=None, head=None, pool=None, **k):
        return ops.evonorm_se_bwd(do, k["y"], k["mean_rstd"], k["gamma"], k["beta"], k["cs"], k["hidden"], k["gate1p"], k["w1"], k["w2"], G,
                                  k["chan"], head=head, pool=pool)
    case("evonorm_se_bwd", se_bwd, "brats_evonorm_se_bwd", do=T("act", _act()), **sebwd)
    case("evonorm_se_bwd(head=)", lambda hw, dl, **k: se_bwd(head=(hw, dl), **k), "brats_evonorm_se_bwd",
         hw=T("weight", hw), dl=T("planes", dl), **sebwd)
    case("evonorm_se_bwd(pool=)", lambda dskip, dpool, am, **k: se_bwd(pool=(dskip, dpool, am, False), **k), "brats_evonorm_se_bwd_pool",
         dskip=T("act", _act()), dpool=T("act", half), am=T("vec", idx), **sebwd)
    case("dconv_run", lambda x, pw, bias, out: ops.dconv_run([([(x, pw, 3, 1)], bias, out)], N, D, D, D, BF), "brats_dconv_run",
         x=T("act", _act()), pw=T("packed", pkd), bias=T("vec", _f(C)), out=T("out", _act()))
    mask = T("any", _f(N, 1, D, D, D), free="sample")
    case("distance_transform_edt", ops.distance_transform_edt, "brats_edt", mask=mask)
    case("softmax_planes", ops.softmax_planes, "brats_softmax_planes", logits=T("any", dl, free="sample"))
    case("argmax_labels", ops.argmax_labels, "brats_argmax_labels", prob_sum=T("any", dl), img=T("any", _f(N, 4, D, D, D)))
    case("staple", lambda a, b: ops.staple([a, b], max_iterations=1),
         ["brats_staple_pack", "brats_staple_pack", "brats_staple_init", "brats_staple_iterate", "brats_staple_apply"],
         a=T("any", _f(N, 1, D, D, D)), b=T("any", _f(N, 1, D, D, D)))
    case("StaplePacker", lambda m: ops.StaplePacker((N, 1, D, D, D), 2).add(m), "brats_staple_pack", m=T("any", _f(N, 1, D, D, D)))
    # CBAM: saved comes from a forward under the stand-in (right sizes, nothing run)
    cb = dict(w1=T("vec", _f(CH, C)), b1=T("vec", _f(CH)), w2=T("vec", _f(C, CH)), b2=T("vec", _f(C)), wc=T("vec", _f(1, 2, 7, 7, 7)),
              gamma=T("vec", _f(1)), beta=T("vec", _f(1)))
    cbt = [a.t for a in cb.values()]
    xf = _act(dtype=torch.float32)
    fwd = ["brats_cbam_pool", "brats_cbam_gate", "brats_cbam_compress", "brats_cbam_spatial"]
    case("cbam_fwd", lambda x, out, **k: ops.cbam_fwd(x, *k.values(), out=out, pool=True), fwd + ["brats_cbam_apply_pool"],
         x=T("act", xf), out=T("out", _act(dtype=torch.float32)), **cb)
    _, _, saved = ops.cbam_fwd(xf, *cbt, pool=True)
    fields = {f: T("vec", getattr(saved, f)) for f in ops.CbamSaved.__slots__}

    def cbam_bwd(dout, x, d_pooled, **k):
        sv = ops.CbamSaved()
        for f in ops.CbamSaved.__slots__:
            setattr(sv, f, k.pop(f))
        return ops.cbam_bwd(dout, x, sv, *k.values(), d_pooled=d_pooled)
    case("cbam_bwd", cbam_bwd, ["brats_cbam_bwd_reduce_pool", "brats_cbam_bwd_spatial", "brats_cbam_bwd_chan", "brats_cbam_bwd_gate",
                                "brats_cbam_bwd_apply_pool"],
         dout=T("act", _act(dtype=torch.float32)), x=T("act", xf), d_pooled=T("act", _act(d=D // 2, dtype=torch.float32)), **fields, **cb)
    # the recurrent block, t = 1: ten parameters in state-dict order
    rp = [_f(C, C, 3, 3, 3), _f(C), _f(C), _f(C), _f(C, C, 3, 3, 3), _f(C), _f(C), _f(C), w1, _f(C)]
    rpt = {f"p{i}": T("vec", p) for i, p in enumerate(rp)}
    unit = ["brats_conv3d_fwd", "brats_gn_finalize"]
    rfwd = (["brats_conv3d_pack_weights", "brats_conv3d_fwd"]
            + ["brats_conv3d_pack_weights"] + unit + ["brats_affine_act_add_fwd"] + unit + ["brats_affine_act_fwd"]
            + ["brats_conv3d_pack_weights"] + unit + ["brats_affine_act_add_fwd"] + unit + ["brats_affine_act_add_fwd"])
    case("rrcnn_fwd", lambda x, **k: ops.rrcnn_fwd(x, None, list(k.values()), G, "relu", 1), rfwd, x=x, **rpt)
    _, rs = ops.rrcnn_fwd(_act(), None, rp, G, "relu", 1)
    rsv = {"sx": T("act", rs.x)}
    for b in (0, 1):
        rsv.update({f"S{b}": T("act", rs.S[b]), f"Y{b}": T("act", rs.Y[b])})
        rsv.update({f"ss{b}{k}": T("vec", rs.ss[b][k]) for k in (0, 1)})
        rsv.update({f"mr{b}{k}": T("vec", rs.mr[b][k]) for k in (0, 1)})

    def rrcnn_bwd(dout, **k):
        sv = ops.RrcnnSaved()
        sv.x, sv.x2, sv.groups, sv.act, sv.t, sv.n = k["sx"], None, G, "relu", 1, N
        sv.S, sv.Y = [k["S0"], k["S1"]], [k["Y0"], k["Y1"]]
        sv.ss, sv.mr = [[k[f"ss{b}0"], k[f"ss{b}1"]] for b in (0, 1)], [[k[f"mr{b}0"], k[f"mr{b}1"]] for b in (0, 1)]
        return ops.rrcnn_bwd(dout, sv, [k[f"p{i}"] for i in range(10)])
    blk = (["brats_conv3d_pack_weights"] + ["brats_gn_act_bwd", "brats_conv3d_fwd"] * 2
           + ["brats_grad_sum", "brats_conv3d_wgrad", "brats_channel_dot"])
    case("rrcnn_bwd", rrcnn_bwd, blk + blk + ["brats_conv3d_wgrad_shift", "brats_channel_dot", "brats_conv3d_pack_weights", "brats_conv3d_fwd"],
         dout=T("act", _act()), **rsv, **rpt)
    return tb


# queries and switches: they reach no entry point that launches; the tensors of the two *_ok queries are only asked for their shape
NO_LAUNCH = {"conv3d_wgrad_f8_ok": lambda: ops.conv3d_wgrad_f8_ok(_act(), _act()),
             "head_fold_ok": lambda: ops.head_fold_ok(_f(K, C, 1, 1, 1), "relu", None)}
NO_TENSOR = {name: "takes no tensor" for name in (
    "KernelTimer", "split_precision", "x3_active", "x3_mode", "is16", "new_act", "conv_chunk", "invalidate_packed_weights", "pack_generation",
    "keep_packed", "PackPlan", "use_plan", "plan_for", "set_kp", "set_vs8", "set_first_min_tiles", "conv_form_launches", "set_x3_wgrad_fused", "split_granule", "tiles_per_sample",
    "conv_pre_ok", "set_f8_min_size", "conv_f8_chunk", "conv_bstats_ok", "set_upsample_bwd_fused", "CbamSaved", "RrcnnSaved", "probe_box")}
NAMES = ["ncdhw_to_ndhwc", "ndhwc_to_ncdhw", "pack_weights", "pack_weights_f8", "pack_weights_direct", "pack_weights_narrow", "conv3d", "Pending",
         "conv3d_narrow", "absmax", "conv3d(x2, split)", "conv3d_f8(x2)", "conv3d_f8", "conv3d_wgrad", "conv3d_wgrad_shift", "conv3d_wgrad_f8",
         "gn_finalize", "evonorm_finalize",
         "affine_act", "affine_act_add", "grad_sum", "dropout", "affine_act_pool", "gn_act_bwd", "conv3d_bstats", "gn_act_bwd_tiles",
         "gn_act_bwd_head", "gn_act_bwd_pool", "prelu_slope_grad", "maxpool2", "maxpool2_bwd(idx)", "maxpool2_bwd", "upsample",
         "upsample_nearest", "upsample_bwd",
         "upsample_nearest_bwd", "planes_nearest", "planes_nearest_bwd", "head", "gn_head", "head_bwd", "evonorm", "evonorm_bwd",
         "evonorm_bwd_tiles", "channel_dot", "channel_scale", "se_gate", "se_gate_bwd", "evonorm_se", "evonorm_head", "evonorm_se_bwd",
         "evonorm_se_bwd(head=)", "evonorm_se_bwd(pool=)", "dconv_run", "distance_transform_edt", "softmax_planes", "argmax_labels", "staple",
         "StaplePacker", "cbam_fwd", "cbam_bwd", "rrcnn_fwd", "rrcnn_bwd"]
_TABLE = {}


def _entry(name, standin):
    if not _TABLE:
        _TABLE.update(_table())
        assert sorted(_TABLE) == sorted(NAMES)
    del standin.calls[:]
    return _TABLE[name]


def test_every_public_wrapper_is_in_the_table():
    public = {n for n, f in vars(ops).items() if not n.startswith("_") and (inspect.isfunction(f) or inspect.isclass(f))
              and f.__module__ == ops.__name__}
    covered = {n.split("(")[0] for n in NAMES} | set(NO_LAUNCH) | set(NO_TENSOR)
    assert public - covered == set(), f"no entry for {sorted(public - covered)}"
    assert covered - public == set(), f"entries for names ops does not have: {sorted(covered - public)}"
    assert set(NO_TENSOR.values()) == {"takes no tensor"}


@pytest.mark.parametrize("name", sorted(NO_LAUNCH))
def test_queries_launch_nothing(name, standin):
    del standin.calls[:]
    NO_LAUNCH[name]()
    assert standin.calls == []


@pytest.mark.parametrize("name", NAMES)
def test_valid_call_is_launched_and_every_corruption_refused(name, standin):
    call, args, expect = _entry(name, standin)
    good = {k: a.t for k, a in args.items()}
    call(**good)
    assert standin.calls == expect
    bad = []
    partners = sum(a.kind in ("act", "out") for a in args.values()) >= 2
    for label, a in args.items():
        for what, t in corruptions(a, partners).items():
            del standin.calls[:]
            try:
                call(**{**good, label: t})
            except (_lib.BratsHipError, ValueError):
                if standin.calls:
                    bad.append(f"{label}/{what}: raised after {standin.calls}")
            else:
                bad.append(f"{label}/{what}: accepted, recorded {standin.calls}")
    assert not bad, f"{name}: " + "; ".join(bad)
