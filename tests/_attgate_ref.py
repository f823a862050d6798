"""Plain-torch restatement of the reference's ``AttentionBlock`` (networks/unet_family.py:104-131) for the tests of
brats21_amd.networks.AttentionBlock, written from its formulas:

    g1 = BN_g(W_g g + b_g),  x1 = BN_x(W_x x + b_x),  s = g1 + x1,  p = act(s),  q = BN_1(w_psi . p + b_psi),  out = x * sigmoid(q)

with nn.BatchNorm3d's rules: training -- batch statistics over N, D, H, W, biased variance in the normalisation, eps 1e-5, running
buffers updated with momentum 0.1 and the UNBIASED variance, num_batches_tracked += 1; eval -- the running buffers.  ``run`` is the
forward in any dtype with gradients through autograd; ``manual_backward`` is the SCHEDULE of ops.attgate_fwd / ops.attgate_bwd
written out in float64 (recompute of s and p, the shared sum of ds, the deferred dout * alpha).  Pinned against the reference's own
class by tests/golden/make_golden_attgate.py -> tests/golden/attgate_*.npz.  Also: the cases, closed-form weights and inputs of those
fixtures, and the seeded inputs of tests/test_attgate_gpu.py, stated once."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import synth, unet

EPS, MOMENTUM = 1e-5, 0.1
# (f_g, f_l, f_int, act, (N, D, H, W)) of the two committed fixtures
CASES = [(16, 16, 8, "relu", (2, 4, 8, 8)), (8, 8, 4, "leakyrelu", (2, 8, 8, 16))]
IDS = [f"{c[0]}_{c[1]}_{c[2]}_{c[3]}" for c in CASES]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BRANCHES = ("W_g", "W_x", "psi")
PARAMS = [f"{b}.{s}" for b in BRANCHES for s in ("0.weight", "0.bias", "1.weight", "1.bias")]
BUFFERS = [f"{b}.1.{s}" for b in BRANCHES for s in ("running_mean", "running_var", "num_batches_tracked")]
KEYS = [f"{b}.{s}" for b in BRANCHES for s in ("0.weight", "0.bias", "1.weight", "1.bias", "1.running_mean", "1.running_var",
                                               "1.num_batches_tracked")]
# the convolution biases in front of a training-mode BatchNorm: their gradients are zero in exact arithmetic, and are held
# absolutely, against the maximum of the matching BatchNorm-bias gradient
DEAD = {"W_g.0.bias": "W_g.1.bias", "W_x.0.bias": "W_x.1.bias", "psi.0.bias": "psi.1.bias"}


def fname(case):
    return f"attgate_{case[0]}_{case[1]}_{case[2]}_{case[3]}.npz"


def golden(case):
    """(npz, metadata) of a committed fixture."""
    z = np.load(os.path.join(GOLDEN, fname(case)), allow_pickle=False)
    return z, json.loads(str(z["meta"]))


def shapes_of(f_g, f_l, f_int):
    """Ordered {key: shape} of the block's state dict."""
    out = {}
    for b, cin, cout in (("W_g", f_g, f_int), ("W_x", f_l, f_int), ("psi", f_int, 1)):
        out[f"{b}.0.weight"], out[f"{b}.0.bias"] = (cout, cin, 1, 1, 1), (cout,)
        for s in ("weight", "bias", "running_mean", "running_var"):
            out[f"{b}.1.{s}"] = (cout,)
        out[f"{b}.1.num_batches_tracked"] = ()
    return out


def weights(shapes):
    """Closed-form float32 values (oracle.synth.closed_form): convolution weights of magnitude sqrt(2 / fan_in) * 1.2, BatchNorm
    scales 1 +- 0.15, biases +- 0.08, running means +- 0.05, running variances 1 +- 0.2, no batch tracked yet."""
    sd = {}
    for k, shp in shapes.items():
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.tensor(0, dtype=torch.long)
        elif k.endswith("running_var"):
            sd[k] = synth.closed_form(k, shp, 0.2, 1.0)
        elif k.endswith("running_mean"):
            sd[k] = synth.closed_form(k, shp, 0.05, 0.0)
        elif k.endswith(".bias"):
            sd[k] = synth.closed_form(k, shp, 0.08, 0.0)
        elif len(shp) == 1:
            sd[k] = synth.closed_form(k, shp, 0.15, 1.0)
        else:
            sd[k] = synth.closed_form(k, shp, float(np.sqrt(2.0 / int(np.prod(shp[1:])))) * 1.2, 0.0)
    return sd


def fixture_inputs(case):
    """(state dict, g, x, dout) of a fixture: seeded CPU normals for the inputs, a closed-form upstream gradient."""
    f_g, f_l, f_int, _, (n, d, h, w) = case
    gen = torch.Generator().manual_seed(11)
    g = torch.randn(n, f_g, d, h, w, generator=gen)
    x = torch.randn(n, f_l, d, h, w, generator=gen)
    dout = synth.closed_form("attgate.dout", (n, f_l, d, h, w), 0.6, 0.0, freq=0.9173)
    return weights(shapes_of(f_g, f_l, f_int)), g, x, dout


# ------------------------------------------------------------------------------------------ the block
def _bn(y, sd, pre, training, new):
    """nn.BatchNorm3d on y [N, C, D, H, W]; training: the updated buffers go to `new`."""
    cs = (1, -1, 1, 1, 1)
    if training:
        m = y.numel() // y.shape[1]
        mean, var = y.mean((0, 2, 3, 4)), y.var((0, 2, 3, 4), unbiased=False)
        with torch.no_grad():
            new[pre + ".running_mean"] = (1 - MOMENTUM) * sd[pre + ".running_mean"].to(y.dtype) + MOMENTUM * mean
            new[pre + ".running_var"] = (1 - MOMENTUM) * sd[pre + ".running_var"].to(y.dtype) + MOMENTUM * var * (m / (m - 1.0))
            new[pre + ".num_batches_tracked"] = sd[pre + ".num_batches_tracked"] + 1
    else:
        mean, var = sd[pre + ".running_mean"].to(y.dtype), sd[pre + ".running_var"].to(y.dtype)
    yh = (y - mean.view(cs)) / torch.sqrt(var.view(cs) + EPS)
    return yh * sd[pre + ".weight"].view(cs) + sd[pre + ".bias"].view(cs)


def forward(sd, g, x, act="relu", training=True):
    """-> (out, {buffer key: value after the call})."""
    new = {k: sd[k] for k in BUFFERS}
    g1 = _bn(F.conv3d(g, sd["W_g.0.weight"], sd["W_g.0.bias"]), sd, "W_g.1", training, new)
    x1 = _bn(F.conv3d(x, sd["W_x.0.weight"], sd["W_x.0.bias"]), sd, "W_x.1", training, new)
    p = unet._act(g1 + x1, act)
    q = _bn(F.conv3d(p, sd["psi.0.weight"], sd["psi.0.bias"]), sd, "psi.1", training, new)
    return x * torch.sigmoid(q), new


def run(sd, g, x, dout, dtype=torch.float64, act="relu", training=True, parts=None):
    """The restatement in `dtype` on the CPU, loss = (out * dout).sum(): -> {"out", "dg", "dx", "grads": {key: gradient},
    "buffers": {key: value after the step}}.  parts: the subset of ("out", "grads", "buffers") wanted (None: all); without
    "grads" no backward runs."""
    cast = {k: (v.detach().cpu().to(dtype) if v.is_floating_point() else v.detach().cpu()) for k, v in sd.items()}
    for k in PARAMS:
        cast[k].requires_grad_(True)
    g_, x_ = (t.detach().cpu().to(dtype).requires_grad_(True) for t in (g, x))
    out, new = forward(cast, g_, x_, act, training)
    res = {"out": out.detach(), "buffers": new}
    if parts is None or "grads" in parts:
        (out * dout.detach().cpu().to(dtype)).sum().backward()
        res.update(dg=g_.grad, dx=x_.grad, grads={k: cast[k].grad for k in PARAMS})
    return res


_RUN64 = {}


def fixture_run64(case, training=True):
    """run in float64 on a fixture's inputs, computed once per process and shared by the tests that need it (read only)."""
    if (case, training) not in _RUN64:
        sd, g, x, dout = fixture_inputs(case)
        _RUN64[(case, training)] = run(sd, g, x, dout, torch.float64, case[3], training)
    return _RUN64[(case, training)]


# ------------------------------------------------------------------------------------------ the schedule of ops.attgate_fwd / _bwd
def _act_grad(pre, act):
    if act == "relu":
        return (pre > 0).to(pre.dtype)
    if act == "leakyrelu":
        return torch.where(pre > 0, torch.ones_like(pre), torch.full_like(pre, 0.01))
    if act == "elu":
        return torch.where(pre > 0, torch.ones_like(pre), torch.exp(pre))
    sg = torch.sigmoid(pre)
    if act == "swish":
        return sg * (1 + pre * (1 - sg))
    if act == "mish":
        th = torch.tanh(F.softplus(pre))
        return th + pre * (1 - th * th) * sg
    raise ValueError(act)


def manual_backward(sd, g, x, dout, act="relu", training=True):
    """Forward and backward as ops.attgate_fwd / ops.attgate_bwd schedule them, in float64 and without autograd: kept are g, x, the raw
    convolution outputs, the plane q WITHOUT b_psi and the small tables; s, p and alpha are recomputed.  -> the dictionary of run."""
    with torch.no_grad():
        sd = {k: (v.detach().cpu().double() if v.is_floating_point() else v) for k, v in sd.items()}
        g, x, dout = (t.detach().cpu().double() for t in (g, x, dout))
        cs, axes = (1, -1, 1, 1, 1), (0, 2, 3, 4)
        m = float(x.numel() // x.shape[1])
        wg, wx, wpsi = sd["W_g.0.weight"], sd["W_x.0.weight"], sd["psi.0.weight"].reshape(-1)
        g1raw, x1raw = F.conv3d(g, wg, sd["W_g.0.bias"]), F.conv3d(x, wx, sd["W_x.0.bias"])

        def tables(y, pre):  # (mean, rstd, scale, shift)
            if training:
                mean, var = y.mean(axes), y.var(axes, unbiased=False)
            else:
                mean, var = sd[pre + ".running_mean"], sd[pre + ".running_var"]
            rstd = 1.0 / torch.sqrt(var + EPS)
            scale = sd[pre + ".weight"] * rstd
            return mean, rstd, scale, sd[pre + ".bias"] - mean * scale
        mg, rg, scg, shg = tables(g1raw, "W_g.1")
        mx, rx, scx, shx = tables(x1raw, "W_x.1")

        def s_of():
            return g1raw * scg.view(cs) + x1raw * scx.view(cs) + (shg + shx).view(cs)
        q = (unet._act(s_of(), act) * wpsi.view(cs)).sum(1)  # the plane: no b_psi
        gamma1, beta1, bpsi = sd["psi.1.weight"][0], sd["psi.1.bias"][0], sd["psi.0.bias"][0]
        if training:
            sub, var1 = q.mean(), q.var(unbiased=False)
        else:
            sub, var1 = sd["psi.1.running_mean"][0] - bpsi, sd["psi.1.running_var"][0]
        rstd1 = 1.0 / torch.sqrt(var1 + EPS)
        a1 = gamma1 * rstd1
        b1 = beta1 - sub * a1
        out = x * torch.sigmoid(a1 * q + b1).unsqueeze(1)
        # ---- backward
        alpha = torch.sigmoid(a1 * q + b1)
        qh = (q - sub) * rstd1
        dqn = (dout * x).sum(1) * alpha * (1 - alpha)
        grads = {"psi.1.weight": (dqn * qh).sum().reshape(1), "psi.1.bias": dqn.sum().reshape(1)}
        m1, m2 = (dqn.sum() / m, (dqn * qh).sum() / m) if training else (0.0, 0.0)
        dq = (a1 * (dqn - m1 - qh * m2)).unsqueeze(1)
        s = s_of()
        ds = wpsi.view(cs) * dq * _act_grad(s, act)
        gh, xh = (g1raw - mg.view(cs)) * rg.view(cs), (x1raw - mx.view(cs)) * rx.view(cs)
        sum_ds = ds.sum(axes)
        grads["W_g.1.bias"], grads["W_x.1.bias"] = sum_ds, sum_ds.clone()
        grads["W_g.1.weight"], grads["W_x.1.weight"] = (ds * gh).sum(axes), (ds * xh).sum(axes)
        grads["psi.0.weight"] = (dq * unet._act(s, act)).sum(axes).reshape(sd["psi.0.weight"].shape)
        grads["psi.0.bias"] = dq.sum().reshape(1)
        k1 = sum_ds / m if training else torch.zeros_like(sum_ds)
        kg = grads["W_g.1.weight"] / m if training else k1
        kx = grads["W_x.1.weight"] / m if training else k1
        dg1 = scg.view(cs) * (ds - k1.view(cs) - gh * kg.view(cs))
        dx1 = scx.view(cs) * (ds - k1.view(cs) - xh * kx.view(cs))
        grads["W_g.0.weight"], grads["W_g.0.bias"] = torch.nn.grad.conv3d_weight(g, wg.shape, dg1), dg1.sum(axes)
        grads["W_x.0.weight"], grads["W_x.0.bias"] = torch.nn.grad.conv3d_weight(x, wx.shape, dx1), dx1.sum(axes)
        dg = F.conv_transpose3d(dg1, wg)
        dx = dout * alpha.unsqueeze(1) + F.conv_transpose3d(dx1, wx)  # dout * alpha is formed here, never stored
        return {"out": out, "dg": dg, "dx": dx, "grads": grads}


# ------------------------------------------------------------------------------------------ the inputs of tests/test_attgate_gpu.py
# (N, f_g, f_l, f_int, D, H, W) and what each is for
SHAPES = {
    "degenerate": (1, 16, 16, 8, 1, 1, 65),     # degenerate extents, N = 1
    "odd": (2, 16, 16, 8, 9, 7, 11),            # odd everything; two unlike samples: per-sample instead of batch statistics shows
    "att2_w48": (2, 48, 48, 24, 5, 6, 7),       # the width-48 Att2 channel counts
    "unlike": (2, 24, 16, 12, 6, 5, 9),         # f_g != f_l, f_int no multiple of 8
    "narrow": (2, 8, 8, 4, 4, 4, 4),            # f_int below a channel vector
    "widest": (2, 384, 384, 192, 4, 4, 4),
    "blocks": (1, 96, 96, 48, 16, 16, 16),      # several workgroups and partials in every reduction
}
SEED_BASE = 100


def bf16_round(t):
    return t.to(torch.bfloat16).float()


def seeded(shape, seed, b_psi=None, b_g=None):
    """(state dict, g, x, dout) from one seed: kaiming-like convolution weights, BatchNorm scales near 1.3 (W_g) / 0.8 (W_x, psi),
    non-zero shifts, so that about half of the activation inputs are positive; inputs 2 * randn and dout randn, rounded to bf16 so
    that every storage type starts from the same values; the second sample of g and x is shifted and scaled against the first."""
    n, f_g, f_l, f_int, d, h, w = shape
    gen = torch.Generator().manual_seed(seed)

    def rn(*s):
        return torch.randn(*s, generator=gen)
    sd = {}
    for k, shp in shapes_of(f_g, f_l, f_int).items():
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.tensor(0, dtype=torch.long)
        elif k.endswith("running_var"):
            sd[k] = 1.0 + 0.3 * torch.rand(shp, generator=gen)
        elif k.endswith("running_mean"):
            sd[k] = 0.1 * rn(*shp)
        elif k.endswith("0.weight"):
            sd[k] = rn(*shp) * float(np.sqrt(2.0 / shp[1]))
        elif k.endswith("0.bias"):
            sd[k] = 0.2 * rn(*shp)
        elif k.endswith("1.weight"):
            sd[k] = (1.3 if k.startswith("W_g") else 0.8) + 0.1 * rn(*shp)
        else:
            sd[k] = 0.3 * rn(*shp)
    if b_psi is not None:
        sd["psi.0.bias"] = torch.full((1,), float(b_psi))
    if b_g is not None:
        sd["W_g.0.bias"] = torch.full((f_int,), float(b_g))
    g, x = 2.0 * rn(n, f_g, d, h, w), 2.0 * rn(n, f_l, d, h, w)
    if n > 1:
        g[1:] = 0.7 * g[1:] + 0.5
        x[1:] = 1.2 * x[1:] - 0.4
    return sd, bf16_round(g), bf16_round(x), bf16_round(rn(n, f_l, d, h, w))


def seed_ok(sd, g, x, dout, act, training=True):
    """The selection rule on the float64 restatement: for relu / leakyrelu no activation input within 1e-5 of the kink, and no
    parameter gradient all zero (the three convolution biases in front of a training-mode BatchNorm excepted).  -> (ok, run64)."""
    r = run(sd, g, x, dout, torch.float64, act, training)
    cast = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    new = {}
    s = (_bn(F.conv3d(g.double(), cast["W_g.0.weight"], cast["W_g.0.bias"]), cast, "W_g.1", training, new)
         + _bn(F.conv3d(x.double(), cast["W_x.0.weight"], cast["W_x.0.bias"]), cast, "W_x.1", training, new))
    if act in ("relu", "leakyrelu") and float(s.abs().min()) < 1e-5:
        return False, r
    live = [k for k in PARAMS if not (training and k in DEAD)]
    return all(float(r["grads"][k].abs().max()) > 0.0 for k in live), r


_PICKED = {}


def pick(name, act="relu", b_psi=None, b_g=None, training=True):
    """The first of SEED_BASE .. SEED_BASE + 19 that seed_ok takes: -> (sd, g, x, dout, run64), computed once per process."""
    key = (name, act, b_psi, b_g, training)
    if key not in _PICKED:
        for seed in range(SEED_BASE, SEED_BASE + 20):
            sd, g, x, dout = seeded(SHAPES[name], seed, b_psi, b_g)
            ok, r = seed_ok(sd, g, x, dout, act, training)
            if ok:
                _PICKED[key] = (sd, g, x, dout, r)
                break
        else:
            raise AssertionError(f"no seed in {SEED_BASE} .. {SEED_BASE + 19} for {key}")
    return _PICKED[key]


def build(f_g, f_l, f_int, act="relu", sd=None):
    """brats21_amd's AttentionBlock (on the CPU), `sd` loaded."""
    from brats21_amd.networks import AttentionBlock
    m = AttentionBlock(f_g, f_l, f_int, act)
    if sd is not None:
        m.load_state_dict(sd, strict=True)
    return m
