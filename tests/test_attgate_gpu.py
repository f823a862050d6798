"""GPU tests of brats21_amd.networks.AttentionBlock / ops.attgate_fwd / ops.attgate_bwd (csrc/attgate.hip) against the float64
restatement tests/_attgate_ref.py, which tests/test_attgate_cpu.py pins to the reference's own class.

Inputs (tests/_attgate_ref.py: seeded, pick) are 2 * randn (dout: randn) rounded to bf16, so that every storage type sees the same
numbers; BatchNorm scales near 1.3 / 0.8 and non-zero shifts leave about half of the ReLUs on.  A seed is accepted only when, on the
float64 restatement, min |s| >= 1e-5 (relu / leakyrelu: no decision within rounding) and no parameter gradient is all zero.

Bar in f32 storage (the rule of tests/test_cbam_gpu.py and tests/test_softmax_loss_gpu.py): the restatement is also run in float32 on
the CPU; per tensor -- out, dg, dx, each parameter gradient, each buffer after the step -- the GPU's max abs error against float64
over that tensor's max abs is at most max(4 x the float32 CPU error, 1e-6).  The three convolution biases ahead of a training-mode
BatchNorm have gradients that are zero in exact arithmetic: they are measured against the maximum of the matching BatchNorm-bias
gradient.  16-bit storage: finite, and mean |16-bit - f32| of out, dg and dx at most 2 x the reference's own deviation under bf16
autocast (the fixtures' ref_bf16_dev_*).  The measured errors are printed (pytest -s) and carried in the assertion messages."""
import pytest
import torch

import _attgate_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
_REF32 = {}


def module(sd, act="relu", storage=torch.float32):
    from brats21_amd.networks import AttentionBlock
    f_int, f_g = sd["W_g.0.weight"].shape[:2]
    m = AttentionBlock(f_g, sd["W_x.0.weight"].shape[1], f_int, act)
    m.load_state_dict(sd, strict=True)
    m.storage = storage
    return m.to(DEV)


def run_module(m, g, x, dout, need_dg=True):
    m.zero_grad(set_to_none=True)
    gg, xx = g.float().to(DEV).requires_grad_(need_dg), x.float().to(DEV).requires_grad_(True)
    out = m(gg, xx)
    out.backward(dout.float().to(DEV))
    torch.cuda.synchronize()
    return {"out": out.detach(), "dg": gg.grad, "dx": xx.grad, "grads": {k: p.grad for k, p in m.named_parameters()},
            "buffers": {k: v.clone() for k, v in m.named_buffers()}}


def ref32(key, sd, g, x, dout, act, training=True):
    if key not in _REF32:
        _REF32[key] = R.run(sd, g, x, dout, torch.float32, act, training)
    return _REF32[key]


def _flat(r, training, buffers):
    items = [("out", r["out"], None), ("dg", r["dg"], None), ("dx", r["dx"], None)]
    items += [(k, r["grads"][k], R.DEAD[k] if (training and k in R.DEAD) else None) for k in R.PARAMS]
    if buffers:
        items += [(k, r["buffers"][k], None) for k in R.BUFFERS if not k.endswith("tracked")]
    return items


def check(what, got, r64, r32, training=True, buffers=True, room=None):
    """The f32 bar; room: {name: extra relative room} (the fixtures held to the reference's own float32 outputs)."""
    lines, ok = [], True
    for (name, w64, dead), (_, g, _), (_, w32, _) in zip(_flat(r64, training, buffers), _flat(got, training, buffers),
                                                         _flat(r32, training, buffers)):
        assert g.dtype == torch.float32 and tuple(g.shape) == tuple(w64.shape) and bool(torch.isfinite(g).all()), name
        scale = float((r64["grads"][dead] if dead else w64).abs().max())
        ref_err = float((w32.double() - w64).abs().max()) / scale
        bar = max(4.0 * ref_err, 1e-6) + (room or {}).get(name, 0.0)
        err = float((g.cpu().double() - w64).abs().max()) / scale
        lines.append(f"{what} {name}: max err / max {err:.2e} (bar {bar:.2e}, float32 CPU {ref_err:.2e})")
        ok = ok and err <= bar
    if buffers:
        ok = ok and all(int(got["buffers"][k]) == int(r64["buffers"][k]) for k in R.BUFFERS if k.endswith("tracked"))
    print("\n" + "\n".join(lines))
    assert ok, lines


@pytest.mark.parametrize("name", list(R.SHAPES))
def test_value_gradients_and_buffers_match_float64(name):
    sd, g, x, dout, r64 = R.pick(name)
    got = run_module(module(sd), g, x, dout)
    check(f"{name} {R.SHAPES[name]}", got, r64, ref32((name, "relu"), sd, g, x, dout, "relu"))


@pytest.mark.parametrize("act", ["leakyrelu", "elu", "swish", "mish"])
def test_every_activation(act):
    sd, g, x, dout, r64 = R.pick("odd", act)
    got = run_module(module(sd, act), g, x, dout)
    check(f"odd {act}", got, r64, ref32(("odd", act), sd, g, x, dout, act))


def test_a_large_psi_bias_cancels_and_reaches_the_running_mean():
    """b_psi = 3, b_g = 2: b_psi cancels in the training-mode normalisation and must cost the variance of the plane no digits;
    psi.1.running_mean includes it (the bar on the buffers)."""
    sd, g, x, dout, r64 = R.pick("odd", b_psi=3.0, b_g=2.0)
    got = run_module(module(sd), g, x, dout)
    check("odd b_psi=3 b_g=2", got, r64, ref32(("odd", "relu", 3.0, 2.0), sd, g, x, dout, "relu"))
    assert abs(float(got["buffers"]["psi.1.running_mean"]) - 0.9 * float(sd["psi.1.running_mean"])) > 0.25  # 0.1 * (3 + mean of w . p)


@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_fixtures_match_the_reference_class(case):
    """The reference's own float32 out, dg, dx, gradients and buffers, with its own error against float64 (ref_err_*) as room."""
    z, _ = R.golden(case)
    sd, g, x, dout = R.fixture_inputs(case)
    got = run_module(module(sd, case[3]), g, x, dout)
    ref = {"out": torch.from_numpy(z["out"]).double(), "dg": torch.from_numpy(z["dg"]).double(), "dx": torch.from_numpy(z["dx"]).double(),
           "grads": {k: torch.from_numpy(z["grad:" + k]).double() for k in R.PARAMS},
           "buffers": {k: torch.from_numpy(z["buf:" + k]) for k in R.BUFFERS}}
    ref["buffers"] = {k: (v.double() if v.is_floating_point() else v) for k, v in ref["buffers"].items()}
    room = {n: float(z["ref_err_" + n]) for n in ("out", "dg", "dx")}
    room.update({k: float(z["ref_err_grad:" + k]) for k in R.PARAMS})
    room.update({k: float(z["ref_err_buf:" + k]) for k in R.BUFFERS if not k.endswith("tracked")})
    check(f"fixture {R.fname(case)}", got, ref, ref32(("fixture", case), sd, g, x, dout, case[3]), room=room)
    check(f"fixture {R.fname(case)} (float64)", got, R.fixture_run64(case), ref32(("fixture", case), sd, g, x, dout, case[3]))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_16_bit_storage_is_finite_and_deviates_like_the_reference(case, dtype):
    z, _ = R.golden(case)
    sd, g, x, dout = R.fixture_inputs(case)
    got = run_module(module(sd, case[3], dtype), g, x, dout)
    assert all(bool(torch.isfinite(got[n]).all()) for n in ("out", "dg", "dx")) and all(bool(torch.isfinite(v).all()) for v in got["grads"].values())
    lines, ok = [], True
    for n in ("out", "dg", "dx"):
        dev, ref = float((got[n].cpu() - torch.from_numpy(z[n])).abs().mean()), float(z["ref_bf16_dev_" + n])
        lines.append(f"mean |{dtype} - f32| of {n} {dev:.4e}; the reference under bf16 autocast {ref:.4e}; ratio {dev / ref:.3f}")
        ok = ok and dev <= 2 * ref
    print("\n" + "\n".join(lines))
    assert ok, lines


def test_eval_mode_uses_the_running_buffers_and_leaves_them_alone():
    """After one training step: the eval output and the eval-mode gradients (frozen statistics: no batch-mean terms, live convolution
    biases) meet the f32 bar against the restatement on the updated buffers, which eval forwards leave bit-unchanged."""
    sd, g, x, dout, r64 = R.pick("odd")
    m = module(sd)
    run_module(m, g, x, dout)
    m.eval()
    before = {k: v.clone() for k, v in m.named_buffers()}
    sd2 = {**sd, **{k: v.cpu() for k, v in before.items()}}
    e64 = R.run(sd2, g, x, dout, torch.float64, "relu", False)
    e32 = R.run(sd2, g, x, dout, torch.float32, "relu", False)
    with torch.no_grad():
        out = m(g.to(DEV), x.to(DEV))
    got = run_module(m, g, x, dout)
    assert torch.equal(out, got["out"])
    check("odd eval", got, e64, e32, training=False, buffers=False)
    assert all(torch.equal(before[k], v) for k, v in m.named_buffers())
    assert all(float(got["grads"][k].abs().max()) > 0 for k in R.DEAD)


def _ops_run(sd, gs, xs, ds, act="relu", out=None, need_dg=True, training=True):
    from brats21_amd import ops
    params = [sd[k].float().to(DEV) for k in R.PARAMS]
    running = None if training else [sd[k].float().to(DEV) for k in R.BUFFERS if not k.endswith("tracked")]
    o, saved, stats = ops.attgate_fwd(gs, xs, params, act, training=training, out=out, running=running)
    return o, saved, stats, ops.attgate_bwd(ds, saved, params, need_dg=need_dg)


def _same(a, b):
    (dga, dxa, ga), (dgb, dxb, gb) = a, b
    return ((dga is None and dgb is None) or torch.equal(dga, dgb)) and torch.equal(dxa, dxb) and all(torch.equal(p, q) for p, q in zip(ga, gb))


@pytest.mark.parametrize("storage", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "fp16"])
def test_channel_slice_views_give_the_same_bits(storage):
    """g, x, dout and out= as channel slices of wider buffers (pitch 2C and 3C): the bits of dense tensors, and the neighbouring
    channels of the output buffer stay untouched."""
    from brats21_amd import ops
    sd, g, x, dout, _ = R.pick("odd")
    gs, xs, ds = (ops.ncdhw_to_ndhwc(t.to(DEV), storage) for t in (g, x, dout))
    o, _, stats, bw = _ops_run(sd, gs, xs, ds)
    c = xs.shape[-1]

    def wide(t, k, at):
        buf = torch.full(tuple(t.shape[:4]) + (k * c,), 7.0, dtype=storage, device=DEV)
        buf[..., at * c:(at + 1) * c] = t
        return buf, buf[..., at * c:(at + 1) * c]
    (_, gv), (_, xv), (_, dv) = wide(gs, 2, 1), wide(xs, 3, 1), wide(ds, 2, 0)
    obuf, ov = wide(torch.zeros_like(xs), 3, 2)
    o2, _, stats2, bw2 = _ops_run(sd, gv, xv, dv, out=ov)
    torch.cuda.synchronize()
    assert o2.data_ptr() == ov.data_ptr() and torch.equal(ov, o) and _same(bw, bw2)
    assert bool((obuf[..., :2 * c] == 7.0).all())
    assert all(torch.equal(a, b) for sa, sb in zip(stats, stats2) for a, b in zip(sa, sb))


@pytest.mark.parametrize("name", ["odd", "blocks"])
def test_two_runs_give_identical_bits(name):
    sd, g, x, dout, _ = R.pick(name)
    a, b = run_module(module(sd), g, x, dout), run_module(module(sd), g, x, dout)
    assert all(torch.equal(a[n], b[n]) for n in ("out", "dg", "dx"))
    assert all(torch.equal(a["grads"][k], b["grads"][k]) for k in R.PARAMS) and all(torch.equal(a["buffers"][k], b["buffers"][k]) for k in R.BUFFERS)


def test_save_false_gives_the_training_forwards_bits_and_keeps_nothing():
    from brats21_amd import ops
    sd, g, x, dout, _ = R.pick("odd")
    full = run_module(module(sd), g, x, dout)
    gd, xd = g.to(DEV), x.to(DEV)
    m = module(sd)
    with torch.no_grad():  # the module under no_grad (training mode: batch statistics, the buffers move)
        out = m(gd, xd)
    assert not out.requires_grad and torch.equal(out, full["out"])
    assert all(torch.equal(v, full["buffers"][k]) for k, v in m.named_buffers())
    m = module(sd)
    for p in m.parameters():
        p.requires_grad_(False)
    out = m(gd, xd)  # frozen parameters, no input gradient: the inference variant
    assert not out.requires_grad and torch.equal(out, full["out"])
    m = module(sd)
    for p in m.parameters():
        p.requires_grad_(False)
    xx = xd.clone().requires_grad_(True)
    out = m(gd, xx)  # frozen parameters, only x wants a gradient: the training path
    out.backward(dout.to(DEV))
    assert torch.equal(out.detach(), full["out"]) and torch.equal(xx.grad, full["dx"])
    # the wrappers: save=False returns no saved state; need_dg=False skips the g-branch input gradient and changes nothing else
    gs, xs, ds = (ops.ncdhw_to_ndhwc(t.to(DEV), torch.float32) for t in (g, x, dout))
    params = [sd[k].float().to(DEV) for k in R.PARAMS]
    o1, saved, _ = ops.attgate_fwd(gs, xs, params, "relu", save=False)
    o2, _, _, bw = _ops_run(sd, gs, xs, ds)
    _, _, _, bw_nodg = _ops_run(sd, gs, xs, ds, need_dg=False)
    assert saved is None and torch.equal(o1, o2) and bw_nodg[0] is None and bw[0] is not None
    assert torch.equal(bw[1], bw_nodg[1]) and all(torch.equal(a, b) for a, b in zip(bw[2], bw_nodg[2]))
    got = run_module(module(sd), g, x, dout, need_dg=False)
    assert got["dg"] is None and torch.equal(got["dx"], full["dx"]) and all(torch.equal(got["grads"][k], full["grads"][k]) for k in R.PARAMS)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_a_captured_step_replays_the_eager_bits(dtype):
    """One forward + backward captured with torch.cuda.graph on a single stream (nothing in the block reads the host) and replayed
    twice on new inputs: the eager bits, the running buffers after the same number of steps included."""
    sd, g, x, dout, _ = R.pick("odd")
    steps = [(g, x, dout), (g.flip(0), x.flip(2), dout.flip(3)), (x.flip(1), g.flip(1), dout.flip(4))]  # (f_g == f_l here)
    eager_m = module(sd, storage=dtype)
    for a, b, c in (steps[0], steps[0], steps[1], steps[2]):
        eager = run_module(eager_m, a, b, c)
    m = module(sd, storage=dtype)
    gs, xs, ds = (torch.zeros(tuple(t.shape), device=DEV) for t in (g, x, dout))
    gs.requires_grad_(True)
    xs.requires_grad_(True)
    with torch.no_grad():
        for dst, src in zip((gs, xs, ds), steps[0]):
            dst.copy_(src.to(DEV))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            m(gs, xs).backward(ds)
    torch.cuda.current_stream().wait_stream(side)
    gs.grad = xs.grad = None
    m.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = m(gs, xs)
        out.backward(ds)
    for step in steps[1:]:
        with torch.no_grad():
            for dst, src in zip((gs, xs, ds), step):
                dst.copy_(src.to(DEV))
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.detach(), eager["out"]) and torch.equal(gs.grad, eager["dg"]) and torch.equal(xs.grad, eager["dx"])
    assert all(torch.equal(p.grad, eager["grads"][k]) for k, p in m.named_parameters())
    assert all(torch.equal(v, eager["buffers"][k]) for k, v in m.named_buffers()) and int(m.psi["1"].num_batches_tracked) == 4


def test_saved_state_holds_no_further_tensor_of_x_or_f_int_size():
    """AttGateSaved: of x's size only g and x themselves, of f_int size only g1raw and x1raw; no alpha, no p."""
    from brats21_amd import ops
    sd, g, x, dout, _ = R.pick("unlike")
    gs, xs, ds = (ops.ncdhw_to_ndhwc(t.to(DEV), torch.float32) for t in (g, x, dout))
    _, saved, _, _ = _ops_run(sd, gs, xs, ds)
    n, f_g, f_l, f_int, d, h, w = R.SHAPES["unlike"]
    vox = n * d * h * w
    big = {f: getattr(saved, f) for f in ops.AttGateSaved.__slots__ if isinstance(getattr(saved, f), torch.Tensor) and getattr(saved, f).numel() > vox}
    assert set(big) == {"g", "x", "g1raw", "x1raw"} and big["g"] is gs and big["x"] is xs
    assert big["g1raw"].numel() == big["x1raw"].numel() == vox * 16  # f_int = 12 padded to 16
    assert saved.q.numel() == vox and saved.q.dtype == torch.float32
    assert all(getattr(saved, f).numel() <= 2 * 16 for f in ("ss_g", "ss_x", "mr_g", "mr_x", "st1"))
