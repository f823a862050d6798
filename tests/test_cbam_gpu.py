"""GPU tests of brats21_amd.networks.CBAM / ops.cbam_fwd / ops.cbam_bwd (csrc/cbam.hip) against the float64 restatement
tests/_cbam_ref.py, which tests/test_cbam_cpu.py pins to the reference's own class.

Inputs are 2 * randn (dout: randn) rounded to bf16, so that float32 and bfloat16 storage see the same numbers; gamma = 1.3 and
beta = 0.2 leave the ReLU of the spatial gate on for roughly half of the voxels.  A case is accepted only when, on the float64
reference, min |zn| >= 1e-5 (no ReLU decision within rounding), the two largest x * s over the channels of every voxel are >= 1e-5
apart (no arg-max decision within rounding) and no parameter gradient is all zero (a dead hidden unit at hidden width 1 would make
its check vacuous); the seed is the first of base, base + 1, ... (at most 20) that meets them.  Equal maxima over the VOXELS of a
channel are exact ties of the bf16-representable input: they are wanted, and (2, 384, 4, 4, 4) has them.

Bar (the rule of tests/test_softmax_loss_gpu.py): the restatement is also run in float32 on the CPU; per tensor -- out, dx, each
parameter gradient -- the GPU's max abs error against float64 over that tensor's max abs is at most max(4 x the float32 CPU error,
1e-6).  out and dx in bfloat16 storage get 2^-8 |ref| elementwise on top: half a bf16 spacing for the one final rounding.  The
measured errors are printed (pytest -s) and carried in the assertion messages."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import _cbam_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = ((1, 16, 1, 1, 65),     # degenerate extents, hidden width 1
          (2, 16, 9, 7, 11),     # odd everything
          (1, 48, 5, 6, 7),      # extents <= 7
          (2, 384, 4, 4, 4),     # extents < 7, widest C, real voxel ties
          (1, 24, 8, 20, 12),    # C not a multiple of 16
          (1, 96, 16, 16, 16))   # several tiles and partials
STORAGES = (torch.float32, torch.bfloat16)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cbam.npz")


def bf16_round(t):
    return t.bfloat16().float()


def make_case(shape, seed):
    g = torch.Generator().manual_seed(seed)
    c = shape[1]
    ch = c // 16
    sd = {R.KEYS[0]: torch.randn((ch, c), generator=g) * (2.0 / ch) ** 0.5, R.KEYS[1]: (torch.rand((ch,), generator=g) - 0.5) * 0.5,
          R.KEYS[2]: torch.randn((c, ch), generator=g) * (2.0 / c) ** 0.5, R.KEYS[3]: (torch.rand((c,), generator=g) - 0.5) * 0.5,
          R.KEYS[4]: torch.randn((1, 2, 7, 7, 7), generator=g) * (2.0 / 343) ** 0.5,
          R.KEYS[5]: torch.tensor([1.3]), R.KEYS[6]: torch.tensor([0.2])}
    x = bf16_round(2 * torch.randn(shape, generator=g))
    dout = bf16_round(torch.randn(shape, generator=g))
    return sd, x, dout


def preconditions(sd, x, dout):
    parts = {}
    ref = R.run(sd, x, dout, torch.float64, parts)
    top2 = parts["x1"].topk(2, dim=1)[0]
    ok = float(parts["zn"].abs().min()) >= 1e-5 and float((top2[:, 0] - top2[:, 1]).min()) >= 1e-5
    ok = ok and all(float(g.abs().max()) > 0 for g in ref[2].values())
    return ok, ref


@functools.lru_cache(maxsize=None)
def case(shape):
    """(seed, sd, x, dout, float64 result, float32 result): computed once per shape, shared, never modified."""
    base = 100 * (SHAPES.index(shape) + 1)
    for seed in range(base, base + 20):
        sd, x, dout = make_case(shape, seed)
        ok, ref64 = preconditions(sd, x, dout)
        if ok:
            return seed, sd, x, dout, ref64, R.run(sd, x, dout, torch.float32)
    raise AssertionError(f"no seed in {base} .. {base + 19} meets the preconditions for {shape}")


def module(sd, storage):
    from brats21_amd.networks import CBAM
    c = sd[R.KEYS[0]].shape[1]
    m = CBAM(c, reduction_ratio=c // sd[R.KEYS[0]].shape[0])
    m.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    m.storage = storage
    return m.to(DEV)


def run_module(sd, x, dout, storage):
    m = module(sd, storage)
    xx = x.float().to(DEV).requires_grad_(True)
    out = m(xx)
    out.backward(dout.float().to(DEV))
    return out.detach(), xx.grad, {k: p.grad for k, p in m.named_parameters()}


def check(what, got, ref64, ref32, storage):
    lines, ok = [], True
    names = ["out", "dx"] + list(R.KEYS)
    flat = lambda r: [r[0], r[1]] + [r[2][k] for k in R.KEYS]  # noqa: E731
    for name, g, w64, w32 in zip(names, flat(got), flat(ref64), flat(ref32)):
        assert g.dtype == torch.float32 and tuple(g.shape) == tuple(w64.shape) and bool(torch.isfinite(g).all()), name
        scale = float(w64.abs().max())
        ref_err = float((w32.double() - w64).abs().max()) / scale
        bar = max(4.0 * ref_err, 1e-6)
        diff = (g.cpu().double() - w64).abs()
        if storage == torch.bfloat16 and name in ("out", "dx"):
            diff = (diff - 2.0 ** -8 * w64.abs()).clamp(min=0)
        err = float(diff.max()) / scale
        lines.append(f"{what} {name}: max err / max {err:.2e} (bar {bar:.2e}, float32 CPU {ref_err:.2e})")
        ok = ok and err <= bar
    print("\n" + "\n".join(lines))
    assert ok, lines


@pytest.mark.parametrize("storage", STORAGES, ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_value_and_gradients_match_float64(shape, storage):
    seed, sd, x, dout, ref64, ref32 = case(shape)
    got = run_module(sd, x, dout, storage)
    check(f"{shape} seed {seed} {storage}", got, ref64, ref32, storage)


def test_voxel_ties_are_present_at_the_widest_shape():
    _, _, x, _, _, _ = case((2, 384, 4, 4, 4))
    flat = x.flatten(2)
    assert bool(((flat == flat.max(2, keepdim=True)[0]).sum(2) > 1).any())


def _ops_run(sd, xs, ds, out=None):
    from brats21_amd import ops
    params = [sd[k].float().to(DEV) for k in R.KEYS]
    o, saved = ops.cbam_fwd(xs, *params, out=out)
    return o, saved, ops.cbam_bwd(ds, xs, saved, *params)


@pytest.mark.parametrize("storage", STORAGES, ids=["f32", "bf16"])
def test_channel_slice_views_give_the_same_bits(storage):
    """x, dout and out as channel slices of wider buffers (pitch 2C and 3C): the same bits as on dense tensors, and the
    neighbouring channels of the output buffer stay untouched."""
    from brats21_amd import ops
    shape = (2, 16, 9, 7, 11)
    _, sd, x, dout, _, _ = case(shape)
    n, c, d, h, w = shape
    xs, ds = ops.ncdhw_to_ndhwc(x.to(DEV), storage), ops.ncdhw_to_ndhwc(dout.to(DEV), storage)
    o0, _, g0 = _ops_run(sd, xs, ds)
    wide_x = torch.full((n, d, h, w, 2 * c), 7.0, dtype=storage, device=DEV)
    wide_d = torch.full((n, d, h, w, 3 * c), -3.0, dtype=storage, device=DEV)
    wide_o = torch.full((n, d, h, w, 2 * c), 5.0, dtype=storage, device=DEV)
    xv, dv, ov = wide_x[..., c:], wide_d[..., c:2 * c], wide_o[..., :c]
    xv.copy_(xs)
    dv.copy_(ds)
    o1, _, g1 = _ops_run(sd, xv, dv, out=ov)
    assert o1.data_ptr() == wide_o.data_ptr() and o1.stride(3) == 2 * c
    assert torch.equal(o1, o0) and bool((wide_o[..., c:] == 5.0).all())
    assert all(torch.equal(a, b) for a, b in zip(g0, g1))


@pytest.mark.parametrize("storage", STORAGES, ids=["f32", "bf16"])
def test_integer_tie_case(storage):
    """The fixture's tie case (the reference class's own float64 output): s is exactly 0.5, so the ties of x are the ties both max
    operations see.  The saved indices equal torch's -- the lowest voxel, the lowest channel -- and the gradients, which a
    differently routed tie would change by O(1), meet the bar."""
    import torch.nn.functional as F
    from brats21_amd import ops
    z = np.load(GOLDEN)
    sd = {k: torch.from_numpy(z[f"tie/sd/{k}"]) for k in R.KEYS}
    x, dout = torch.from_numpy(z["tie/x"]), torch.from_numpy(z["tie/dout"])
    assert json.loads(str(z["meta"]))["cases"]["tie"] == list(x.shape)
    ref64 = (torch.from_numpy(z["tie/out"]), torch.from_numpy(z["tie/dx"]), {k: torch.from_numpy(z[f"tie/grad/{k}"]) for k in R.KEYS})
    got = run_module(sd, x, dout, storage)
    ref32 = R.run(sd, x, dout, torch.float32)
    # (W2 = 0 in this case: the gradients of W1 and b1 are exactly zero in the reference; compare those absolutely)
    for k in (R.KEYS[0], R.KEYS[1]):
        assert float(ref64[2][k].abs().max()) == 0.0 and float(got[2][k].abs().max()) == 0.0
        ref64[2][k] = ref64[2][k] + 1.0
        ref32[2][k].add_(1.0)
        got[2][k] = got[2][k] + 1.0
    check(f"tie case {storage}", got, ref64, ref32, storage)
    xs = ops.ncdhw_to_ndhwc(x.float().to(DEV), storage)
    _, saved = ops.cbam_fwd(xs, *[sd[k].float().to(DEV) for k in R.KEYS])
    vol = tuple(x.shape[2:])
    _, vox = F.max_pool3d(x, vol, stride=vol, return_indices=True)
    assert torch.equal(saved.argvox.cpu().long(), vox.view(x.shape[0], x.shape[1]))
    assert bool((saved.scale == 0.5).all())
    assert torch.equal(saved.cidx.cpu().long().view(x.shape[0], *vol), torch.max(x * 0.5, 1)[1])


@pytest.mark.parametrize("storage", STORAGES, ids=["f32", "bf16"])
def test_two_runs_give_identical_bits(storage):
    _, sd, x, dout, _, _ = case((1, 96, 16, 16, 16))
    a, b = run_module(sd, x, dout, storage), run_module(sd, x, dout, storage)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(a[2][k], b[2][k]) for k in R.KEYS)


@pytest.mark.parametrize("storage", STORAGES, ids=["f32", "bf16"])
def test_inference_forward_saves_nothing_and_equals_the_training_forward(storage):
    """ops.cbam_fwd(save=False) -- no channel-index plane written, nothing kept -- gives the bits of the training forward."""
    from brats21_amd import ops
    _, sd, x, _, _, _ = case((2, 16, 9, 7, 11))
    xs = ops.ncdhw_to_ndhwc(x.to(DEV), storage)
    params = [sd[k].float().to(DEV) for k in R.KEYS]
    out_train, saved = ops.cbam_fwd(xs, *params)
    out_infer, nothing = ops.cbam_fwd(xs, *params, save=False)
    assert isinstance(saved, ops.CbamSaved) and saved.cidx is not None and nothing is None
    assert out_infer.data_ptr() != out_train.data_ptr() and torch.equal(out_infer, out_train)


@pytest.mark.parametrize("storage", STORAGES, ids=["f32", "bf16"])
def test_module_takes_the_inference_forward_under_no_grad(storage, monkeypatch):
    """The module's parameters always require grad, so only the grad mode tells training from inference: under no_grad (train
    or eval mode) and with nothing to differentiate the module calls cbam_fwd(save=False); the output is the training one."""
    from brats21_amd import ops
    _, sd, x, _, _, _ = case((2, 16, 9, 7, 11))
    m = module(sd, storage)
    calls = []
    real = ops.cbam_fwd

    def spy(*args, **kwargs):
        res = real(*args, **kwargs)
        calls.append((kwargs.get("save", True), res[1]))
        return res

    monkeypatch.setattr(ops, "cbam_fwd", spy)
    out = m(x.to(DEV))  # grad mode on, parameters require grad: the training forward
    assert calls[-1][0] is True and isinstance(calls[-1][1], ops.CbamSaved) and out.requires_grad
    with torch.no_grad():
        out_ng = m(x.to(DEV).requires_grad_(True))
    assert calls[-1] == (False, None) and not out_ng.requires_grad
    m.eval()  # instance statistics in eval as in training: InstanceNorm3d tracks nothing
    with torch.no_grad():
        out_eval = m(x.to(DEV))
    assert calls[-1] == (False, None)
    for p in m.parameters():
        p.requires_grad_(False)
    out_frozen = m(x.to(DEV))  # grad mode on, nothing to differentiate
    assert calls[-1] == (False, None) and not out_frozen.requires_grad
    out_x = m(x.to(DEV).requires_grad_(True))  # frozen parameters, but the input wants its gradient
    assert calls[-1][0] is True and out_x.requires_grad
    assert all(torch.equal(out.detach(), o.detach()) for o in (out_ng, out_eval, out_frozen, out_x))


def test_forward_and_backward_replay_from_a_graph():
    """One forward + backward captured with torch.cuda.graph on a single stream (nothing in the block reads the host), replayed
    twice on new inputs: the bits of the eager run."""
    shape = (2, 16, 9, 7, 11)
    _, sd, x, dout, _, _ = case(shape)
    eager = run_module(sd, x, dout, torch.bfloat16)
    m = module(sd, torch.bfloat16)
    xs = torch.zeros(shape, device=DEV).requires_grad_(True)
    ds = torch.zeros(shape, device=DEV)
    with torch.no_grad():  # captured on other numbers than it is replayed on
        xs.copy_(x.flip(0).to(DEV))
        ds.copy_(dout.flip(1).to(DEV))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            m(xs).backward(ds)
    torch.cuda.current_stream().wait_stream(side)
    xs.grad = None
    m.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = m(xs)
        out.backward(ds)
    with torch.no_grad():
        xs.copy_(x.to(DEV))
        ds.copy_(dout.to(DEV))
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.detach(), eager[0]) and torch.equal(xs.grad, eager[1])
        assert all(torch.equal(p.grad, eager[2][k]) for k, p in m.named_parameters())
