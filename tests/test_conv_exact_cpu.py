"""The exact integer-operand references of tests/_conv_exact_ref.py against torch's f32 CPU convolution and autograd: on
integer operands under the stated bounds both are exact, so they agree bit for bit; one voxel changed by 1 makes the
comparison the GPU tests use (assert_exact) report a mismatch; the preconditions reject operands that violate them; the
mirror of the weight-gradient host rules gives the values worked out by hand from csrc/conv_wgrad.hip."""
import pytest
import torch
import torch.nn.functional as F

import _conv_exact_ref as R

SHAPES = [  # c1, c2, cout, n, size, dil
    (16, 0, 32, 2, (5, 6, 18), 1),     # ragged on every axis
    (8, 0, 48, 1, (8, 8, 16), 2),      # dilation 2
    (16, 48, 32, 2, (4, 6, 7), 1),     # two sources of different widths
    (48, 48, 24, 1, (6, 5, 9), 2),     # two sources at dilation 2
]


def _nc(t):
    return t.permute(0, 4, 1, 2, 3).contiguous()


def _torch_f32(x, x2, w, bias, dy, dil):
    xr = _nc(R._cat(x, x2)).requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    br = bias.clone().requires_grad_(True)
    y = F.conv3d(xr, wr, br, 1, dil, dil)
    y.backward(_nc(dy))
    return y.detach().permute(0, 2, 3, 4, 1), xr.grad.permute(0, 2, 3, 4, 1), wr.grad, br.grad


@pytest.mark.parametrize("c1,c2,cout,n,size,dil", SHAPES)
def test_references_equal_torch_f32_exactly(c1, c2, cout, n, size, dil):
    x, x2, w, bias, y_ref = R.fwd_case(c1, c2, cout, n, size, dil)
    dy = R.int_tensor((n, *size, cout), 11)
    R.require_wgrad_exact(x, dy, x2)
    R.require_fwd_exact(dy, w.transpose(0, 1))
    y, dx, dw, db = _torch_f32(x, x2, w, bias, dy, dil)
    R.assert_exact(y, y_ref, what="forward")
    R.assert_exact(dx, R.dgrad_ref(dy, w, dil), what="input gradient")
    R.assert_exact(dw, R.wgrad_ref(x, dy, dil, 3, x2), what="weight gradient")
    R.assert_exact(db, R.dbias_ref(dy), what="bias gradient")
    for dt in (torch.bfloat16, torch.float16):  # the 16-bit statement: RNE of the exact integer
        R.assert_exact(y.to(dt), y_ref, dt, what="forward, 16-bit")


def test_one_by_one_references_equal_torch():
    x, _, w, bias, y_ref = R.fwd_case(24, 0, 48, 2, (5, 6, 7), 1, 1)
    dy = R.int_tensor((2, 5, 6, 7, 48), 12)
    xr, wr = _nc(x).requires_grad_(True), w.clone().requires_grad_(True)
    y = F.conv3d(xr, wr, bias)
    y.backward(_nc(dy))
    R.assert_exact(y.detach().permute(0, 2, 3, 4, 1), y_ref, what="1x1x1 forward")
    R.assert_exact(wr.grad, R.wgrad_ref(x, dy, 1, 1), what="1x1x1 weight gradient")
    R.assert_exact(xr.grad.permute(0, 2, 3, 4, 1), R.dgrad_ref(dy, w, 1), what="1x1x1 input gradient")


@pytest.mark.parametrize("dil", [4, 6])
def test_wide_dilation_weight_gradient_reference_equals_torch(dil):
    x, _, dy, dw_ref, _ = R.wgrad_case(16, 0, 24, 1, (10, 12, 20), dil)
    wr = torch.zeros(24, 16, 3, 3, 3, requires_grad=True)
    F.conv3d(_nc(x), wr, None, 1, dil, dil).backward(_nc(dy))
    R.assert_exact(wr.grad, dw_ref, what=f"dilation {dil}")


def test_one_voxel_changes_the_comparison():
    """One element of x off by 1 (what a dropped, doubled or misplaced voxel does to a sum) fails assert_exact for the weight
    gradient and for the forward output, f32 and 16-bit."""
    c1, c2, cout, n, size, dil = SHAPES[0]
    x, x2, w, bias, y_ref = R.fwd_case(c1, c2, cout, n, size, dil)
    dy = R.int_tensor((n, *size, cout), 11)
    dw_ref = R.wgrad_ref(x, dy, dil)
    xb = x.clone()
    xb[1, 4, 5, 17, 3] += 1  # the last voxel: a corner of the volume
    assert int((dy[1, 3:, 4:, 16:] != 0).sum()) > 0
    with pytest.raises(AssertionError, match="entries differ"):
        R.assert_exact(R.wgrad_ref(xb, dy, dil).float(), dw_ref, what="dW")
    yb = R.fwd_ref(xb, w, bias, dil)
    with pytest.raises(AssertionError, match="entries differ"):
        R.assert_exact(yb.float(), y_ref, what="y")
    with pytest.raises(AssertionError, match="entries differ"):
        R.assert_exact(yb.float().to(torch.bfloat16), y_ref, torch.bfloat16, what="y bf16")
    st = torch.stack([yb.sum((1, 2, 3)), (yb * yb).sum((1, 2, 3))], -1).float()[:, None]  # one "tile" per sample
    with pytest.raises(AssertionError, match="differs"):
        R.assert_stats_exact(st, y_ref, what="stats")
    good = torch.stack(R.tile_sums_ref(y_ref), -1).float()[:, None]
    R.assert_stats_exact(good, y_ref, squares=R.stats_exact_ok(y_ref), what="stats")


def test_preconditions_reject_violations():
    x = R.int_tensor((1, 4, 4, 16, 8), 1)
    dy = R.int_tensor((1, 4, 4, 16, 8), 2)
    R.require_wgrad_exact(x, dy)
    with pytest.raises(AssertionError, match="2\\^24"):
        R.require_wgrad_exact(x * 2 ** 9, dy * 2 ** 6)           # 256 * 1024 * 128 = 2^25
    with pytest.raises(AssertionError, match="integers"):
        R.require_wgrad_exact(x + 0.5, dy)
    # K alone: 2 x 128 x 128 x 128 voxels of [-2, 2] operands is exactly the bound (K = 4,194,304)
    big = torch.zeros((2, 128, 128, 128, 1))
    big[0, 0, 0, 0, 0] = 2
    with pytest.raises(AssertionError, match="2\\^24"):
        R.require_wgrad_exact(big, big)
    w = R.int_tensor((8, 8, 3, 3, 3), 3)
    R.require_fwd_exact(x, w, R.int_tensor((8,), 4))
    with pytest.raises(AssertionError, match="2\\^24"):
        R.require_fwd_exact(x * 2 ** 10, w * 2 ** 6)             # 27 * 8 * 2048 * 128 > 2^24
    y = torch.full((1, 16, 16, 16, 2), 64.0)                      # 4096 voxels * 64^2 = 2^24
    assert not R.stats_exact_ok(y)
    with pytest.raises(AssertionError, match="y\\^2"):
        R.require_stats_exact(y)
    R.require_stats_exact(y / 2)
    # thinning brings a deep layer's sum of y^2 under its bound
    _, _, _, _, y_thin = R.fwd_case(192, 0, 16, 1, (8, 8, 16), 1, thin=True)
    R.require_stats_exact(y_thin)


def test_generators_are_seeded_integer_and_thin():
    a, b = R.int_tensor((4, 1000), 5), R.int_tensor((4, 1000), 5)
    assert torch.equal(a, b) and not torch.equal(a, R.int_tensor((4, 1000), 6))
    assert set(a.unique().tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    t = R.int_tensor((100000,), 7, 0.25)
    assert 0.24 < float((t != 0).float().mean()) < 0.26 and float(t.abs().max()) == 2.0
    for dt in (torch.bfloat16, torch.float16, torch.float8_e4m3fn):
        assert torch.equal(a.to(dt).float(), a)


def test_mirror_of_the_weight_gradient_host_rules():
    """Values worked out by hand from csrc/conv_wgrad.hip for a 256-CU device."""
    assert [R.wgrad_nlane(t) for t in (4, 16, 31, 32, 63, 64, 127, 128, 1024)] == [1, 1, 1, 2, 2, 4, 4, 8, 8]
    assert R.wgrad_tiles(False, 48, 0, 48) == (3, 3) and R.wgrad_tiles(False, 16, 48, 32) == (2, 1)
    assert R.wgrad_tiles(False, 32, 32, 64) == (2, 2) and R.wgrad_tiles(True, 48, 0, 40) == (3, 1)
    assert R.wgrad_tiles(False, 8, 0, 8) == (1, 1) and R.wgrad_tiles(False, 24, 0, 40) == (3, 2)
    # 384 -> 384 at 16^3, one sample: 16 tiles, one lane; tap-plane: ceil(512 / (3 * 64)) = 3 slabs; all-taps: 64 blocks,
    # g8 = 4, and 16 tiles is exactly the threshold 4 * 1 * 4
    p0 = R.wgrad_plan(True, 1, 384, 0, 384, 1, 16, 16, 16, 0, 256)
    assert (p0["ntiles"], p0["nlane"], p0["nsplit"], p0["cof"], p0["cif"], p0["reduce"]) == (16, 1, 3, 3, 3, "reduce_taps")
    p1 = R.wgrad_plan(True, 1, 384, 0, 384, 1, 16, 16, 16, 1, 256)
    assert (p1["kernel"], p1["nsplit"]) == ("alltaps2<3, 3>", 4)
    assert R.wgrad_plan(True, 2, 384, 0, 384, 1, 16, 16, 16, 1, 256)["kernel"] == "tapplane<16, 2, 3, 3>"
    assert R.wgrad_alltaps_ok(1, True, 1, 384, 0, 384, 15, 256) is None
    # 48 -> 48: one block, 8 lanes x 32: 1024 tiles = 2 x 32 x 64 x 64
    assert R.wgrad_alltaps_ok(1, True, 1, 48, 0, 48, 1023, 256) is None
    assert R.wgrad_alltaps_ok(1, True, 1, 48, 0, 48, 1024, 256) == (32, "alltaps2<3, 3>")
    assert R.smallest_alltaps_volume(48, 0, 48, 256) == (2, (32, 64, 64))
    assert R.wgrad_alltaps_ok(1, True, 1, 8, 0, 64, 1024, 256)[1] == "alltaps_kernel<1, 4>"
    assert R.wgrad_alltaps_ok(1, True, 1, 32, 32, 128, 1024, 256)[1] == "alltaps2<4, 2>"
    assert R.wgrad_alltaps_ok(1, True, 1, 16, 0, 48, 1024, 256)[1] == "alltaps2<3, 1>"
    assert R.wgrad_alltaps_ok(1, False, 1, 48, 0, 48, 1024, 256) is None
    # the reduction: the all-taps-per-block form from 32768 (co, ci) pairs on
    assert R.wgrad_reduce_kind(192, 192, 27) == "reduce_taps" and R.wgrad_reduce_kind(128, 248, 27) == "reduce"
    assert R.wgrad_reduce_kind(384, 96, 1) == "reduce"
    # n = 2, (16, 16, 64) at 48 -> 48: 128 tiles, 8 lanes, g8 = min(ceil(512 / 24), 16) = 16: 128 slabs
    p = R.wgrad_plan(True, 1, 48, 0, 48, 2, 16, 16, 64, 0, 256)
    assert (p["ntiles"], p["nlane"], p["nsplit"], p["reduce"], p["memset"]) == (128, 8, 128, "reduce", False)
    assert R.wgrad_plan(True, 1, 24, 0, 40, 2, 5, 6, 18, 0, 256)["memset"]
    s = R.wgrad_shift_plan(True, 1, 384, 96, 1, 8, 8, 16)
    assert (s["ntiles"], s["nlane"], s["cof"], s["cif"], s["nsplit"]) == (4, 1, 3, 3, 4)


# ---------------------------------------------------------------------------------------------- direct (gather) convolution
def _torch_term(x, w, dy, k, dil):
    """F.conv3d (padding = dilation for k = 3) and its autograd input gradient, channels-last f32."""
    xr = _nc(x).requires_grad_(True)
    y = F.conv3d(xr, w, None, 1, dil if k == 3 else 0, dil)
    y.backward(_nc(dy))
    return y.detach().permute(0, 2, 3, 4, 1), xr.grad.permute(0, 2, 3, 4, 1)


@pytest.mark.parametrize("k,dil,n,size", [(3, 3, 2, (5, 6, 7)), (3, 4, 1, (8, 8, 8)), (3, 6, 2, (5, 6, 7)), (3, 6, 1, (7, 13, 14)),
                                          (1, 1, 2, (5, 6, 7)), (1, 1, 1, (1, 1, 33))])
def test_wide_dilation_and_pointwise_references_equal_torch(k, dil, n, size):
    """fwd_ref and dgrad_ref at the dilations of the ASPP branches (3, 4, 6; on 5x6x7 every extent is thinner than dilation 6)
    and at k = 1, against torch's f32 CPU convolution and autograd, bit for bit."""
    cin, cout = 24, 16
    x, _, w, bias, y_ref = R.fwd_case(cin, 0, cout, n, size, dil, k, seed=3)
    dy = R.int_tensor((n, *size, cout), 13)
    R.require_fwd_exact(dy, w.transpose(0, 1))
    y, dx = _torch_term(x, w, dy, k, dil)
    R.assert_exact(y + bias, y_ref, what=f"forward k {k} dilation {dil}")
    R.assert_exact(dx, R.dgrad_ref(dy, w, dil), what=f"input gradient k {k} dilation {dil}")


def test_dilation_wider_than_the_volume_leaves_the_centre_tap():
    """2 x (5, 6, 7) at dilation 6: every tap that moves in z (extent 5) or y (extent 6) leaves the volume, and an x tap stays
    inside only between the columns x = 0 and x = 6 (extent 7).  So the branch equals a 1x1x1 convolution with the centre
    weights at x = 1..5, and the three (centre, centre, *) taps everywhere -- what the direct kernel's tap masks must reproduce.
    On 2 x (5, 6, 6) the centre tap is all that is left."""
    x, _, w, bias, y_ref = R.fwd_case(16, 0, 32, 2, (5, 6, 7), 6, 3, seed=4)
    centre = w[:, :, 1:2, 1:2, 1:2].contiguous()
    assert torch.equal(y_ref[:, :, :, 1:6], R.fwd_ref(x, centre, bias, 1)[:, :, :, 1:6])
    assert not torch.equal(y_ref[:, :, :, 0], R.fwd_ref(x, centre, bias, 1)[:, :, :, 0])
    wx = torch.zeros_like(w)
    wx[:, :, 1, 1, :] = w[:, :, 1, 1, :]
    assert torch.equal(y_ref, R.fwd_ref(x, wx, bias, 6))
    dy = R.int_tensor((2, 5, 6, 7, 32), 14)
    assert torch.equal(R.dgrad_ref(dy, w, 6), R.dgrad_ref(dy, wx, 6))
    assert torch.equal(R.dgrad_ref(dy, w, 6)[:, :, :, 1:6], R.dgrad_ref(dy, centre, 1)[:, :, :, 1:6])
    x6, _, w6, b6, y6 = R.fwd_case(16, 0, 32, 2, (5, 6, 6), 6, 3, seed=4)
    assert torch.equal(y6, R.fwd_ref(x6, w6[:, :, 1:2, 1:2, 1:2].contiguous(), b6, 1))


def test_four_term_sum_equals_the_sum_of_four_torch_input_gradients():
    """The reference of a four-term PACK_DGRAD job (dconv_case, mode "dgrad") = the sum of four F.conv3d autograd input gradients
    (summed in float64: every one of them is an exact integer), and that of a forward job = the sum of four F.conv3d outputs."""
    n, size = R.VOL_RAGGED
    terms = ((16, 1, 1), (48, 3, 3), (32, 3, 6), (8, 3, 2))
    case = R.dconv_case(n, size, ((36, terms, False),), "dgrad")
    job = case.jobs[0]
    tot = torch.zeros((n, *size, 36), dtype=torch.float64)
    for t in job.terms:
        xr = torch.zeros((n, 36, *size), requires_grad=True)
        F.conv3d(xr, t.w, None, 1, t.dil if t.k == 3 else 0, t.dil).backward(_nc(t.x))
        tot += xr.grad.permute(0, 2, 3, 4, 1).double()
    R.assert_exact(tot.float(), job.ref, what="four-term input gradient")
    fwd = R.dconv_case(n, size, ((36, terms, True),), "fwd").jobs[0]
    tot = sum(F.conv3d(_nc(t.x), t.w, None, 1, t.dil if t.k == 3 else 0, t.dil).permute(0, 2, 3, 4, 1).double() for t in fwd.terms)
    R.assert_exact((tot + fwd.bias.double()).float(), fwd.ref, what="four-term forward")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "f32"])
def test_every_dconv_case_meets_its_preconditions(dtype):
    """Every launch of tests/test_dconv_exact_gpu.py, built on the CPU: the builders assert the 2^24 bound on the operands and, for
    the 16-bit types, max|reference| <= 256 (bf16) / 2048 (fp16) -- the store then rounds nothing and a change of 1 in any output
    is visible.  Checked again here from outside the builders, with the operands' exactness in the storage type."""
    bound = R.OUT_BOUND[dtype]
    cases = R.dconv_cases(dtype)
    assert len(cases) == len(R.dconv_cases(torch.float32))
    for name, args in cases.items():
        case = R.dconv_case(*args)
        for job in case.jobs:
            assert job.ref.shape == (case.n, *case.size, job.rows) and float(job.ref.abs().max()) > 0, name
            assert torch.equal(job.ref, job.ref.round()), name
            if bound is not None:
                assert float(job.ref.abs().max()) <= bound, name
                assert torch.equal(job.ref.float().to(dtype).double(), job.ref), name  # the final rounding is the identity
            for t in job.terms:
                assert torch.equal(t.x.to(dtype).float(), t.x) and torch.equal(t.w.to(dtype).float(), t.w), name
    for c1, c2, cout, (n, size), k, dil in R.DCONV_SPLIT_CASES:
        y = R.dconv_split_case(c1, c2, cout, n, size, k, dil, bound)[-1]
        assert bound is None or torch.equal(y.float().to(dtype).double(), y)
    for nb, cin, q, n, size in R.ASPP_CASES:
        a = R.aspp_case(nb, cin, q, n, size, bound)
        assert len(a.dx_parts) == (nb + 3) // 4 and torch.equal(sum(a.dx_parts), a.dx)
        if bound is not None:
            # each launch's partial is stored unrounded, so torch's 16-bit adds of the parts are exact too
            run = torch.zeros_like(a.dx)
            for p in a.dx_parts:
                run = run + p
                assert float(p.abs().max()) <= bound and float(run.abs().max()) <= bound
            for t in (a.acat, a.dx):
                assert torch.equal(t.float().to(dtype).double(), t)


def test_dconv_case_list_reaches_the_kernel_geometry():
    """The properties of the case list that the kernel's branches need (NF = 3 row fragments of 32 per workgroup, 256 voxels per
    workgroup, a pipeline three steps deep), asserted on the list itself."""
    for dtype in (torch.bfloat16, torch.float32):
        kch, cases = R.DCONV_KCH[dtype], R.dconv_cases(dtype)
        steps = {sum(R._taps_of(k) * cin // kch for cin, k, _ in jobs[0][1]) for name, (_, _, jobs, _, _) in cases.items() if name.startswith("k1-")}
        assert steps == {1, 2, 3, 4, 7}   # below, at and above the pipeline depth, and no multiple of it
        rows = sorted({jobs[0][0] for name, (_, _, jobs, _, _) in cases.items() if name.startswith("rows")})
        assert rows == [4, 16, 36, 96, 100, 132]
        frags = [(r + 31) // 32 for r in rows]
        assert [(f + R.DCONV_NF - 1) // R.DCONV_NF for f in frags] == [1, 1, 1, 1, 2, 2]     # 100, 132: a second blockIdx.y ...
        assert [f - R.DCONV_NF for f in frags[4:]] == [1, 2]                                  # ... with one and with two live fragments
        assert [r % 32 for r in rows] == [4, 16, 4, 0, 4, 4]                                  # tails inside a fragment at a granule of 4
        net = cases["net-rows-2x5x6x7"][2]
        assert [j[0] for j in net] == [100, 16, 36, 4] and [j[1][0][1:] for j in net] == [(1, 1), (3, 2), (3, 4), (3, 6)]
    vox = [n * s[0] * s[1] * s[2] for n, s in R.DCONV_VOLUMES]
    assert vox == [420, 90, 33, 1024]
    assert vox[0] % R.DCONV_WG_VOX and vox[0] % 32 and (vox[0] // 2) % 32     # partial workgroup and fragment, a fragment across samples
    assert vox[1] < R.DCONV_WG_VOX - 64 and vox[3] % R.DCONV_WG_VOX == 0      # a whole wave idle / whole workgroups only


def test_dconv_preconditions_reject_violations():
    x, w = R.int_tensor((1, 2, 2, 4, 16), 1), R.int_tensor((8, 16, 3, 3, 3), 2)
    R.require_terms_exact([(x, w), (x, w)], R.int_tensor((8,), 3))
    with pytest.raises(AssertionError, match="2\\^24"):
        R.require_terms_exact([(x * 2 ** 7, w * 2 ** 5)] * 4)      # 4 * 27 * 16 * 256 * 64 > 2^24 though one term alone is below
    R.require_terms_exact([(x * 2 ** 7, w * 2 ** 5)])
    with pytest.raises(AssertionError, match="integers"):
        R.require_terms_exact([(x, w + 0.5)])
    R.require_within(torch.tensor([256.0, -3.0]), 256.0)
    with pytest.raises(AssertionError, match="exceeds 256"):
        R.require_within(torch.tensor([257.0]), 256.0)
    with pytest.raises(AssertionError, match="exceeds 256"):      # dense operands at cin = 96 do not fit bf16 (the builder thins them)
        R.require_within(R.fwd_case(96, 0, 32, 2, (8, 8, 8), 1)[-1], 256.0)
    assert R.thin_density(16, 256.0) == 1.0 and R.thin_density(27 * 96, 256.0) < 0.5 and R.thin_density(27 * 96, None) == 1.0
