"""-m gpu: the size-selected forms of the streaming norm / pool / up-sampling kernels, one op at a time.

From 256 MiB on (csrc/common.hpp stream_nt(), big_tensor(), big_tensor16()) these kernels run another template instantiation
(non-temporal loads and stores) under other grid caps; the statistics finalize takes two launches from 32768 (tile, channel)
pairs per group on, and the slab reduction has more than one slab from 128 tiles on.  The other op-level tests run 1 - 3
blocks per sample and reach none of this, so every op is run here at the smallest shape that crosses its switch, on both
sides of it, against a float64 statement of the same operation on the same stored inputs (torch, on the device), and --
where an op is per-sample and per-element -- the two forms against each other bit for bit.

Tolerances are derived, not measured:
  * an element stored in 16 bits: |got - ref| <= ulp16 * |ref| + 2^-22 * M, ulp16 = 2^-8 (bf16) / 2^-11 (fp16) -- one full
    storage step against the half step round-to-nearest needs --, M = the f64 sum of the absolute values of the terms the
    formula adds before it rounds; f32 storage: 2^-21 * M.  fp16 results below 2^-14 are subnormal: the storage step stays
    2^-24 there however small |ref| is, so the first term is max(ulp16 * |ref|, 2^-24) for fp16 (a leaky-relu output of
    -2.68e-7 is stored as -2.38e-7, the nearest fp16 value, half a step away: with ulp16 * |ref| alone 5401 of 67 M such
    elements miss the bound, every one of them below 2^-14 and within 0.51 x 2^-24 of the reference);
  * an f32 sum over voxels: |got - ref| <= 2^-24 * sqrt(n) * sum|t| (n terms t), the gradients here given a positive offset so
    that sum t is comparable to sum|t| (one block of 2048 going missing moves a sum by ~5e-4, the tolerance is ~7e-5);
  * dy of a backward also carries the error of the sums it is built from: + |d dy / d sum| * tol(sum);
  * elements whose pre-activation lies within 2^-20 * M of zero are left out of a dy comparison (their mask may differ
    legitimately); every test asserts that this share is at most 1e-5;
  * exact-count cases (all terms exactly 1): sums equal the voxel count with ==, dy equals the formula's constant everywhere.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BIG = 256 << 20            # bytes; csrc/common.hpp stream_nt() (big_tensor(), big_tensor16()): >= BIG takes the large form
S = (112, 112, 112)        # 1,404,928 voxels: x 48 channels x 2 B = 134.9 MB (N = 1: normal, capped grids), 269.7 MB (N = 2: big)
S32 = (80, 80, 80)         # f32 x 48 channels = 98.3 MB: the normal form of f32 tensors with gx = 3048 > 2048 blocks
G = 8                      # groups
BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
ULP16 = {BF: 2.0 ** -8, HF: 2.0 ** -11}
STEP_MIN = {BF: 0.0, HF: 2.0 ** -24}   # the storage step where it stops shrinking: fp16 is subnormal below 2^-14 (bf16: 2^-133, never met)
SLOPE = float(torch.tensor(0.01, dtype=torch.float32))   # the f32 value the kernels multiply by
EXCLUDED_MAX = 1e-5


@pytest.fixture(autouse=True)
def _release():
    yield
    torch.cuda.empty_cache()  # (a handful of 1.1 GB f64 tensors per case)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _gen(seed):
    return torch.Generator(device=_dev()).manual_seed(seed)


def _randn(g, shape, dtype=F32, scale=1.0, positive=False):
    """N(0, 1) * scale (positive: 0.5 + |N(0, 1)|), generated on the device and rounded to the storage type."""
    t = torch.randn(shape, generator=g, device=_dev())
    if positive:
        t.abs_().add_(0.5)
    if scale != 1.0:
        t.mul_(scale)
    return t.to(dtype)


def _rand(g, shape, lo=0.5):
    return torch.rand(shape, generator=g, device=_dev()) + lo


def _side(t, big):
    """The tensor's byte count is on the intended side of the switch."""
    nbytes = t.numel() * t.element_size()
    assert (nbytes >= BIG) == big, f"{tuple(t.shape)} {t.dtype}: {nbytes} bytes is on the wrong side of {BIG}"
    return t


def _bc(p):
    """[N, C] -> f64 [N, 1, 1, 1, C]"""
    return p.double()[:, None, None, None, :]


def _gbc(p, c):
    """[N, groups] -> f64 [N, 1, 1, 1, C]"""
    return _bc(p.repeat_interleave(c // p.shape[1], 1))


def _vsum(t):
    return t.sum((1, 2, 3))


def _cut(t, i):
    """Piece i of 2 of an activation tensor, whole for a per-sample, per-element op and below BIG: sample i of an N = 2
    tensor, depth half i of an N = 1 tensor."""
    if t.shape[0] > 1:
        return t[i].unsqueeze(0)
    h = t.shape[1] // 2
    return t[0, i * h:(i + 1) * h].unsqueeze(0)


def _cutp(p, i):
    """The per-sample parameters that go with _cut(t, i)."""
    return p[i:i + 1] if p.shape[0] > 1 else p


def _check_elem(name, got, ref, m, dtype, extra=None, keep=None):
    """|got - ref| <= max(ulp16 * |ref|, smallest storage step) + 2^-22 * M (+ extra); f32 storage: 2^-21 * M (+ extra)."""
    err = (got.double() - ref).abs_()
    bound = m * (2.0 ** -21 if dtype == F32 else 2.0 ** -22)
    if dtype != F32:
        bound += (ref.abs() * ULP16[dtype]).clamp_min_(STEP_MIN[dtype])
    if extra is not None:
        bound += extra
    ratio = err.div_(bound.clamp_min_(1e-300))
    if keep is not None:
        ratio = torch.where(keep, ratio, torch.zeros((), dtype=ratio.dtype, device=ratio.device))
    worst = float(ratio.max())
    print(f"  {name}: worst |got - ref| / bound = {worst:.3f}")
    assert bool(torch.isfinite(got).all()), name
    assert worst <= 1.0, (name, worst)


def _check_sum(name, got, ref, n_terms, abs_sum, extra=None):
    """|got - ref| <= 2^-24 * sqrt(n) * sum|t| (+ extra)."""
    tol = abs_sum * (2.0 ** -24 * math.sqrt(n_terms))
    if extra is not None:
        tol = tol + extra
    err = (got.double() - ref).abs()
    worst = float((err / tol.clamp_min(1e-300)).max())
    rel = float((err / ref.abs().clamp_min(1e-300)).max())
    print(f"  {name}: worst |got - ref| / bound = {worst:.3f} (worst relative error {rel:.2e})")
    assert bool(torch.isfinite(got).all()), name
    assert worst <= 1.0, (name, worst)


def _share(name, keep):
    share = 1.0 - float(keep.sum()) / keep.numel()
    print(f"  {name}: share of elements within 2^-20 * M of a zero pre-activation (left out of dy) = {share:.2e}")
    assert share <= EXCLUDED_MAX, (name, share)


def _ulps(ref64):
    """The f32 spacing at ref (f64 tensor)."""
    r = ref64.float().abs()
    return (torch.nextafter(r, torch.full_like(r, float("inf"))) - r).double()


# =====================================================================================================================
# affine_act / affine_act_pool
# =====================================================================================================================
def _affine_params(g, n, c):
    return torch.stack([1.0 + 0.3 * _randn(g, (n, c)), 0.2 * _randn(g, (n, c))], -1).contiguous()


def _affine_ref(y, ss, act):
    """f64: z = act(y * scale + shift), M = |y * scale| + |shift|; also pre and M for the backward's exclusion rule."""
    sc, sh = _bc(ss[..., 0]), _bc(ss[..., 1])
    t = y.double() * sc
    m = t.abs() + sh.abs()
    pre = t.add_(sh)
    z = torch.where(pre > 0, pre, pre * (0.0 if act == "relu" else SLOPE))
    return z, m, pre


AFFINE_CASES = [  # dtype, act, N, size, C, big
    (BF, "relu", 1, S, 48, False), (BF, "leakyrelu", 2, S, 48, True), (BF, "relu", 1, S, 96, True),
    (HF, "leakyrelu", 1, S, 48, False), (HF, "relu", 2, S, 48, True),
    (F32, "relu", 1, S32, 48, False), (F32, "leakyrelu", 1, S, 48, True),
]


@pytest.mark.parametrize("dtype,act,n,size,c,big", AFFINE_CASES)
def test_affine_act(dtype, act, n, size, c, big):
    """brats_affine_act_fwd: caps 2048 / 8192 blocks (gx = 4182 at C = 48, 8363 at C = 96, 3048 for f32 at 80^3), the
    unrolled-by-two loop and its tail, the NT instantiations of bf16 / fp16 / f32.  z against f64; |max| == the maximum of the
    stored values; the big form == the normal form on each sample (N = 2) or depth half (N = 1), bit for bit."""
    from brats21_amd import ops
    g = _gen(101)
    y = _side(_randn(g, (n, *size, c), dtype), big)
    ss = _affine_params(g, n, c)
    amax = torch.zeros(1, device=y.device)
    z = ops.affine_act(y, ss, act, slope=0.01, amax=amax)
    ref, m, _ = _affine_ref(y, ss, act)
    _check_elem("z", z, ref, m, dtype)
    del ref, m
    assert float(amax) == float(z.abs().max()), "amax is the maximum of the stored values"
    if big:
        am = []
        for i in range(2):
            a_i = torch.zeros(1, device=y.device)
            z_i = ops.affine_act(_side(_cut(y, i), False), _cutp(ss, i), act, slope=0.01, amax=a_i)
            assert torch.equal(z_i, _cut(z, i)), f"piece {i}: big form != normal form"
            am.append(float(a_i))
        assert float(amax) == max(am)


def _windows(z):
    """[N, D, H, W, C] -> [N, D/2, H/2, W/2, C, 8], the window in d, h, w order."""
    n, d, h, w, c = z.shape
    return z.view(n, d // 2, 2, h // 2, 2, w // 2, 2, c).permute(0, 1, 3, 5, 7, 2, 4, 6).reshape(n, d // 2, h // 2, w // 2, c, 8)


POOL_CASES = [  # dtype, act, N, C, with_avg, big
    (BF, "relu", 1, 48, False, False), (BF, "leakyrelu", 2, 48, True, True), (BF, "relu", 1, 96, False, True),
    (HF, "leakyrelu", 1, 48, False, False), (HF, "relu", 2, 48, False, True),
]


@pytest.mark.parametrize("dtype,act,n,c,with_avg,big", POOL_CASES)
def test_affine_act_pool(dtype, act, n, c, with_avg, big):
    """brats_affine_act_pool_fwd: 9408 items per sample at C = 48 (18816 at C = 96) against caps of 2048 / 8192 blocks, so
    every block walks several items through its two LDS buffers.  z against f64; the pooled maximum == the maximum of the
    STORED window, the arg-max byte == the first maximum in d, h, w order (both exact); the pooled mean against f64 of the
    stored window; |max| == max |z|; big form == normal form per piece (z, pooled, arg-max bytes, |max|)."""
    from brats21_amd import ops
    g = _gen(102)
    y = _side(_randn(g, (n, *S, c), dtype), big)
    ss = _affine_params(g, n, c)
    amax = torch.zeros(1, device=y.device)
    z, pooled = ops.affine_act_pool(y, ss, act, slope=0.01, amax=amax, with_avg=with_avg, want_argmax=True)
    idx = z._pool_argmax
    ref, m, _ = _affine_ref(y, ss, act)
    _check_elem("z", z, ref, m, dtype)
    del ref, m
    assert float(amax) == float(z.abs().max())
    win = _windows(z)
    mx = win.amax(-1)
    assert torch.equal(pooled[..., :c], mx), "pooled maximum != maximum of the stored window"
    order = torch.arange(8, 0, -1, dtype=torch.uint8, device=y.device)
    first = 8 - ((win == mx[..., None]).to(torch.uint8) * order).amax(-1)
    assert torch.equal(idx, first.to(torch.uint8)), "arg-max byte != first maximum of the window in d, h, w order"
    if with_avg:
        w64 = win.double()
        _check_elem("pooled mean", pooled[..., c:], w64.sum(-1) * 0.125, w64.abs().sum(-1) * 0.125, dtype)
        del w64
    del win, mx, first
    if big:
        am = []
        for i in range(2):
            a_i = torch.zeros(1, device=y.device)
            z_i, p_i = ops.affine_act_pool(_side(_cut(y, i), False), _cutp(ss, i), act, slope=0.01, amax=a_i, with_avg=with_avg,
                                           want_argmax=True)
            assert torch.equal(z_i, _cut(z, i)) and torch.equal(p_i, _cut(pooled, i)), f"piece {i}: big form != normal form"
            assert torch.equal(z_i._pool_argmax, _cut(idx, i)), f"piece {i}: arg-max bytes differ between the forms"
            am.append(float(a_i))
        assert float(amax) == max(am)


# =====================================================================================================================
# GroupNorm + activation backward: gn_act_bwd, _pool, _head, _tiles
# =====================================================================================================================
def _gn_params(g, n, c):
    ss = _affine_params(g, n, c)
    mr = torch.stack([0.1 * _randn(g, (n, G)), _rand(g, (n, G))], -1).contiguous()  # (mean, rstd in [0.5, 1.5))
    gamma = 1.0 + 0.3 * _randn(g, (c,))
    return ss, mr, gamma


def _gn_bwd_ref(dz, dzabs, y, ss, mr, gamma, act, sums=None, want_z=False):
    """f64 statement of csrc/norm.hip's two passes.  u = dz * act'(pre), pre = y * scale + shift; xhat = (y - mean_g) * rstd_g;
    S1 = sum_v u, S2 = sum_v u * xhat per (n, c); m_i = sum_{c in g} gamma_c * S_i / (cpg * V);
        dy = rstd * (gamma * u - m1 - xhat * m2);  dbeta = sum_n S1, dgamma = sum_n S2.
    The terms dy adds: rstd * gamma * u, the cpg terms rstd * gamma_c * S1_c / M, and (y * rstd) and (mean * rstd) times the cpg
    terms rstd * gamma_c * S2_c / M -- their absolute sum is M_dy.  d dy / d m1 = -rstd, d dy / d m2 = -rstd * xhat, and m_i
    inherits sum_c |gamma_c| * tol(S_i,c) / M from the f32 sums, tol(S) = 2^-24 * sqrt(V) * sum|t|: that is `extra`.
    sums = (S1, S2, A1, A2, tol1, tol2) replaces the sums over voxels (the _tiles form, whose sums come from its tile input).
    dz / dzabs: the gradient and the absolute sum of the terms it is composed from (f64)."""
    n, c = ss.shape[0], ss.shape[1]
    cpg = c // G
    vox = y[0, ..., 0].numel()
    y = y.double()
    z, mpre, pre = _affine_ref(y, ss, act)
    keep = pre.abs() > mpre * 2.0 ** -20
    mask = torch.where(pre > 0, 1.0, 0.0 if act == "relu" else SLOPE)
    del mpre, pre
    if not want_z:
        z = None
    u = dz * mask
    uabs = dzabs * mask
    del mask
    mean, r = _gbc(mr[..., 0], c), _gbc(mr[..., 1], c)
    xhat = (y - mean) * r
    if sums is None:
        s1, s2 = _vsum(u), _vsum(u * xhat)
        a1, a2 = _vsum(uabs), _vsum(uabs * xhat.abs())
        t1, t2 = a1 * (2.0 ** -24 * math.sqrt(vox)), a2 * (2.0 ** -24 * math.sqrt(vox))
    else:
        s1, s2, a1, a2, t1, t2 = sums
    gm = gamma.double()

    def grp(q):  # [N, C] -> sum over the group's channels / M, back on [N, 1, 1, 1, C]
        return _gbc(q.view(n, G, cpg).sum(2) / (cpg * vox), c)

    m1, m2 = grp(s1 * gm), grp(s2 * gm)
    m1a, m2a = grp((s1 * gm).abs()), grp((s2 * gm).abs())
    d1, d2 = grp(t1 * gm.abs()), grp(t2 * gm.abs())
    ref = r * (u * gm - m1 - xhat * m2)
    m = (uabs * gm.abs() + m1a + ((y * r).abs_() + (mean * r).abs()) * m2a) * r
    extra = (xhat.abs_() * d2 + d1) * r
    return dict(dy=ref, m=m, extra=extra, keep=keep, z=z, s=(s1, s2, a1, a2), n_sum=n * vox)


def _check_gn_bwd(res, dtype, dy, dgamma, dbeta, n_sum=None):
    _share("dy", res["keep"])
    _check_elem("dy", dy, res["dy"], res["m"], dtype, extra=res["extra"], keep=res["keep"])
    s1, s2, a1, a2 = res["s"]
    n_sum = n_sum or res["n_sum"]
    _check_sum("dbeta", dbeta, s1.sum(0), n_sum, a1.sum(0))
    _check_sum("dgamma", dgamma, s2.sum(0), n_sum, a2.sum(0))


GN_CASES = [  # dtype, act, N, size, C, big
    (BF, "relu", 1, S, 48, False), (BF, "leakyrelu", 2, S, 48, True), (BF, "relu", 1, S, 96, True),
    (HF, "leakyrelu", 1, S, 48, False), (HF, "relu", 2, S, 48, True),
    (F32, "relu", 1, S32, 48, False), (F32, "leakyrelu", 1, S, 48, True),
]


@pytest.mark.parametrize("dtype,act,n,size,c,big", GN_CASES)
def test_gn_act_bwd(dtype, act, n, size, c, big):
    """brats_gn_act_bwd: pass 1 on 512 / 2048 blocks (four voxels in flight + single-voxel tail, per-block partials added in
    block order), pass 2 on 2048 / 8192 blocks; dy = rstd * (gamma * u - m1 - xhat * m2) -- see _gn_bwd_ref for the terms of M
    and for d dy / d sum."""
    from brats21_amd import ops
    g = _gen(103)
    y = _side(_randn(g, (n, *size, c), dtype), big)
    dz = _randn(g, (n, *size, c), dtype, positive=True)
    ss, mr, gamma = _gn_params(g, n, c)
    amax = torch.zeros(1, device=y.device)
    dy, dgamma, dbeta = ops.gn_act_bwd(dz, y, ss, mr, gamma, G, act, slope=0.01, amax=amax)
    assert float(amax) == float(dy.abs().max())
    dz64 = dz.double()
    _check_gn_bwd(_gn_bwd_ref(dz64, dz64, y, ss, mr, gamma, act), dtype, dy, dgamma, dbeta)


def _pool_dz(dskip, dpool, idx, with_avg=False):
    """f64: dskip + max-pool backward of dpool through the arg-max bytes (+ the mean's share), and the absolute sum of the
    pieces."""
    n, d, h, w, c = dskip.shape
    dev = dskip.device
    kz, ky, kx = (torch.arange(s, device=dev) & 1 for s in (d, h, w))
    k = ((kz[:, None, None] << 2) | (ky[None, :, None] << 1) | kx[None, None, :]).to(torch.uint8)  # window index of a voxel

    def full(t):  # pooled resolution -> full resolution
        return t.repeat_interleave(2, 1).repeat_interleave(2, 2).repeat_interleave(2, 3)

    sel = full(idx) == k[None, :, :, :, None]
    dz = full(dpool[..., :c]).double() * sel
    del sel
    dza = dz.abs()
    if with_avg:
        av = full(dpool[..., c:]).double() * 0.125
        dz += av
        dza += av.abs_()
        del av
    sk = dskip.double()
    dz += sk
    dza += sk.abs_()
    return dz, dza


POOLBWD_CASES = [(BF, "relu", 1, False), (BF, "leakyrelu", 2, True), (HF, "leakyrelu", 1, False), (HF, "relu", 2, True)]


@pytest.mark.parametrize("dtype,act,n,big", POOLBWD_CASES)
def test_gn_act_bwd_pool(dtype, act, n, big):
    """brats_gn_act_bwd_pool, the arg-max bytes from affine_act_pool: dz = dskip + (argmax == window index ? dpool : 0) is
    composed inside both passes (two voxels in flight + tail)."""
    from brats21_amd import ops
    g = _gen(104)
    c = 48
    y = _side(_randn(g, (n, *S, c), dtype), big)
    ss, mr, gamma = _gn_params(g, n, c)
    z, _ = ops.affine_act_pool(y, ss, act, slope=0.01, want_argmax=True)
    idx = z._pool_argmax
    del z
    dskip = _randn(g, (n, *S, c), dtype, positive=True)
    dpool = _randn(g, (n, S[0] // 2, S[1] // 2, S[2] // 2, c), dtype, positive=True)
    amax = torch.zeros(1, device=y.device)
    dy, dgamma, dbeta = ops.gn_act_bwd_pool(dskip, dpool, idx, y, ss, mr, gamma, G, act, slope=0.01, amax=amax)
    assert float(amax) == float(dy.abs().max())
    dz64, dza = _pool_dz(dskip, dpool, idx)
    _check_gn_bwd(_gn_bwd_ref(dz64, dza, y, ss, mr, gamma, act), dtype, dy, dgamma, dbeta)


@pytest.mark.parametrize("dtype,act,n,big", POOLBWD_CASES)
def test_gn_act_bwd_head(dtype, act, n, big):
    """brats_gn_act_bwd_head (K = 3): dz = W_head^T dlogits on the fly, four voxels in flight + tail; the head's weight / bias
    gradients sum_v dl[k] * z[c] and sum_v dl[k] come out of pass 1 (n = N * V terms each)."""
    from brats21_amd import ops
    g = _gen(105)
    c, k = 48, 3
    vox = S[0] * S[1] * S[2]
    y = _side(_randn(g, (n, *S, c), dtype), big)
    ss, mr, gamma = _gn_params(g, n, c)
    dl = _randn(g, (n, k, *S), positive=True)
    hw = 0.1 + 0.1 * _randn(g, (k, c, 1, 1, 1)).abs()
    dy, dgamma, dbeta, dhw, dhb = ops.gn_act_bwd_head(dl, hw, y, ss, mr, gamma, G, act, slope=0.01)
    dl64 = dl.double().view(n, k, vox)
    dz64 = (dl64.transpose(1, 2) @ hw.double().view(k, c)).view(n, *S, c)  # (all terms positive: dz is its own absolute sum)
    res = _gn_bwd_ref(dz64, dz64, y, ss, mr, gamma, act, want_z=True)
    _check_gn_bwd(res, dtype, dy, dgamma, dbeta)
    zf = res["z"].view(n, vox, c)
    _check_sum("dhead_weight", dhw.view(k, c), (dl64 @ zf).sum(0), n * vox, (dl64 @ zf.abs()).sum(0))
    _check_sum("dhead_bias", dhb, dl64.sum((0, 2)), n * vox, dl64.sum((0, 2)))


def _chunk_sums(t, tps):
    """[N, V, C] f64 -> [N, tps, C]: sums over tps consecutive chunks of the voxels (the last ones one voxel shorter when tps
    does not divide V)."""
    n, v, c = t.shape
    if v % tps == 0:
        return t.view(n, tps, v // tps, c).sum(2)
    ends = (torch.arange(1, tps + 1, device=t.device) * v) // tps
    cs = t.cumsum(1)[:, ends - 1]
    return torch.cat([cs[:, :1], cs[:, 1:] - cs[:, :-1]], 1)


def _tile_totals(stats):
    """f64 sums over the tiles of an f32 [N, tps, C, 2] statistics tensor and of its absolute values."""
    t = stats.double()
    return t[..., 0].sum(1), t[..., 1].sum(1), t[..., 0].abs().sum(1), t[..., 1].abs().sum(1)


TILES_CASES = [  # dtype, act, N, size, C, tps, big
    (BF, "relu", 1, S, 48, 5488, False), (BF, "leakyrelu", 2, S, 48, 5488, True), (BF, "relu", 1, S, 48, 130, False),
    (BF, "relu", 1, S, 96, 5488, True), (F32, "leakyrelu", 1, S32, 48, 5488, False), (F32, "relu", 1, S, 48, 5488, True),
]


@pytest.mark.parametrize("dtype,act,n,size,c,tps,big", TILES_CASES)
def test_gn_act_bwd_tiles(dtype, act, n, size, c, tps, big):
    """brats_gn_act_bwd_tiles: pass 1 is the f64 slab reduction of the tile statistics (tps = 5488: 64 slabs of 86 tiles, the
    last one short; tps = 130: two slabs of 65), then pass 2 on 2048 / 8192 blocks.  The statistics are built here with torch
    (sum u, sum u * y over consecutive chunks of the voxels, cast to f32) -- the kernels only add tiles, so any partition is a
    valid input --, and the reference sums are the f64 sums of those f32 tiles: S1 = sum T0, S2 = rstd * (sum T1 - mean * sum T0)."""
    from brats21_amd import ops
    g = _gen(106)
    vox = size[0] * size[1] * size[2]
    y = _side(_randn(g, (n, *size, c), dtype), big)
    dz = _randn(g, (n, *size, c), dtype, positive=True)
    ss, mr, gamma = _gn_params(g, n, c)
    dz64, y64 = dz.double(), y.double()
    _, _, pre = _affine_ref(y, ss, act)
    u = dz64 * torch.where(pre > 0, 1.0, 0.0 if act == "relu" else SLOPE)
    del pre
    stats = torch.stack([_chunk_sums(u.view(n, vox, c), tps), _chunk_sums((u * y64).view(n, vox, c), tps)], -1).float().contiguous()
    del u
    assert stats.shape == (n, tps, c, 2)
    dy, dgamma, dbeta = ops.gn_act_bwd_tiles(stats, dz, y, ss, mr, gamma, G, act, slope=0.01)
    t0, t1, a0, a1 = _tile_totals(stats)
    mean, r = mr[..., 0].double().repeat_interleave(c // G, 1), mr[..., 1].double().repeat_interleave(c // G, 1)
    s1, s2 = t0, r * (t1 - mean * t0)
    b1, b2 = a0, r * (a1 + mean.abs() * a0)
    rule = 2.0 ** -24 * math.sqrt(tps)
    res = _gn_bwd_ref(dz64, dz64, y, ss, mr, gamma, act, sums=(s1, s2, b1, b2, b1 * rule, b2 * rule))
    _check_gn_bwd(res, dtype, dy, dgamma, dbeta, n_sum=n * tps)


# =====================================================================================================================
# EvoNorm-S0 family
# =====================================================================================================================
def _evo_params(g, n, c):
    mr = torch.stack([0.1 * _randn(g, (n, G)), _rand(g, (n, G))], -1).contiguous()
    gamma = _rand(g, (c,))
    beta = 0.3 * _randn(g, (c,))
    return mr, gamma, beta


def _se_params(g, c):
    ch = c // 2
    return 0.3 * _randn(g, (ch, c)), 0.2 * _randn(g, (ch,)), 0.3 * _randn(g, (c, ch)), 0.2 * _randn(g, (c,))


def _evo_num(y64):
    """num = x * sigmoid(x) and its derivative"""
    sg = torch.sigmoid(y64)
    return y64 * sg, sg * (1.0 + y64 * (1.0 - sg))


EVO_CASES = [(BF, 1, False), (BF, 2, True), (HF, 1, False), (HF, 2, True)]


@pytest.mark.parametrize("dtype,n,big", EVO_CASES)
def test_evonorm(dtype, n, big):
    """brats_evonorm_fwd with the channel sums and |max|: z = x * sigmoid(x) * rstd_g * gamma_c + beta_c on 1024 blocks per
    sample (gx = 4182), plain and NT.  z against f64 (M = |num * rstd * gamma| + |beta|), sum_v z by the sum rule (n = V),
    |max| == max |z|; z of the big form == z of the normal form per sample."""
    from brats21_amd import ops
    g = _gen(107)
    c = 48
    vox = S[0] * S[1] * S[2]
    y = _side(_randn(g, (n, *S, c), dtype), big)
    mr, gamma, beta = _evo_params(g, n, c)
    amax = torch.zeros(1, device=y.device)
    z, cs = ops.evonorm(y, mr, gamma, beta, G, want_chansum=True, amax=amax)
    num, _ = _evo_num(y.double())
    t = num * (_gbc(mr[..., 1], c) * gamma.double())
    m = t.abs() + beta.double().abs()
    ref = t.add_(beta.double())
    _check_elem("z", z, ref, m, dtype)
    _check_sum("chansum", cs, _vsum(ref), vox, _vsum(m))
    assert float(amax) == float(z.abs().max())
    del num, t, m, ref
    if big:
        for i in range(2):
            z_i, _ = ops.evonorm(_side(_cut(y, i), False), _cutp(mr, i), gamma, beta, G, want_chansum=True)
            assert torch.equal(z_i, _cut(z, i)), f"sample {i}: big form != normal form"


def _dot_tol(abs_terms, length):
    """f32 dot product of `length` terms: 2^-24 * sqrt(length) * sum|t| (the sum rule)."""
    return abs_terms * (2.0 ** -24 * math.sqrt(length))


def _se_fwd_ref(cs, dcs, vox, w1, b1, w2, b2):
    """f64 ResidualSELayer gate on the channel sums cs [N, C] (gap = cs / V, hid = relu(W1 gap + b1), gate = sigmoid(W2 hid +
    b2)) and the tolerance of 1 + gate given |delta cs| <= dcs: relu and sigmoid are 1- and 1/4-Lipschitz, each small dot product
    adds the sum rule's slack, the sigmoid and the final 1 + gate (a value in [1, 2]) two f32 steps."""
    w1, b1, w2, b2 = (t.double() for t in (w1, b1, w2, b2))
    gap = cs / vox
    hid_pre = gap @ w1.t() + b1
    hid = hid_pre.clamp_min(0)
    t_hid = (dcs / vox) @ w1.abs().t() + _dot_tol(gap.abs() @ w1.abs().t() + b1.abs(), w1.shape[1] + 1)
    lin = hid @ w2.t() + b2
    t_lin = t_hid @ w2.abs().t() + _dot_tol(hid.abs() @ w2.abs().t() + b2.abs(), w2.shape[1] + 1)
    gate = torch.sigmoid(lin)
    # exp(-lin) through v_exp_f32 carries |lin| * 2^-23 of relative error (argument scaling) + an ulp; d gate = gate * (1 - gate) * ...
    t_gate = 0.25 * (t_lin + (lin.abs() + 2.0) * 2.0 ** -23) + 2.0 ** -22
    return 1.0 + gate, hid, t_gate, t_hid


@pytest.mark.parametrize("n,big", [(1, False), (2, True)])
def test_evonorm_se(n, big):
    """brats_evonorm_se_fwd (bf16): the num-sum pass on 512 / 1024 blocks (unrolled by two + tail), the gate, then the EvoNorm
    pass writing out = z * (1 + gate).  chansum = rstd * gamma * sum num + beta * V by the sum rule; 1 + gate and the hidden
    layer against the f64 gate within what that chansum tolerance allows (_se_fwd_ref); out against f64 GIVEN the returned
    1 + gate (M = |num * rstd * gamma * g| + |beta * g|).
    Bit-equality between the forms: out depends on the block-partitioned sums through the gate, so that run uses W2 = 0
    (gate = sigmoid(b2), independent of the sums): what remains is the per-element pass, NT against plain."""
    from brats21_amd import ops
    g = _gen(108)
    c, dtype = 48, BF
    vox = S[0] * S[1] * S[2]
    y = _side(_randn(g, (n, *S, c), dtype), big)
    mr, gamma, beta = _evo_params(g, n, c)
    w1, b1, w2, b2 = _se_params(g, c)
    amax = torch.zeros(1, device=y.device)
    out, cs, gate1p, hidden = ops.evonorm_se(y, mr, gamma, beta, w1, b1, w2, b2, G, amax=amax)
    num, _ = _evo_num(y.double())
    rg = mr[..., 1].double().repeat_interleave(c // G, 1) * gamma.double()  # [N, C]
    numsum, numabs = _vsum(num), _vsum(num.abs())
    cs_ref = rg * numsum + beta.double() * vox
    cs_abs = rg * numabs + beta.double().abs() * vox
    _check_sum("chansum", cs, cs_ref, vox, cs_abs, extra=cs_abs * 2.0 ** -22)  # (+ the f32 map from sum num to sum z)
    g_ref, h_ref, t_gate, t_hid = _se_fwd_ref(cs_ref, cs_abs * (2.0 ** -24 * math.sqrt(vox) + 2.0 ** -22), vox, w1, b1, w2, b2)
    for name, got, ref, tol in (("1 + gate", gate1p, g_ref, t_gate), ("hidden", hidden, h_ref, t_hid)):
        worst = float(((got.double() - ref).abs() / tol).max())
        print(f"  {name}: worst |got - ref| / bound = {worst:.3f}")
        assert worst <= 1.0, (name, worst)
    t = num * _bc(rg * gate1p.double())
    bg = _bc(beta.double()[None] * gate1p.double())
    m = t.abs() + bg.abs()
    _check_elem("out", out, t.add_(bg), m, dtype)
    assert float(amax) == float(out.abs().max())
    del num, t, m
    if big:
        w2z = torch.zeros_like(w2)
        out0, _, g0, _ = ops.evonorm_se(y, mr, gamma, beta, w1, b1, w2z, b2, G)
        for i in range(2):
            o_i, _, g_i, _ = ops.evonorm_se(_side(_cut(y, i), False), _cutp(mr, i), gamma, beta, w1, b1, w2z, b2, G)
            assert torch.equal(g_i, _cutp(g0, i)), "the gate of W2 = 0 does not depend on the sums"
            assert torch.equal(o_i, _cut(out0, i)), f"sample {i}: big form != normal form"


def _evo_bwd_ref(gr, grabs, y64, mr, gamma, q, qtol, dgr=None):
    """f64 statement of EvoNorm's pass 2 (csrc/norm.hip evonorm_bwd_apply_kernel):
        dx = gr * gamma * r * num'(x) - r^3 * A_g / (M - 1) * (x - mean_g),  A_g = sum_{c in g} q_c,  M = cpg * V
    gr: the gradient the pass reads (dz * gscale + gadd), grabs the absolute sum of its terms, dgr its own tolerance (from
    gadd); q [N, C] = gamma_c * sum_v gr * num with tolerance qtol.  Terms of M_dx: gr * gamma * r * num', and x and mean times
    the cpg terms r^3 * q_c / (M - 1); d dx / d A = -r^3 * (x - mean) / (M - 1).  -> (dx, M_dx, extra, A, sum|q|, tol(A)) """
    n, c = q.shape
    cpg = c // G
    vox = y64[0, ..., 0].numel()
    mean, r = _gbc(mr[..., 0], c), _gbc(mr[..., 1], c)
    _, dnum = _evo_num(y64)

    def grp(t):
        return t.view(n, G, cpg).sum(2).repeat_interleave(cpg, 1)

    k3 = r ** 3 / (cpg * vox - 1.0)
    a, aabs, atol = grp(q), grp(q.abs()), grp(qtol)
    w = dnum * (r * gamma.double())
    ref = gr * w - (y64 - mean) * (k3 * _bc(a))
    m = grabs * w.abs() + (y64.abs() + mean.abs()) * (k3 * _bc(aabs))
    extra = (y64 - mean).abs_() * (k3 * _bc(atol))
    if dgr is not None:
        extra += w.abs_() * dgr
    return ref, m, extra, a, aabs, atol


def _evo_dcb_ref(s3, s3tol, a, aabs, atol, sumx, mr, gamma, c, vox):
    """dconvbias[c] = sum_n gamma_c * r * S3 - r^3 * A_g / (M - 1) * (sum_v x - V * mean_g): the tolerance carries the two
    sums' own and 2^-21 of the absolute terms (a chain of up to eight f32 operations at half an ulp each)."""
    gm = gamma.double()
    mean, r = mr[..., 0].double().repeat_interleave(c // G, 1), mr[..., 1].double().repeat_interleave(c // G, 1)
    k3 = r ** 3 / ((c // G) * vox - 1.0)
    ref = (gm * r * s3 - k3 * a * (sumx - vox * mean)).sum(0)
    tol = (gm.abs() * r * s3tol + k3 * atol * (sumx - vox * mean).abs()).sum(0)
    tol += 2.0 ** -21 * ((gm * r * s3).abs() + k3 * aabs * (sumx.abs() + vox * mean.abs())).sum(0)
    return ref, tol


EVOBWD_CASES = [  # dtype, N, C, big, with gscale / gadd
    (BF, 1, 48, False, False), (BF, 2, 48, True, False), (BF, 1, 96, True, False), (HF, 1, 48, False, False), (HF, 2, 48, True, True),
]


@pytest.mark.parametrize("dtype,n,c,big,mapped", EVOBWD_CASES)
def test_evonorm_bwd(dtype, n, c, big, mapped):
    """brats_evonorm_bwd with the forward's channel sums (dconvbias), once with the folded gradient map dz * gscale + gadd:
    pass 1 on 512 / 1024 blocks (three sums; unrolled by two + tail), pass 2 on 2048 / 8192 blocks."""
    from brats21_amd import ops
    g = _gen(109)
    vox = S[0] * S[1] * S[2]
    y = _side(_randn(g, (n, *S, c), dtype), big)
    dz = _randn(g, (n, *S, c), dtype, positive=True)
    mr, gamma, _ = _evo_params(g, n, c)
    gs = _rand(g, (n, c)) if mapped else None
    ga = 0.05 * _randn(g, (n, c)).abs() if mapped else None
    y64 = y.double()
    chan = torch.stack([_vsum(y64), _vsum(y64 * y64)], -1).contiguous()
    amax = torch.zeros(1, device=y.device)
    dy, dgamma, dbeta, dcb = ops.evonorm_bwd(dz, y, mr, gamma, G, chan=chan, amax=amax, gscale=gs, gadd=ga)
    assert float(amax) == float(dy.abs().max())
    gr = dz.double()
    if mapped:
        gr = gr * _bc(gs) + _bc(ga)  # (every term positive: gr is its own absolute sum)
    num, dnum = _evo_num(y64)
    rule = 2.0 ** -24 * math.sqrt(vox)
    s1, s2, s3 = _vsum(gr), _vsum(gr * num), _vsum(gr * dnum)
    a2, a3 = _vsum(gr * num.abs()), _vsum(gr * dnum.abs())
    del num, dnum
    gm = gamma.double()
    ref, m, extra, a, aabs, atol = _evo_bwd_ref(gr, gr, y64, mr, gamma, s2 * gm, a2 * gm.abs() * rule)
    _check_elem("dy", dy, ref, m, dtype, extra=extra)
    del ref, m, extra
    r = mr[..., 1].double().repeat_interleave(c // G, 1)
    _check_sum("dbeta", dbeta, s1.sum(0), n * vox, s1.sum(0))
    _check_sum("dgamma", dgamma, (s2 * r).sum(0), n * vox, (a2 * r).sum(0))
    dcb_ref, dcb_tol = _evo_dcb_ref(s3, a3 * rule, a, aabs, atol, chan[..., 0], mr, gamma, c, vox)
    worst = float(((dcb.double() - dcb_ref).abs() / dcb_tol).max())
    print(f"  dconvbias: worst |got - ref| / bound = {worst:.3f}")
    assert worst <= 1.0, worst


@pytest.mark.parametrize("n,tps,big", [(1, 5488, False), (2, 5488, True), (1, 130, False)])
def test_evonorm_bwd_tiles(n, tps, big):
    """brats_evonorm_bwd_tiles (bf16): the tile statistics are (sum dz, sum dz * z) over consecutive chunks of the voxels, z =
    num * rstd * gamma + beta the EvoNorm output (in f64 here, cast to f32 per tile); the f64 slab reduction gives S1 and
    gamma_c * sum dz * num = (sum T1 - beta_c * sum T0) / rstd_g, pass 2 (512 / 2048 blocks, unrolled by two + tail) writes dx and
    takes the two sums that are not linear in z (sum dz * num for dgamma, sum dz * num' for dconvbias) itself."""
    from brats21_amd import ops
    g = _gen(110)
    c, dtype = 48, BF
    vox = S[0] * S[1] * S[2]
    y = _side(_randn(g, (n, *S, c), dtype), big)
    dz = _randn(g, (n, *S, c), dtype, positive=True)
    mr, gamma, beta = _evo_params(g, n, c)
    y64, gr = y.double(), dz.double()
    chan = torch.stack([_vsum(y64), _vsum(y64 * y64)], -1).contiguous()
    num, dnum = _evo_num(y64)
    r = mr[..., 1].double().repeat_interleave(c // G, 1)
    z64 = num * _bc(r * gamma.double()) + beta.double()
    stats = torch.stack([_chunk_sums(gr.view(n, vox, c), tps), _chunk_sums((gr * z64).view(n, vox, c), tps)], -1).float().contiguous()
    del z64
    dy, dgamma, dbeta, dcb = ops.evonorm_bwd_tiles(stats, dz, y, mr, gamma, beta, G, chan=chan)
    t0, t1, a0, a1 = _tile_totals(stats)
    rule_t, rule_v = 2.0 ** -24 * math.sqrt(tps), 2.0 ** -24 * math.sqrt(vox)
    p = (t1 - beta.double() * t0) / r               # = gamma_c * sum dz * num, what pass 2 adds up per group
    ptol = (a1 + beta.double().abs() * a0) / r * rule_t
    ref, m, extra, a, aabs, atol = _evo_bwd_ref(gr, gr, y64, mr, gamma, p, ptol)
    _check_elem("dy", dy, ref, m, dtype, extra=extra)
    del ref, m, extra
    _check_sum("dbeta", dbeta, t0.sum(0), n * tps, a0.sum(0))
    s2, a2 = _vsum(gr * num), _vsum(gr * num.abs())
    s3, a3 = _vsum(gr * dnum), _vsum(gr * dnum.abs())
    _check_sum("dgamma", dgamma, (s2 * r).sum(0), n * vox, (a2 * r).sum(0))
    dcb_ref, dcb_tol = _evo_dcb_ref(s3, a3 * rule_v, a, aabs, atol, chan[..., 0], mr, gamma, c, vox)
    worst = float(((dcb.double() - dcb_ref).abs() / dcb_tol).max())
    print(f"  dconvbias: worst |got - ref| / bound = {worst:.3f}")
    assert worst <= 1.0, worst


SEBWD_CASES = [  # N, C, big, pool form (None / with_avg)
    (1, 48, False, None), (2, 48, True, None), (1, 96, True, None), (1, 48, False, False), (2, 48, True, True),
]


@pytest.mark.parametrize("n,c,big,pool", SEBWD_CASES)
def test_evonorm_se_bwd(n, c, big, pool):
    """brats_evonorm_se_bwd and its pool= form (bf16): pass 1 with five raw sums R0..R4 = sum do, do * num, do * num', num, num'
    on 512 / 1024 blocks, the SE backward on the sums, pass 2 on 2048 / 8192 blocks reading dz = do * (1 + gate) + gadd.
    f64, with the forward's (1 + gate, hidden, chansum) as given inputs (tests/test_assp_gpu.py's restatement of the SE layer):
        dgate = r * gamma * R1 + beta * R0;  ds = dgate * g * (1 - g);  dh = (ds W2) * [hidden > 0];  gadd = dh W1 / V;
        dW2 = ds^T hidden, db2 = sum_n ds, dW1 = dh^T gap, db1 = sum_n dh;
        S1 = g1p * R0 + gadd * V, S2 = g1p * R1 + gadd * R3, S3 = g1p * R2 + gadd * R4, then EvoNorm's pass 2 (_evo_bwd_ref).
    Every tolerance is the sum rule on R0..R4 (n = V) pushed through these maps with absolute values, each small dot product
    adding the sum rule for its own length."""
    from brats21_amd import ops
    g = _gen(111)
    dtype = BF
    vox = S[0] * S[1] * S[2]
    y = _side(_randn(g, (n, *S, c), dtype), big)
    mr, gamma, beta = _evo_params(g, n, c)
    w1, b1, w2, b2 = _se_params(g, c)
    out, cs, gate1p, hidden = ops.evonorm_se(y, mr, gamma, beta, w1, b1, w2, b2, G, apply=pool is not None)
    y64 = y.double()
    chan = torch.stack([_vsum(y64), _vsum(y64 * y64)], -1).contiguous()
    if pool is None:
        do = _randn(g, (n, *S, c), dtype, positive=True)
        got = ops.evonorm_se_bwd(do, y, mr, gamma, beta, cs, hidden, gate1p, w1, w2, G, chan=chan)
        do64 = do.double()
        doabs = do64
    else:
        ops.maxpool2(out, pool, want_argmax=True)
        idx = out._pool_argmax
        dskip = _randn(g, (n, *S, c), dtype, positive=True)
        dpool = _randn(g, (n, S[0] // 2, S[1] // 2, S[2] // 2, c * (2 if pool else 1)), dtype, positive=True)
        got = ops.evonorm_se_bwd(None, y, mr, gamma, beta, cs, hidden, gate1p, w1, w2, G, chan=chan, pool=(dskip, dpool, idx, pool))
        do64, doabs = _pool_dz(dskip, dpool, idx, with_avg=pool)
    del out
    dy, dgamma, dbeta, dcb, dw1, db1, dw2, db2 = got
    num, dnum = _evo_num(y64)
    rule = 2.0 ** -24 * math.sqrt(vox)
    rr = [_vsum(do64), _vsum(do64 * num), _vsum(do64 * dnum), _vsum(num), _vsum(dnum)]
    ra = [rr[0], _vsum(doabs * num.abs()), _vsum(doabs * dnum.abs()), _vsum(num.abs()), _vsum(dnum.abs())]
    rt = [q * rule for q in ra]
    del num, dnum
    gm, bt = gamma.double(), beta.double()
    r = mr[..., 1].double().repeat_interleave(c // G, 1)
    g1p, hid = gate1p.double(), hidden.double()
    w1d, w2d = w1.double(), w2.double()
    ch = w1.shape[0]
    dgate = r * gm * rr[1] + bt * rr[0]
    dgate_abs = r * gm.abs() * ra[1] + bt.abs() * ra[0]
    t_dgate = r * gm.abs() * rt[1] + bt.abs() * rt[0] + dgate_abs * 2.0 ** -22
    gg = (g1p - 1.0) * (2.0 - g1p)
    ds, ds_abs, t_ds = dgate * gg, dgate_abs * gg, t_dgate * gg + dgate_abs * gg * 2.0 ** -22
    hmask = (hid > 0).double()
    dh = (ds @ w2d) * hmask
    dh_abs = (ds_abs @ w2d.abs()) * hmask
    t_dh = (t_ds @ w2d.abs()) * hmask + _dot_tol(dh_abs, c)
    gadd = dh @ w1d / vox
    gadd_abs = dh_abs @ w1d.abs() / vox
    t_gadd = t_dh @ w1d.abs() / vox + _dot_tol(gadd_abs, ch) + gadd_abs * 2.0 ** -23
    gap = cs.double() / vox
    small = (("dW2", dw2, ds.t() @ hid, t_ds.t() @ hid.abs() + _dot_tol(ds_abs.t() @ hid.abs(), n)),
             ("db2", db2, ds.sum(0), t_ds.sum(0) + _dot_tol(ds_abs.sum(0), n)),
             ("dW1", dw1, dh.t() @ gap, t_dh.t() @ gap.abs() + _dot_tol(dh_abs.t() @ gap.abs(), n) + (dh_abs.t() @ gap.abs()) * 2.0 ** -23),
             ("db1", db1, dh.sum(0), t_dh.sum(0) + _dot_tol(dh_abs.sum(0), n)))
    for name, a_, ref_, tol_ in small:
        tol_ = tol_ + ref_.abs() * 2.0 ** -23  # (the stored f32 itself)
        worst = float(((a_.double() - ref_).abs() / tol_.clamp_min(1e-300)).max())
        print(f"  {name}: worst |got - ref| / bound = {worst:.3f}")
        assert worst <= 1.0, (name, worst)
    s1 = g1p * rr[0] + gadd * vox
    s2 = g1p * rr[1] + gadd * rr[3]
    s3 = g1p * rr[2] + gadd * rr[4]
    s1abs = g1p * ra[0] + gadd_abs * vox
    s2abs = g1p * ra[1] + gadd_abs * ra[3]
    s3abs = g1p * ra[2] + gadd_abs * ra[4]
    t_s1 = g1p * rt[0] + t_gadd * vox + s1abs * 2.0 ** -22
    t_s2 = g1p * rt[1] + gadd_abs * rt[3] + t_gadd * ra[3] + s2abs * 2.0 ** -22
    t_s3 = g1p * rt[2] + gadd_abs * rt[4] + t_gadd * ra[4] + s3abs * 2.0 ** -22
    gr = do64 * _bc(g1p) + _bc(gadd)
    grabs = doabs * _bc(g1p) + _bc(gadd_abs)
    ref, m, extra, a, aabs, atol = _evo_bwd_ref(gr, grabs, y64, mr, gamma, s2 * gm, t_s2 * gm.abs(), dgr=_bc(t_gadd))
    _check_elem("dy", dy, ref, m, dtype, extra=extra)
    del ref, m, extra, gr, grabs
    for name, a_, ref_, tol_ in (("dbeta", dbeta, s1.sum(0), t_s1.sum(0)), ("dgamma", dgamma, (s2 * r).sum(0), (t_s2 * r).sum(0))):
        tol_ = tol_ + ref_.abs() * 2.0 ** -22
        worst = float(((a_.double() - ref_).abs() / tol_).max())
        print(f"  {name}: worst |got - ref| / bound = {worst:.3f}")
        assert worst <= 1.0, (name, worst)
    dcb_ref, dcb_tol = _evo_dcb_ref(s3, t_s3, a, aabs, atol, chan[..., 0], mr, gamma, c, vox)
    worst = float(((dcb.double() - dcb_ref).abs() / dcb_tol).max())
    print(f"  dconvbias: worst |got - ref| / bound = {worst:.3f}")
    assert worst <= 1.0, worst


# =====================================================================================================================
# channel_dot, channel_scale, up-sampling, PReLU slope gradient
# =====================================================================================================================
@pytest.mark.parametrize("n,big", [(1, False), (2, True)])
def test_channel_dot(n, big):
    """brats_channel_dot (bf16), one and two operands: 512 / 1024 blocks, unrolled by two + tail; the sum rule with n = V."""
    from brats21_amd import ops
    g = _gen(112)
    c = 48
    vox = S[0] * S[1] * S[2]
    a = _side(_randn(g, (n, *S, c), BF, positive=True), big)
    b = _randn(g, (n, *S, c), BF, positive=True)
    ref1 = _vsum(a.double())
    _check_sum("sum a", ops.channel_dot(a), ref1, vox, ref1)
    ref2 = _vsum(a.double() * b.double())
    _check_sum("sum a * b", ops.channel_dot(a, b), ref2, vox, ref2)


@pytest.mark.parametrize("n,big", [(1, False), (2, True)])
def test_channel_scale(n, big):
    """brats_channel_scale (bf16) with add and |max|: 4096 / 8192 blocks; out = a * scale + add against f64, |max| == max |out|,
    big form == normal form per sample (out, |max|)."""
    from brats21_amd import ops
    g = _gen(113)
    c = 48
    a = _side(_randn(g, (n, *S, c), BF), big)
    sc, ad = _rand(g, (n, c)), 0.3 * _randn(g, (n, c))
    amax = torch.zeros(1, device=a.device)
    out = ops.channel_scale(a, sc, add=ad, amax=amax)
    t = a.double() * _bc(sc)
    m = t.abs() + _bc(ad).abs()
    _check_elem("out", out, t.add_(_bc(ad)), m, BF)
    del t, m
    assert float(amax) == float(out.abs().max())
    if big:
        am = []
        for i in range(2):
            a_i = torch.zeros(1, device=a.device)
            o_i = ops.channel_scale(_side(_cut(a, i), False), _cutp(sc, i), add=_cutp(ad, i), amax=a_i)
            assert torch.equal(o_i, _cut(out, i)), f"sample {i}: big form != normal form"
            am.append(float(a_i))
        assert float(amax) == max(am)


def _lerp(in_len, out_len, dev):
    """torch's align_corners=True coefficients as f32 arithmetic produces them (area_pixel_compute_source_index): scale =
    (in - 1) / (out - 1), src = scale * o, i0 = (int) src, i1 = i0 + (i0 < in - 1), w1 = src - i0, w0 = 1 - w1."""
    scale = torch.tensor(float(in_len - 1), dtype=F32) / torch.tensor(float(out_len - 1), dtype=F32)
    src = scale * torch.arange(out_len, dtype=F32)
    i0 = src.to(torch.int64).clamp_(max=in_len - 1)
    i1 = i0 + (i0 < in_len - 1)
    w1 = (src - i0.float()).clamp_(0.0, 1.0)
    w0 = 1.0 - w1
    return i0.to(dev), i1.to(dev), w0.double().to(dev), w1.double().to(dev)


def _upsample_ref(x64):
    """f64 trilinear x2, one axis after the other, with the f32 coefficients above."""
    for dim in (1, 2, 3):
        i0, i1, w0, w1 = _lerp(x64.shape[dim], 2 * x64.shape[dim], x64.device)
        shape = [1] * x64.dim()
        shape[dim] = -1
        x64 = x64.index_select(dim, i0) * w0.view(shape) + x64.index_select(dim, i1) * w1.view(shape)
    return x64


UP_CASES = [  # dtype, N, input size, C, big, LDS-staged
    (BF, 1, (56, 56, 56), 48, False, True), (BF, 2, (56, 56, 56), 48, True, True),
    (BF, 1, (48, 48, 40), 96, False, False), (BF, 2, (48, 48, 40), 96, True, False),
    (HF, 1, (56, 56, 56), 48, False, True), (HF, 2, (56, 56, 56), 48, True, True),
    (HF, 1, (48, 48, 40), 96, False, False), (HF, 2, (48, 48, 40), 96, True, False),
]


@pytest.mark.parametrize("dtype,n,size,c,big,ldsx", UP_CASES)
def test_upsample_x2(dtype, n, size, c, big, ldsx):
    """brats_upsample_fwd, scale 2: the LDS-staged form (12 * W * C * 2 B <= 80 KiB) and the plain form, each with plain and
    non-temporal stores (switch on the OUTPUT's bytes).  y against the f64 interpolation with torch's f32 coefficients (M = the
    same interpolation of |x|); the big form's sample n == the normal form on x[n]."""
    from brats21_amd import ops
    g = _gen(114)
    assert (12 * size[2] * c * 2 <= 80 * 1024) == ldsx
    x = _randn(g, (n, *size, c), dtype)
    y = _side(ops.upsample(x, 2), big)
    x64 = x.double()
    _check_elem("y", y, _upsample_ref(x64), _upsample_ref(x64.abs()), dtype)
    del x64
    if big:
        for i in range(n):
            y_i = _side(ops.upsample(x[i].unsqueeze(0), 2), False)
            assert torch.equal(y_i, y[i].unsqueeze(0)), f"sample {i}: big form != normal form"


@pytest.mark.parametrize("dtype,n,size", [(BF, 1, S), (BF, 2, S), (F32, 1, S32), (BF, 2, (8, 8, 8)), (F32, 2, (8, 8, 8))])
def test_prelu_slope_grad(dtype, n, size):
    """brats_prelu_slope_grad = sum over (n, voxel, channel) of dz * min(y * scale + shift, 0): grid capped at 1024 blocks per
    sample (gx = 4182 at 112^3, 3048 for f32 at 80^3), per-block partials added in order; one block at 8^3.  dz > 0 makes every
    term <= 0: the sum rule with n = N * V * C."""
    from brats21_amd import ops
    g = _gen(115)
    c = 48
    y = _randn(g, (n, *size, c), dtype)
    dz = _randn(g, (n, *size, c), dtype, positive=True)
    ss = _affine_params(g, n, c)
    got = ops.prelu_slope_grad(dz, y, ss)
    _, _, pre = _affine_ref(y, ss, "relu")
    ref = (pre.clamp_max_(0.0) * dz.double()).sum().reshape(1)
    _check_sum("dslope", got, ref, y.numel(), ref.abs())


# =====================================================================================================================
# exact counts: every term exactly 1, so a voxel dropped, counted twice or never written shows with ==
# =====================================================================================================================
def _ones_gn(n, c, dev):
    ss = torch.zeros((n, c, 2), device=dev)
    ss[..., 0] = 1.0
    mr = torch.zeros((n, G, 2), device=dev)
    mr[..., 1] = 1.0
    return ss, mr, torch.ones(c, device=dev)


@pytest.mark.parametrize("n,big", [(1, False), (2, True)])
def test_exact_count_gn_act_bwd(n, big):
    """dz = y = 1, scale = 1, shift = 0, mean = 0, rstd = 1, gamma = 1: u = xhat = 1, so dbeta = dgamma = N * V exactly (2,809,856 <
    2^24: f32 sums of ones are exact in any order) and dy = 1 - m1 - m2 = -1 at every voxel (bf16 absorbs the rounding of 1 / M)."""
    from brats21_amd import ops
    dev = _dev()
    c, vox = 48, S[0] * S[1] * S[2]
    one = _side(torch.ones((n, *S, c), dtype=BF, device=dev), big)
    ss, mr, gamma = _ones_gn(n, c, dev)
    dy, dgamma, dbeta = ops.gn_act_bwd(one, one, ss, mr, gamma, G, "relu")
    assert bool((dbeta == n * vox).all()) and bool((dgamma == n * vox).all()), (dbeta, dgamma)
    assert bool((dy == -1.0).all())


@pytest.mark.parametrize("n,big", [(1, False), (2, True)])
def test_exact_count_gn_act_bwd_pool(n, big):
    """dskip = 0, dpool = 1, y = 1 with RANDOM arg-max bytes: every pooled (voxel, channel) hands its 1 to exactly one voxel of its
    window, so dbeta = dgamma = N * V / 8 exactly, m1 = m2 = 1 / 8 and dy = 0.75 where the byte selects the voxel, -0.25
    elsewhere."""
    from brats21_amd import ops
    dev = _dev()
    c, vox = 48, S[0] * S[1] * S[2]
    one = _side(torch.ones((n, *S, c), dtype=BF, device=dev), big)
    ss, mr, gamma = _ones_gn(n, c, dev)
    ps = (n, S[0] // 2, S[1] // 2, S[2] // 2, c)
    idx = torch.randint(0, 8, ps, generator=_gen(116), device=dev, dtype=torch.uint8)
    dskip, dpool = torch.zeros_like(one), torch.ones(ps, dtype=BF, device=dev)
    dy, dgamma, dbeta = ops.gn_act_bwd_pool(dskip, dpool, idx, one, ss, mr, gamma, G, "relu")
    assert bool((dbeta == n * vox // 8).all()) and bool((dgamma == n * vox // 8).all()), (dbeta, dgamma)
    dz, _ = _pool_dz(dskip, dpool, idx)
    assert torch.equal(dy, (dz - 0.25).to(BF))


@pytest.mark.parametrize("n,big", [(1, False), (2, True)])
def test_exact_count_evonorm_bwd(n, big):
    """dz = 1, x = 0, gamma = rstd = 1, mean = 0: sum dz = N * V exactly (dbeta), sum dz * num = 0 exactly (dgamma, A_g), and
    dx = num'(0) = 1 / 2 at every voxel."""
    from brats21_amd import ops
    dev = _dev()
    c, vox = 48, S[0] * S[1] * S[2]
    one = _side(torch.ones((n, *S, c), dtype=BF, device=dev), big)
    _, mr, gamma = _ones_gn(n, c, dev)
    dy, dgamma, dbeta, _ = ops.evonorm_bwd(one, torch.zeros_like(one), mr, gamma, G)
    assert bool((dbeta == n * vox).all()) and bool((dgamma == 0).all()), (dbeta, dgamma)
    assert bool((dy == 0.5).all())


@pytest.mark.parametrize("n,big", [(1, False), (2, True)])
def test_exact_count_channel_dot(n, big):
    from brats21_amd import ops
    vox = S[0] * S[1] * S[2]
    one = _side(torch.ones((n, *S, 48), dtype=BF, device=_dev()), big)
    assert bool((ops.channel_dot(one) == vox).all()) and bool((ops.channel_dot(one, one) == vox).all())


@pytest.mark.parametrize("dtype", [BF, F32])
def test_exact_count_prelu_slope_grad(dtype):
    """dz = 1, y = -1, scale = 1, shift = 0: every term is -1.  The total, -N * V * C = -134,873,088, is beyond 2^24, but every
    per-block partial is a multiple of 48 (whole voxels x 48 channels) below 2^24 and every partial sum a multiple of 16 below
    2^28, where f32 steps by 16: exact in any order."""
    from brats21_amd import ops
    dev = _dev()
    n, c, vox = 2, 48, S[0] * S[1] * S[2]
    one = torch.ones((n, *S, c), dtype=dtype, device=dev)
    ss, _, _ = _ones_gn(n, c, dev)
    assert float(ops.prelu_slope_grad(one, -one, ss)) == -float(n * vox * c)


# =====================================================================================================================
# statistics finalize: the one-launch form up to 32768 (tile, channel) pairs per group, two launches beyond
# =====================================================================================================================
FINALIZE_CASES = [  # C, tiles per sample, mean / std of the data
    (48, 5461, 0.3),    # 32766 pairs: the last direct case
    (48, 5462, 0.3),    # 32772 pairs: the first two-stage case (85 slabs -> 64 of 86, last short)
    (48, 8192, 30.0),   # the 128^3 level itself, 64 slabs; mean = 30 x std: E[x^2] - mean^2 cancels 3 digits
    (384, 700, 0.3),    # cpg 48, two-stage, 10 slabs
    (8, 40000, 0.3),    # cpg 1, two-stage, slab cap
    (2048, 129, 0.3),   # cpg 256 (the widest group the argument check admits), two slabs of 65 and 64 tiles
]


@pytest.mark.parametrize("c,tps,offset", FINALIZE_CASES)
def test_finalize(c, tps, offset):
    """brats_gn_finalize and brats_evonorm_finalize (unbiased variance; its f64 channel totals too) on synthetic tile statistics,
    N = 2, 64 voxels per tile.  The kernels add in f64 and round once, so against f64 sums of the same f32 statistics: mean and
    rstd within 2 f32 ulps, scale = rstd * gamma within 3, shift within 2^-22 * (|beta| + |mean * scale|), the channel totals
    within 1e-13 * sum|t|."""
    from brats21_amd import ops
    g = _gen(117 + c + tps)
    n, k = 2, 64
    vox = tps * k
    cpg = c // G
    m_t = offset + 0.1 * _randn(g, (n, tps, c)).double()      # per-tile mean and variance of a channel
    v_t = _rand(g, (n, tps, c)).double()
    stats = torch.stack([k * m_t, k * (v_t + m_t * m_t)], -1).float().contiguous()
    del m_t, v_t
    assert (tps * cpg <= 32768) == ((c, tps) == (48, 5461))
    gamma, beta = 1.0 + 0.3 * _randn(g, (c,)), 0.2 * _randn(g, (c,))
    t = stats.double()
    tot, tot_abs = t.sum(1), t.abs().sum(1)                      # [N, C, 2]
    cnt = float(cpg * vox)
    gs = tot.view(n, G, cpg, 2).sum(2)
    mean = gs[..., 0] / cnt
    var = (gs[..., 1] / cnt - mean * mean).clamp_min(0.0)
    eps = float(torch.tensor(1e-5, dtype=F32))

    def close(name, got, ref, ulps):
        worst = float(((got.double() - ref).abs() / _ulps(ref)).max())
        print(f"  {name}: worst error {worst:.2f} f32 ulps (bound {ulps})")
        assert worst <= ulps, (name, worst)

    for unbiased in (False, True):
        rstd = 1.0 / torch.sqrt((var * cnt / (cnt - 1.0) if unbiased else var) + eps)
        if unbiased:
            mr, chan = ops.evonorm_finalize(stats, n, c, G, vox)
            err = (chan[:n * c * 2].view(n, c, 2) - tot).abs() / tot_abs
            print(f"  channel totals: worst |got - ref| / sum|t| = {float(err.max()):.2e}")
            assert float(err.max()) <= 1e-13
        else:
            mr, ss = ops.gn_finalize(stats, n, c, G, vox, gamma, beta)
            sc = rstd.repeat_interleave(cpg, 1) * gamma.double()
            mc = mean.repeat_interleave(cpg, 1)
            close("scale", ss[..., 0], sc, 3)
            sh_err = (ss[..., 1].double() - (beta.double() - mc * sc)).abs() / (beta.double().abs() + (mc * sc).abs())
            print(f"  shift: worst |got - ref| / (|beta| + |mean * scale|) = {float(sh_err.max()) * 2 ** 22:.3f} x 2^-22")
            assert float(sh_err.max()) <= 2.0 ** -22
        close("mean" + ("" if not unbiased else " (unbiased)"), mr[..., 0], mean, 2)
        close("rstd" + ("" if not unbiased else " (unbiased)"), mr[..., 1], rstd, 2)
