"""Exact integer-operand references for the convolution kernels (tests/test_conv_exact_cpu.py, tests/test_conv_exact_gpu.py,
tests/test_first_layer_gpu.py, tests/test_dconv_exact_gpu.py).

The technique: every element of x, dy, w (and the bias) is a small integer, exact in bf16, fp16, f32, e4m3 and in the hi
half of a split-precision pair.  Every product is then an integer, and while the worst-case sum of absolute values stays
below 2^24 every partial sum in every summation order is exactly representable in f32: a kernel's f32 result must equal the
reference BIT FOR BIT whatever its split-K schedule, slab order or MFMA shape, and a 16-bit output is the round-to-nearest-
even of an exact integer.  The bounds are preconditions asserted on the operands / the reference alone (require_*).

The references are float64 shifted GEMMs, one per tap, independent of torch's convolution.  Activations are channels-last
[N, D, H, W, C] CPU float32 tensors (the layout the kernels read), weights torch's [Cout, Cin, k, k, k].

The second half mirrors the host selection rules of csrc/conv_wgrad.hip (wgrad_nlane, wgrad_split_g8, wgrad_blocks_g8,
wgrad_tiles, wgrad_plan, wgrad_reduce_launch) -- the arithmetic is copied, so that a change of a rule makes the
GPU tests fail (their mirrored workspace size no longer equals the library's) instead of quietly exercising another branch."""
import functools
import math
from types import SimpleNamespace

import torch

EXACT = float(2 ** 24)  # integers up to here are exact in f32


# ------------------------------------------------------------------------------------------ operands
def int_tensor(shape, seed, density=1.0, amax=2):
    """Seeded CPU float32 tensor with integer values in [-amax, amax]; an element is non-zero with probability `density`
    (non-zero values uniform over -amax..-1, 1..amax).  density = 1: uniform over -amax..amax (zero included)."""
    g = torch.Generator().manual_seed(seed)
    if density >= 1.0:
        return torch.randint(-amax, amax + 1, shape, generator=g).float()
    mag = torch.randint(1, amax + 1, shape, generator=g).float()
    sign = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
    keep = (torch.rand(shape, generator=g) < density).float()
    return mag * sign * keep


def stats_density(cin, voxels, amax_x=2, amax_w=1):
    """A density of x at which the EXPECTED per-(n, channel) total of y^2 of a 3x3x3 layer is 2^22 (a quarter of the bound
    require_stats_exact asserts), for dense weights uniform over -amax_w..amax_w.  Derived from the operand distributions
    only: E[y^2] = 27 cin density E[x^2 | x != 0] E[w^2]."""
    ex2 = sum(v * v for v in range(1, amax_x + 1)) / amax_x
    ew2 = sum(v * v for v in range(-amax_w, amax_w + 1)) / (2 * amax_w + 1)
    return min(1.0, 2.0 ** 22 / (voxels * 27.0 * cin * ex2 * ew2))


# ------------------------------------------------------------------------------------------ preconditions
def require_wgrad_exact(x, dy, x2=None):
    """Weight / bias gradient: K max|x| max|dy| < 2^24 with K = n d h w (every partial sum over voxels is an exact integer)."""
    k = dy.shape[0] * dy.shape[1] * dy.shape[2] * dy.shape[3]
    ax = float(x.abs().max()) if x2 is None else max(float(x.abs().max()), float(x2.abs().max()))
    bound = k * max(ax, 1.0) * max(float(dy.abs().max()), 1.0)
    for t in (x, dy) + (() if x2 is None else (x2,)):
        assert bool((t == t.round()).all()), "operands must be integers"
    assert bound < EXACT, f"weight-gradient precondition violated: K max|x| max|dy| = {bound:.0f} >= 2^24"


def require_fwd_exact(x, w, bias=None, x2=None):
    """Forward / input gradient: taps (cin + cin2) max|x| max|w| + max|bias| < 2^24."""
    cin = x.shape[-1] + (x2.shape[-1] if x2 is not None else 0)
    taps = w.shape[2] * w.shape[3] * w.shape[4]
    ax = float(x.abs().max()) if x2 is None else max(float(x.abs().max()), float(x2.abs().max()))
    bound = taps * cin * max(ax, 1.0) * max(float(w.abs().max()), 1.0) + (float(bias.abs().max()) if bias is not None else 0.0)
    for t in (x, w) + (() if x2 is None else (x2,)) + (() if bias is None else (bias,)):
        assert bool((t == t.round()).all()), "operands must be integers"
    assert bound < EXACT, f"forward precondition violated: taps cin max|x| max|w| + |bias| = {bound:.0f} >= 2^24"


def require_sum_exact(y_ref):
    """Per-(n, channel) sum of y: exact when the total of |y| is below 2^24 (it bounds every partial sum)."""
    tot = float(y_ref.abs().sum((1, 2, 3)).max())
    assert tot < EXACT, f"statistics precondition violated: per-(n, channel) sum of |y| = {tot:.0f} >= 2^24"


def require_stats_exact(y_ref):
    """Per-(n, channel) sum of y^2: all terms are non-negative, so every partial sum is bounded by the total."""
    tot = float((y_ref.double() ** 2).sum((1, 2, 3)).max())
    assert tot < EXACT, f"statistics precondition violated: per-(n, channel) sum of y^2 = {tot:.0f} >= 2^24"


def stats_exact_ok(y_ref):
    return float((y_ref.double() ** 2).sum((1, 2, 3)).max()) < EXACT


# ------------------------------------------------------------------------------------------ float64 shifted-GEMM references
def _taps(k, dil):
    """[(tap index in torch's k x k x k order, (dz, dy, dx) voxel offset)]"""
    if k == 1:
        return [(0, (0, 0, 0))]
    return [((a * 3 + b) * 3 + c, ((a - 1) * dil, (b - 1) * dil, (c - 1) * dil)) for a in range(3) for b in range(3) for c in range(3)]


def _cat(x, x2):
    return x if x2 is None else torch.cat([x, x2], -1)


def _padded(x, r):
    """float64 copy of the channels-last x with r zero voxels on every face."""
    n, d, h, w, c = x.shape
    xp = torch.zeros((n, d + 2 * r, h + 2 * r, w + 2 * r, c), dtype=torch.float64)
    xp[:, r:r + d, r:r + h, r:r + w] = x.double()
    return xp


def wgrad_ref(x, dy, dil=1, k=3, x2=None):
    """dW[co][ci][tap] = sum_v dy[v][co] * [x | x2][v + off(tap)][ci]: one float64 GEMM dy^T @ x_shifted per tap."""
    x = _cat(x, x2)
    n, d, h, w, c = x.shape
    co = dy.shape[-1]
    r = dil if k == 3 else 0
    xp = _padded(x, r)
    dyt = dy.double().reshape(-1, co).t().contiguous()
    out = torch.empty((co, c, k ** 3), dtype=torch.float64)
    for t, (oz, oy, ox) in _taps(k, dil):
        xs = xp[:, r + oz:r + oz + d, r + oy:r + oy + h, r + ox:r + ox + w].reshape(-1, c)
        out[:, :, t] = dyt @ xs
    return out.reshape(co, c, k, k, k)


def dbias_ref(dy):
    return dy.double().sum((0, 1, 2, 3))


def fwd_ref(x, wt, bias=None, dil=1, x2=None):
    """y[v][co] = bias[co] + sum_tap [x | x2][v + off(tap)] @ wt[:, :, tap]^T, channels-last float64."""
    x = _cat(x, x2)
    n, d, h, w, c = x.shape
    co, k = wt.shape[0], wt.shape[2]
    r = dil if k == 3 else 0
    xp = _padded(x, r)
    wm = wt.double().reshape(co, c, k ** 3)
    y = torch.zeros((n * d * h * w, co), dtype=torch.float64)
    for t, (oz, oy, ox) in _taps(k, dil):
        xs = xp[:, r + oz:r + oz + d, r + oy:r + oy + h, r + ox:r + ox + w].reshape(-1, c)
        y += xs @ wm[:, :, t].t()
    if bias is not None:
        y += bias.double()
    return y.reshape(n, d, h, w, co)


def dgrad_ref(dy, wt, dil=1):
    """dx[v + off(tap)][ci] += dy[v] @ wt[:, :, tap]: the forward loop transposed (a scatter into a padded dx), float64."""
    n, d, h, w, co = dy.shape
    c, k = wt.shape[1], wt.shape[2]
    r = dil if k == 3 else 0
    wm = wt.double().reshape(co, c, k ** 3)
    dxp = torch.zeros((n, d + 2 * r, h + 2 * r, w + 2 * r, c), dtype=torch.float64)
    dym = dy.double().reshape(-1, co)
    for t, (oz, oy, ox) in _taps(k, dil):
        dxp[:, r + oz:r + oz + d, r + oy:r + oy + h, r + ox:r + ox + w] += (dym @ wm[:, :, t]).reshape(n, d, h, w, c)
    return dxp[:, r:r + d, r:r + h, r:r + w].contiguous()


def tile_sums_ref(y_ref):
    """(sum y, sum y^2) per (n, channel) of the unrounded result: [n, cout] float64 each."""
    yd = y_ref.double()
    return yd.sum((1, 2, 3)), (yd * yd).sum((1, 2, 3))


# ------------------------------------------------------------------------------------------ the comparison
def assert_exact(got, ref, dtype=None, what=""):
    """`got` (any device) equals the float64 reference bit for bit: `ref` is cast to f32 (exact under the preconditions) and,
    for a 16-bit kernel output, rounded to `dtype` (round to nearest even, as the kernels' conversions do).  The one
    comparison of the CPU and the GPU tests; a mismatch reports how many entries differ and the first of them."""
    want = ref.float()
    assert torch.equal(want.double(), ref.double()), f"{what}: the reference itself is not exact in f32"
    if dtype is not None and dtype != torch.float32:
        want = want.to(dtype)
    g = got.detach().cpu()
    assert g.shape == want.shape, f"{what}: shape {tuple(g.shape)} != {tuple(want.shape)}"
    assert g.dtype == want.dtype, f"{what}: dtype {g.dtype} != {want.dtype}"
    if torch.equal(g, want):
        return
    bad = (g.float() != want.float()) | (g.float().isnan() != want.float().isnan())
    idx = bad.nonzero()
    first = tuple(int(i) for i in idx[0])
    raise AssertionError(f"{what}: {idx.shape[0]} of {bad.numel()} entries differ; first at {first}: got {float(g[first])}, "
                         f"want {float(want[first])}")


def assert_stats_exact(stats, y_ref, squares=True, what=""):
    """The tile statistics [N, tiles, cout, 2] summed over the tiles in float64 equal the reference's sums exactly."""
    s = stats.detach().double().sum(1).cpu()
    r1, r2 = tile_sums_ref(y_ref)
    require_sum_exact(y_ref)
    assert torch.equal(s[..., 0], r1), f"{what}: sum of y differs at {int((s[..., 0] != r1).sum())} of {r1.numel()} (n, channel) entries"
    if squares:
        require_stats_exact(y_ref)
        assert torch.equal(s[..., 1], r2), f"{what}: sum of y^2 differs at {int((s[..., 1] != r2).sum())} of {r2.numel()} entries"


TILE_Z, TILE_Y, TILE_X = 4, 4, 16  # the statistics tile of every convolution kernel (CONV_TZ, CONV_TY, CONV_TX of csrc/conv_igemm.hpp)


def tile_stats_ref(y_ref):
    """(sum y, sum y^2) of the unrounded result per 4x4x16 tile: float64 [N, tz * ty * tx, cout, 2] in the library's tile order
    (x fastest, then y, then z); the tiles at the far faces of a ragged volume are clipped to it."""
    n, d, h, w, c = y_ref.shape
    tz, ty, tx = -(-d // TILE_Z), -(-h // TILE_Y), -(-w // TILE_X)
    yp = torch.zeros((n, tz * TILE_Z, ty * TILE_Y, tx * TILE_X, c), dtype=torch.float64)
    yp[:, :d, :h, :w] = y_ref.double()
    yt = yp.reshape(n, tz, TILE_Z, ty, TILE_Y, tx, TILE_X, c)
    return torch.stack([yt.sum((2, 4, 6)), (yt * yt).sum((2, 4, 6))], -1).reshape(n, tz * ty * tx, c, 2)


@functools.lru_cache(maxsize=None)
def _tile_stats_cached(y_ref):
    """(tile_stats_ref, the largest per-(tile, channel) sum of |y|) of a shared, unchanged reference (keyed by the tensor object)."""
    return tile_stats_ref(y_ref), float(tile_stats_ref(y_ref.double().abs())[..., 0].max())


def tile_stats_exact_ok(y_ref, squares=True):
    """The precondition of assert_tile_stats_exact: per (tile, channel) the sum of |y| -- and, with squares, of y^2 -- is below
    2^24, which bounds every partial sum of either in any order."""
    ref, tot = _tile_stats_cached(y_ref)
    return tot < EXACT and (not squares or float(ref[..., 1].max()) < EXACT)


def assert_tile_stats_exact(stats, y_ref, squares=True, what=""):
    """The tile statistics [N, tiles, cout, 2] equal the reference's per-tile sums entry by entry.  assert_stats_exact adds the
    tiles up first, so sums written to another tile's slot of the same sample pass it; here they do not."""
    ref, tot = _tile_stats_cached(y_ref)
    assert tot < EXACT, f"tile statistics precondition violated: per-(tile, channel) sum of |y| = {tot:.0f} >= 2^24"
    s = stats.detach().double().cpu()
    assert s.shape == ref.shape, f"{what}: statistics shape {tuple(s.shape)} != {tuple(ref.shape)}"

    def compare(e, name):
        if not torch.equal(s[..., e], ref[..., e]):
            bad = (s[..., e] != ref[..., e]).nonzero()
            first = tuple(int(i) for i in bad[0])
            raise AssertionError(f"{what}: per-tile sum of {name} differs at {bad.shape[0]} of {ref[..., e].numel()} (n, tile, channel) "
                                 f"entries; first at {first}: got {float(s[..., e][first])}, want {float(ref[..., e][first])}")
    compare(0, "y")
    if squares:
        tot2 = float(ref[..., 1].max())
        assert tot2 < EXACT, f"tile statistics precondition violated: per-(tile, channel) sum of y^2 = {tot2:.0f} >= 2^24"
        compare(1, "y^2")


# ------------------------------------------------------------------------------------------ mirror of csrc/conv_igemm_first.hpp
FIRST_MIN_TILES = 2048  # CONV_FIRST_MIN_TILES: the default of brats_conv3d_set_first_min_tiles


def first_walk(ntiles, ncu):
    """The tile walk of conv_first_kernel as conv_launch_first starts it on a device of `ncu` CUs -- the arithmetic of the
    launcher's grid line and of the kernel's three walk lines (per_xcd / wg_per_xcd, t_lo / t_hi, the loop) copied.
    -> namespace(grid, per_xcd, wg_per_xcd, slices = [(t_lo, t_hi)] per XCD, tiles = [[tile, ...]] per workgroup, trips)."""
    assert ntiles >= 8
    grid = max(min(ntiles, 2 * ncu) & ~7, 8)
    per_xcd, wg_per_xcd = (ntiles + 7) >> 3, grid >> 3
    slices = [(x * per_xcd, min(ntiles, x * per_xcd + per_xcd)) for x in range(8)]
    tiles = []
    for b in range(grid):
        t_lo, t_hi = slices[b & 7]
        tiles.append(list(range(t_lo + (b >> 3), t_hi, wg_per_xcd)))
    return SimpleNamespace(ntiles=ntiles, grid=grid, per_xcd=per_xcd, wg_per_xcd=wg_per_xcd, slices=slices, tiles=tiles,
                           trips=[len(t) for t in tiles])


def first_layer_form(n, size, min_tiles=FIRST_MIN_TILES, dense=True, aligned=True, stats=True, vs8=True):
    """"first" | "vs8" | "tile": what conv_launch<bf16_t, 3, 1> does with an 8 -> 48 layer (conv_first_ok, then the ck == 8 rule)."""
    d, h, w = size
    ntiles = n * ceil_div(d, TILE_Z) * ceil_div(h, TILE_Y) * ceil_div(w, TILE_X)
    if dense and aligned and stats and d % 4 == 0 and h % 4 == 0 and w % 16 == 0 and ntiles >= 8 and ntiles >= min_tiles:
        return "first"
    return "vs8" if vs8 and ntiles >= min_tiles else "tile"


def ntiles_of(n, size):
    return n * ceil_div(size[0], TILE_Z) * ceil_div(size[1], TILE_Y) * ceil_div(size[2], TILE_X)


# the volumes of tests/test_first_layer_gpu.py, named by their tile count: n, (d, h, w)
FIRST_WALKS = {8: (1, (8, 16, 16)), 9: (1, (12, 12, 16)), 36: (2, (8, 12, 48)), 525: (1, (20, 28, 240)), 1170: (1, (36, 52, 160))}
FIRST_NOBIAS = (36, 1170)                               # these run without a bias as well
FIRST_RAGGED = [(2, (9, 21, 37)), (1, (12, 20, 40))]    # no whole tiles / H a multiple of 4 and not of 8: the slice kernel only
FIRST_DEFAULT = [(1, (36, 60, 272)), (1, (36, 52, 240))]  # 2295 and 1755 tiles: above and below the default threshold


def first_walk_properties(ntiles, n, ncu):
    """What the volume with `ntiles` tiles (FIRST_WALKS, FIRST_DEFAULT[0]) is in the tests for, evaluated on the walk a device of
    `ncu` CUs makes: [(description, holds)].  The GPU tests assert every one as a precondition -- on a device with another CU count
    a shape that no longer exercises its property fails there by name and is not silently weaker."""
    w = first_walk(ntiles, ncu)
    tps = ntiles // n
    lens = [max(hi - lo, 0) for lo, hi in w.slices]
    xcd = [[w.trips[b] for b in range(x, w.grid, 8)] for x in range(8)]  # trip counts of each XCD's workgroups, in walk order
    once = sorted(t for ts in w.tiles for t in ts) == list(range(ntiles))
    props = [("the mirrored walk visits every tile exactly once", once)]
    if ntiles == 8:
        props += [("grid 8", w.grid == 8), ("one tile per workgroup: no prefetch anywhere", set(w.trips) == {1})]
    elif ntiles == 9:
        props += [("grid 8, below 2 * CUs", w.grid == 8 < 2 * ncu), ("per_xcd 2", w.per_xcd == 2),
                  ("XCDs 0-3 do two tiles (both halo buffers), XCD 4 one", w.trips[:5] == [2, 2, 2, 2, 1]),
                  ("XCDs 5-7 have t_lo > ntiles", all(lo > ntiles for lo, _ in w.slices[5:]) and w.trips[5:] == [0, 0, 0])]
    elif ntiles == 36:
        props += [("grid 32 (ntiles & ~7), below 2 * CUs", w.grid == 32 < 2 * ncu), ("per_xcd 5 over 4 workgroups", (w.per_xcd, w.wg_per_xcd) == (5, 4)),
                  ("unequal trip counts inside an XCD", xcd[0] == [2, 1, 1, 1]),
                  ("a slice crosses the sample boundary", any(lo < tps < hi for lo, hi in w.slices)),
                  ("the last slice has one tile and three idle workgroups", lens[7] == 1 and xcd[7] == [1, 0, 0, 0])]
    elif ntiles == 525:
        props += [("grid capped at 2 * CUs", w.grid == 2 * ncu < ntiles), ("per_xcd no multiple of the workgroups", w.per_xcd % w.wg_per_xcd != 0),
                  ("one or two tiles per workgroup in the full slices", set(xcd[0]) == {1, 2}),
                  ("the last slice is shorter than its workgroups: the last one has no tile", 0 < lens[7] < w.wg_per_xcd and xcd[7][-1] == 0)]
    elif ntiles == 1170:
        props += [("grid capped at 2 * CUs", w.grid == 2 * ncu), ("two and three tiles per workgroup", set(w.trips) == {2, 3}),
                  ("the last slice is shorter", 0 < lens[7] < w.per_xcd)]
    elif ntiles == 2295:
        props += [("an odd tile count at or above the default threshold", ntiles % 2 == 1 and ntiles >= FIRST_MIN_TILES),
                  ("four and five tiles per workgroup", set(w.trips) == {4, 5}), ("the last slice is one tile shorter", lens[7] == w.per_xcd - 1)]
    else:
        raise AssertionError(f"no walk properties written down for {ntiles} tiles")
    return props


# ------------------------------------------------------------------------------------------ mirror of csrc/conv_wgrad.hip
WG_TZ, WG_TY, WG_TX = 4, 4, 16


def ceil_div(a, b):
    return (a + b - 1) // b


def wgrad_ntiles(n, d, h, w):
    return n * ceil_div(d, WG_TZ) * ceil_div(h, WG_TY) * ceil_div(w, WG_TX)


def wgrad_nlane(ntiles):
    nl = 8
    while nl > 1 and ntiles // nl < 16:
        nl >>= 1
    return nl


def wgrad_g8(ntiles, cotiles, citiles, ntaps_planes=3):
    nl = wgrad_nlane(ntiles)
    g8 = ceil_div(512, ntaps_planes * nl * cotiles * citiles)
    g8 = min(g8, ceil_div(ntiles, nl))
    return max(g8, 1)


def wgrad_tiles(f32, c1, c2, cout):
    """(COF, CIF): 16-channel fragments per co / ci tile."""
    co16 = ceil_div(cout, 16)
    cof = 3 if co16 % 3 == 0 else (2 if co16 % 2 == 0 else 1)
    if f32:
        return cof, 1
    a, b = ceil_div(c1, 16), (ceil_div(c2, 16) if c2 > 0 else 0)

    def ok(f):
        return a % f == 0 and (b == 0 or b % f == 0)

    return cof, (3 if ok(3) else (2 if ok(2) else 1))


def wgrad_alltaps_ok(mode, bits16, dil, c1, c2, cout, ntiles, ncu):
    """None, or (g8, kernel name) of the all-taps form the library takes (mode = brats_conv3d_set_wgrad_alltaps)."""
    cin = c1 + max(c2, 0)
    narrow = c2 <= 0 and c1 <= 16
    if not mode or not bits16 or dil != 1:
        return None
    wide = False
    if cout % 48 or (not narrow and (c1 % 48 or (c2 > 0 and c2 % 48))):
        if cout % 64 or (not narrow and (c1 % 32 or (c2 > 0 and c2 % 32))):
            return None
        wide = True
    blocks = (cout // 64) * (1 if narrow else cin // 32) if wide else (cout // 48) * (1 if narrow else cin // 48)
    nl = wgrad_nlane(ntiles)
    g8 = max(ceil_div(ncu, nl * blocks), 1)
    if ntiles < 4 * nl * g8:
        return None
    if wide and narrow:
        name = "alltaps_kernel<1, 4>"
    elif wide:
        name = "alltaps2<4, 2>"
    elif narrow and c1 % 8 == 0:
        name = "alltaps2<3, 1>"
    elif narrow:
        name = "alltaps_kernel<1>"
    else:
        name = "alltaps2<3, 3>"
    return g8, name


def wgrad_reduce_kind(cout, cin, taps):
    tblocks = (cout * cin // 4 + 31) // 32
    return "reduce_taps" if (1 < taps <= 32 and tblocks >= 256) else "reduce"


def wgrad_plan(bits16, dil, c1, c2, cout, n, d, h, w, mode, ncu):
    """What brats_conv3d_wgrad does with a 3x3x3 layer: dict(kernel, cof, cif, nlane, nsplit, reduce, ws_bytes, memset)."""
    c2 = max(c2, 0)
    ntiles = wgrad_ntiles(n, d, h, w)
    cof, cif = wgrad_tiles(not bits16, c1, c2, cout)
    cot = ceil_div(cout, 16 * cof)
    cit = ceil_div(c1, 16 * cif) + (ceil_div(c2, 16 * cif) if c2 > 0 else 0)
    nl = wgrad_nlane(ntiles)
    ns_tap = nl * wgrad_g8(ntiles, cot, cit)
    at = wgrad_alltaps_ok(mode, bits16, dil, c1, c2, cout, ntiles, ncu)
    at1 = wgrad_alltaps_ok(mode, bits16, 1, c1, c2, cout, ntiles, ncu)  # (the workspace size does not know the dilation)
    ns_ws = max(ns_tap, nl * at1[0]) if at1 else ns_tap
    plan = dict(ntiles=ntiles, cof=cof, cif=cif, nlane=nl, reduce=wgrad_reduce_kind(cout, c1 + c2, 27),
                ws_bytes=ns_ws * 27 * cout * (c1 + c2) * 4)
    if at:
        plan.update(kernel=at[1], nsplit=nl * at[0], memset=False)
    else:
        plan.update(kernel=f"tapplane<{'16' if bits16 else 'f32'}, {dil}, {cof}, {cif}>", nsplit=ns_tap,
                    memset=bool((c1 + c2) % 16 or cout % 16))
    return plan


def wgrad_shift_plan(bits16, ksize, cin, cout, n, d, h, w):
    """brats_conv3d_wgrad_shift (wgrad_plan, shifted): one workgroup per tap, so the 512-workgroup rule divides by ntaps."""
    ntiles = wgrad_ntiles(n, d, h, w)
    ntaps = 27 if ksize == 3 else 1
    cof, cif = wgrad_tiles(not bits16, cin, 0, cout)
    cot, cit = ceil_div(cout, 16 * cof), ceil_div(cin, 16 * cif)
    nl = wgrad_nlane(ntiles)
    ns = nl * wgrad_g8(ntiles, cot, cit, ntaps)
    return dict(ntiles=ntiles, cof=cof, cif=cif, nlane=nl, nsplit=ns, reduce=wgrad_reduce_kind(cout, cin, ntaps),
                kernel=f"shift<{'16' if bits16 else 'f32'}, {cof}, {cif}>", memset=bool(cin % 16 or cout % 16),
                ws_bytes=ns * ntaps * cout * cin * 4)


def smallest_alltaps_volume(c1, c2, cout, ncu, ragged=False):
    """(n, (d, h, w)) with the fewest voxels at which the mirror says the all-taps form is taken on a device of `ncu` CUs."""
    if ragged:
        ds, hs, ws = (6, 10, 18, 34), (6, 14, 30, 62), (18, 34, 66)
    else:
        ds, hs, ws = (4, 8, 16, 32), (4, 8, 16, 32, 64), (16, 32, 64)
    best = None
    for n in (1, 2, 3):
        for d in ds:
            for h in hs:
                for w in ws:
                    if wgrad_alltaps_ok(1, True, 1, c1, c2, cout, wgrad_ntiles(n, d, h, w), ncu):
                        key = (n * d * h * w, n, d, h, w)
                        if best is None or key < best:
                            best = key
    assert best is not None, f"no candidate volume selects the all-taps form for {c1}+{c2} -> {cout} at {ncu} CUs"
    return best[1], best[2:]


# ------------------------------------------------------------------------------------------ shared, unchanged references
@functools.lru_cache(maxsize=None)
def wgrad_case(c1, c2, cout, n, size, dil=1, k=3, seed=0):
    """(x, x2 | None, dy, dW float64, dbias float64) of one weight-gradient problem; computed once, shared, never modified."""
    x = int_tensor((n, *size, c1), 1000 + seed)
    x2 = int_tensor((n, *size, c2), 2000 + seed) if c2 else None
    dy = int_tensor((n, *size, cout), 3000 + seed)
    require_wgrad_exact(x, dy, x2)
    return x, x2, dy, wgrad_ref(x, dy, dil, k, x2), dbias_ref(dy)


@functools.lru_cache(maxsize=None)
def fwd_case(c1, c2, cout, n, size, dil=1, k=3, seed=0, thin=False, with_bias=True, real_cin=None):
    """(x, x2 | None, w, bias | None, y float64) of one forward problem.  thin: x at stats_density(), w in {-1, 0, 1}, so that
    the sum of y^2 meets its bound.  real_cin: channels [real_cin, c1) of x and w are zero (the padded first layer)."""
    vox = size[0] * size[1] * size[2]
    dens = stats_density(c1 + c2, vox) if thin else 1.0
    x = int_tensor((n, *size, c1), 4000 + seed, dens)
    x2 = int_tensor((n, *size, c2), 5000 + seed, dens) if c2 else None
    w = int_tensor((cout, c1 + c2, k, k, k), 6000 + seed, 1.0, 1 if thin else 2)
    if real_cin is not None:
        x[..., real_cin:] = 0
        w[:, real_cin:] = 0
    bias = int_tensor((cout,), 7000 + seed) if with_bias else None
    require_fwd_exact(x, w, bias, x2)
    return x, x2, w, bias, fwd_ref(x, w, bias, dil, x2)


@functools.lru_cache(maxsize=None)
def dgrad_case(cin, cout, n, size, dil=1, k=3, seed=0):
    """(dy, w, dx float64) of one input-gradient problem."""
    dy = int_tensor((n, *size, cout), 8000 + seed)
    w = int_tensor((cout, cin, k, k, k), 9000 + seed)
    require_fwd_exact(dy, w.transpose(0, 1))
    return dy, w, dgrad_ref(dy, w, dil)


# ------------------------------------------------------------------------------------------ direct (gather) convolution, csrc/dconv.hip
# One launch of ops.dconv_run = up to 4 jobs, a job's output = bias + the sum of up to 4 terms, every term with its own input,
# channel count, kernel size and dilation.  The reference of a job is the sum of fwd_ref (or dgrad_ref) over its terms.
#
# 16-bit storage: the kernel rounds its f32 accumulators once, to the storage type.  Integers up to 2^8 (bf16, 8 significand bits)
# and 2^11 (fp16, 11 bits) are exact there, so a case whose reference stays within OUT_BOUND is stored unrounded and a change of
# 1 in any output is visible.  The builders thin the operands for that (below) and assert it on the reference alone.
OUT_BOUND = {torch.bfloat16: 256.0, torch.float16: 2048.0, torch.float32: None}
DCONV_KCH = {torch.bfloat16: 16, torch.float16: 16, torch.float32: 8}  # channels per pipeline step (DcT<T>::KCH)
DCONV_NF, DCONV_WG_VOX = 3, 256     # row fragments of 32 per workgroup; voxels per workgroup (4 waves x 2 fragments of 32)

VOL_RAGGED = (2, (5, 6, 7))     # 420 voxels: partial last workgroup and fragment, fragments across the sample boundary
VOL_TINY = (3, (2, 3, 5))       # 90 voxels: less than one workgroup, whole waves return early
VOL_LINE = (1, (1, 1, 33))      # degenerate z and y: only the x taps survive
VOL_WHOLE = (2, (8, 8, 8))      # 1024 voxels: whole workgroups only
DCONV_VOLUMES = (VOL_RAGGED, VOL_TINY, VOL_LINE, VOL_WHOLE)


def _taps_of(k):
    return 27 if k == 3 else 1


def thin_density(kdim, bound, other=None):
    """The density of two operand sets (x in +-{1, 2}: E[x^2 | x != 0] = 2.5; w in +-1) at which the standard deviation of a
    sum of `kdim` products is bound / 8 -- from the operand distributions alone; the extreme of the 10^5 outputs of a case
    lies near 4.5 standard deviations.  other: the density of one set is given, that of the second is returned."""
    if bound is None:
        return 1.0
    var = (bound / 8.0) ** 2
    if other is None:
        return min(1.0, math.sqrt(var / (2.5 * kdim)))
    return min(1.0, var / (2.5 * kdim * other))


def require_terms_exact(terms, bias=None):
    """terms: [(x, w as [rows, cin, k, k, k])].  Sum over the terms of taps cin max|x| max|w|, plus max|bias|, below 2^24."""
    bound = float(bias.abs().max()) if bias is not None else 0.0
    for x, w in terms:
        assert x.shape[-1] == w.shape[1], "term: channels of x and w differ"
        bound += w.shape[2] ** 3 * w.shape[1] * max(float(x.abs().max()), 1.0) * max(float(w.abs().max()), 1.0)
        for t in (x, w):
            assert bool((t == t.round()).all()), "operands must be integers"
    assert bias is None or bool((bias == bias.round()).all()), "operands must be integers"
    assert bound < EXACT, f"direct-convolution precondition violated: sum of taps cin max|x| max|w| + |bias| = {bound:.0f} >= 2^24"


def require_within(ref, bound, what=""):
    """The 16-bit condition: max|ref| <= bound (None: f32 storage, no condition), so that the store rounds nothing."""
    if bound is not None:
        m = float(ref.abs().max())
        assert m <= bound, f"{what}: max|reference| = {m:.0f} exceeds {bound:.0f}, the largest range of exact integers of the storage type"


@functools.lru_cache(maxsize=None)
def dconv_case(n, size, jobs, mode="fwd", bound=None, seed=0):
    """One launch.  jobs: up to 4 of (rows, ((cin, k, dil), ... up to 4 terms), with_bias).
    mode "fwd":   term = conv(x [.., cin], w [rows, cin, k, k, k]) at dilation dil (packed PACK_FWD)
    mode "dgrad": term = input gradient of dy [.., cin] through w [cin, rows, k, k, k] (packed PACK_DGRAD)
    bound None (f32 storage): dense operands in [-2, 2].  Otherwise (OUT_BOUND of a 16-bit type) x in [-2, 2] and w in
    {-1, 0, 1} at thin_density() of the job's K, and max|reference| <= bound is asserted.
    Terms (of any job) with the same position and channel count share ONE input tensor (the network's forward: four jobs over
    one x).  -> namespace(n, size, mode, jobs = [namespace(rows, terms = [namespace(x, w, k, dil, cin)], bias, ref float64)])."""
    assert 1 <= len(jobs) <= 4 and all(1 <= len(terms) <= 4 for _, terms, _ in jobs)
    shared = {}
    out = []
    for j, (rows, terms, with_bias) in enumerate(jobs):
        dens = thin_density(sum(_taps_of(k) * cin for cin, k, _ in terms), bound)
        ts = []
        for t, (cin, k, dil) in enumerate(terms):
            if mode == "fwd":
                key = (t, cin)
                if key not in shared:  # (one density for a shared input: that of the first job that uses it)
                    shared[key] = int_tensor((n, *size, cin), 4000 + 100 * seed + 10 * t + cin, dens)
                x = shared[key]
                w = int_tensor((rows, cin, k, k, k), 6000 + 100 * seed + 10 * j + t, dens, 2 if bound is None else 1)
            else:
                x = int_tensor((n, *size, cin), 8000 + 100 * seed + 10 * j + t, dens)
                w = int_tensor((cin, rows, k, k, k), 9000 + 100 * seed + 10 * j + t, dens, 2 if bound is None else 1)
            ts.append(SimpleNamespace(x=x, w=w, k=k, dil=dil, cin=cin))
        bias = int_tensor((rows,), 7000 + 100 * seed + j) if with_bias else None
        if mode == "fwd":
            require_terms_exact([(t.x, t.w) for t in ts], bias)
            ref = sum(fwd_ref(t.x, t.w, None, t.dil) for t in ts)
        else:
            require_terms_exact([(t.x, t.w.transpose(0, 1)) for t in ts], bias)
            ref = sum(dgrad_ref(t.x, t.w, t.dil) for t in ts)
        if bias is not None:
            ref = ref + bias.double()
        require_within(ref, bound, f"dconv_case job {j}")
        out.append(SimpleNamespace(rows=rows, terms=ts, bias=bias, ref=ref))
    return SimpleNamespace(n=n, size=size, mode=mode, jobs=out)


@functools.lru_cache(maxsize=None)
def dconv_split_case(c1, c2, cout, n, size, k, dil, bound=None, seed=0):
    """One weight over two inputs: y = conv([x | x2], w) run as a two-term job with w[:, :c1] over x and w[:, c1:] over x2
    (cin_off / cin_cnt of pack_weights_direct).  -> (x, x2, w, bias, y float64)."""
    dens = thin_density(_taps_of(k) * (c1 + c2), bound)
    x = int_tensor((n, *size, c1), 4500 + seed, dens)
    x2 = int_tensor((n, *size, c2), 5500 + seed, dens)
    w = int_tensor((cout, c1 + c2, k, k, k), 6500 + seed, dens, 2 if bound is None else 1)
    bias = int_tensor((cout,), 7500 + seed)
    require_fwd_exact(x, w, bias, x2)
    y = fwd_ref(x, w, bias, dil, x2)
    require_within(y, bound, "dconv_split_case")
    return x, x2, w, bias, y


def dconv_cases(dtype):
    """name -> arguments of dconv_case, for every launch tests/test_dconv_exact_gpu.py makes in storage type `dtype` (channel
    counts follow the type's KCH).  tests/test_conv_exact_cpu.py builds them all: the builders assert the preconditions."""
    kch, bound = DCONV_KCH[dtype], OUT_BOUND[dtype]
    c = {}
    for n, size in DCONV_VOLUMES:
        v = "x".join(str(s) for s in (n,) + size)
        for s in (1, 2, 3, 4, 7):  # S = cin / KCH steps against a pipeline three deep
            c[f"k1-S{s}-{v}"] = (n, size, ((32, ((s * kch, 1, 1),), s % 2 == 1),), "fwd", bound)
        for dil in (1, 2, 3, 4, 6) if (n, size) in (VOL_RAGGED, VOL_WHOLE) else (1, 2):
            for with_bias in (True, False):
                c[f"k3-d{dil}-{'bias' if with_bias else 'nobias'}-{v}"] = (n, size, ((48, ((2 * kch, 3, dil),), with_bias),), "fwd", bound)
    for n, size in (VOL_RAGGED, VOL_WHOLE):
        v = "x".join(str(s) for s in (n,) + size)
        for rows in (4, 16, 36, 96, 100, 132):
            c[f"rows{rows}-{v}"] = (n, size, ((rows, ((kch, 3, 1),), True),), "fwd", bound)
        net = ((1, 1), (3, 2), (3, 4), (3, 6))
        c[f"net-equal-{v}"] = (n, size, tuple((16, ((32, k, dl),), True) for k, dl in net), "fwd", bound)
        c[f"net-rows-{v}"] = (n, size, tuple((r, ((32, k, dl),), True) for r, (k, dl) in zip((100, 16, 36, 4), net)), "fwd", bound)
        c[f"dgrad-four-{v}"] = (n, size, ((32, tuple((16, k, dl) for k, dl in net), False),), "dgrad", bound)
        mixed = ((16, 1, 1), (48, 3, 3), (32, 3, 6), (kch, 3, 1))
        for nt in (1, 2, 3, 4):
            c[f"dgrad-mixed{nt}-{v}"] = (n, size, ((36, mixed[:nt], False),), "dgrad", bound)
    return c


DCONV_SPLIT_CASES = [(16, 32, 36, VOL_RAGGED, 3, 2), (32, 16, 32, VOL_WHOLE, 3, 4), (16, 48, 100, VOL_RAGGED, 1, 1)]  # c1, c2, cout, volume, k, dil

ASPP_BRANCHES = {  # (kernel sizes, dilations) of SimpleASPPEVO: the default, five (two launches), nine (three launches)
    4: ((1, 3, 3, 3), (1, 2, 4, 6)),
    5: ((1, 3, 3, 3, 3), (1, 1, 2, 4, 6)),
    9: ((1, 3, 3, 3, 3, 1, 3, 3, 3), (1, 1, 2, 4, 6, 1, 2, 4, 6)),
}


@functools.lru_cache(maxsize=None)
def aspp_case(nb, cin, q, n, size, bound=None, seed=0):
    """The ASPP stage with ASPP_BRANCHES[nb]: x [.., cin], per branch w [q, cin, k, k, k] and bias [q], d_acat [.., nb q].
    -> namespace(ks, dils, x, ws, bs, dy, acat, dx, dx_parts, dws, dbs), the references in float64.  dx_parts: the partial input
    gradients of the launches _aspp_bwd makes (four branches each); the network rounds each to the storage type before torch
    adds them, so under a 16-bit bound every partial and the total must stay within it (then the split sum is exact)."""
    ks, dils = ASPP_BRANCHES[nb]
    d_fwd = thin_density(27 * cin, bound)
    x = int_tensor((n, *size, cin), 4700 + seed, d_fwd)
    ws = [int_tensor((q, cin, k, k, k), 6700 + 10 * seed + i, d_fwd, 2 if bound is None else 1) for i, k in enumerate(ks)]
    bs = [int_tensor((q,), 7700 + 10 * seed + i) for i in range(nb)]
    dy = int_tensor((n, *size, nb * q), 8700 + seed, thin_density(sum(_taps_of(k) * q for k in ks), bound, d_fwd))
    dys = [dy[..., i * q:(i + 1) * q] for i in range(nb)]
    for i in range(nb):
        require_fwd_exact(x, ws[i], bs[i])
        require_wgrad_exact(x, dys[i])
    require_terms_exact([(dys[i], ws[i].transpose(0, 1)) for i in range(nb)])
    acat = torch.cat([fwd_ref(x, ws[i], bs[i], dils[i]) for i in range(nb)], -1)
    parts = [sum(dgrad_ref(dys[i], ws[i], dils[i]) for i in range(j0, min(j0 + 4, nb))) for j0 in range(0, nb, 4)]
    dx = sum(parts)
    for what, t in [("acat", acat), ("dx", dx)] + [(f"dx part {i}", p) for i, p in enumerate(parts)]:
        require_within(t, bound, f"aspp_case {what}")
    dws = [wgrad_ref(x, dys[i], dils[i], ks[i]) for i in range(nb)]
    dbs = [dbias_ref(dys[i]) for i in range(nb)]
    return SimpleNamespace(ks=ks, dils=dils, x=x, ws=ws, bs=bs, dy=dy, acat=acat, dx=dx, dx_parts=parts, dws=dws, dbs=dbs)


ASPP_CASES = [(nb, 32, 16, n, size) for nb in (4, 5, 9) for n, size in (VOL_RAGGED, VOL_WHOLE)]  # nb, cin, q, n, size
