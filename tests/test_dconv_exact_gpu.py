"""-m gpu: the direct (gather) convolution of the ASPP head, csrc/dconv.hip (ops.dconv_run, ops.pack_weights_direct), on small
INTEGER operands against the float64 references of tests/_conv_exact_ref.py, bit for bit (no tolerance anywhere in this file).

The kernel stages nothing in LDS: every operand is an unconditional 16-byte buffer load whose offset is forced to all ones when
a tap leaves the volume, a pipeline step lies past the end of the (tap, channel-step) loop or a row fragment is dead, and the
descriptor's range check must return zeros for it.  A wrong mask, a step dropped or doubled at the ends of the three-deep
pipeline, a row fragment mapped to the wrong block or a store past a job's rows changes an integer.

16-bit storage (bf16 and fp16): the case builders thin the operands until max|reference| <= 256 (bf16) / 2048 (fp16); the
kernel's one rounding, at the store, is then the identity, and a change of 1 in any output shows
(tests/test_conv_exact_cpu.py builds every case listed here on the CPU and asserts that condition).  f32 cases keep dense
operands.  Outputs are channel slices of one buffer pre-filled with a sentinel; inputs, where stated, channel slices of buffers
filled with 7.  tests/CONV_EXACT.md, item 9, lists what each case reaches.

Not exercised by a call: the 2 GiB offset guard of brats_dconv_run (a missing guard would mean a wild launch)."""
import pytest
import torch

import _conv_exact_ref as R

pytestmark = pytest.mark.gpu

BF, FH, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = pytest.mark.parametrize("dtype", [BF, FH, F32], ids=["bf16", "fp16", "f32"])
TWO_VOLUMES = pytest.mark.parametrize("vol", [R.VOL_RAGGED, R.VOL_WHOLE], ids=["2x5x6x7", "2x8x8x8"])
SENTINEL = -77.0    # exact in every storage type; no reference value of a 16-bit case is excluded by it (it is compared by position)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _vname(vol):
    return "x".join(str(s) for s in (vol[0],) + vol[1])


def _case(dtype, name):
    return R.dconv_case(*R.dconv_cases(dtype)[name])


def _dv(t, dtype):
    d = t.to(_dev()).to(dtype)
    assert torch.equal(d.float().cpu(), t)  # the operands really are exact in the storage type
    return d


def _sliced(ts, dtype):
    """CPU channels-last tensors -> channel slices, side by side, of ONE buffer filled with 7 whose pitch is the channels + 16:
    8 channels of 7s (16 bytes in 16-bit storage, 32 in f32: what the 16-byte alignment rule allows) before and after."""
    pitch = sum(t.shape[-1] for t in ts) + 16
    buf = torch.full(tuple(ts[0].shape[:4]) + (pitch,), 7.0, dtype=dtype, device=_dev())
    out, off = [], 8
    for t in ts:
        buf[..., off:off + t.shape[-1]] = _dv(t, dtype)
        out.append(buf[..., off:off + t.shape[-1]])
        off += t.shape[-1]
    return out


def _launch(case, dtype, views=False, gap=4, packed=None):
    """One ops.dconv_run of a _conv_exact_ref.dconv_case.  Every job writes its channel slice of ONE buffer pre-filled with
    SENTINEL, `gap` untouched channels before, between and after the slices (gap 0: a dense output).  views: every input is a
    channel slice of a buffer of 7s -- the distinct inputs of a job side by side in one buffer, an input shared by several jobs
    (the network's forward) once.  packed: {(job, term): buffer} replacing what pack_weights_direct returns.
    -> (the whole output buffer, {(job, term): packed weights})."""
    from brats21_amd import ops
    mode = ops.PACK_FWD if case.mode == "fwd" else ops.PACK_DGRAD
    buf = torch.full((case.n, *case.size, gap + sum(j.rows + gap for j in case.jobs)), SENTINEL, dtype=dtype, device=_dev())
    memo, jobs, packs, off = {}, [], {}, gap
    for ji, job in enumerate(case.jobs):
        new = []
        for t in job.terms:
            if id(t.x) not in memo and all(t.x is not u for u in new):
                new.append(t.x)
        if new:
            memo.update({id(x): d for x, d in zip(new, _sliced(new, dtype) if views else [_dv(x, dtype) for x in new])})
        terms = []
        for ti, t in enumerate(job.terms):
            packs[ji, ti] = ops.pack_weights_direct(t.w.to(_dev()), dtype, mode)
            terms.append((memo[id(t.x)], (packed or packs)[ji, ti], t.k, t.dil))
        jobs.append((terms, job.bias.to(_dev()) if job.bias is not None else None, buf[..., off:off + job.rows]))
        off += job.rows + gap
    ops.dconv_run(jobs, case.n, *case.size, dtype)
    torch.cuda.synchronize()
    return buf, packs


def _check(case, buf, dtype, gap=4, what=""):
    """Every job's slice equals its reference; every channel outside the slices still holds the sentinel."""
    off, outside = gap, torch.ones(buf.shape[-1], dtype=torch.bool)
    for ji, job in enumerate(case.jobs):
        R.require_within(job.ref, R.OUT_BOUND[dtype], what)
        R.assert_exact(buf[..., off:off + job.rows], job.ref, dtype, what=f"{what} job {ji} ({job.rows} rows)")
        outside[off:off + job.rows] = False
        off += job.rows + gap
    assert int(outside.sum()) == gap * (len(case.jobs) + 1)
    if gap:
        left = buf.cpu()[..., outside].float()
        assert bool((left == SENTINEL).all()), f"{what}: {int((left != SENTINEL).sum())} entries outside the output slices were written"


def _run(dtype, name, **kw):
    case = _case(dtype, name)
    buf, _ = _launch(case, dtype, **kw)
    _check(case, buf, dtype, kw.get("gap", 4), name)
    return case, buf


# ---------------------------------------------------------------------------------------------- forward, one job and one term
@pytest.mark.parametrize("steps", [1, 2, 3, 4, 7])
@DTYPES
def test_pointwise_forward_at_the_short_ends_of_the_pipeline(dtype, steps):
    """k = 1 at cin = steps * KCH: S = 1 and 2 end inside the three-step prologue (the loop body runs once, multiplying the
    zeros of dropped loads), 3 fills it exactly, 4 and 7 end one step into a round of three.  All four volumes; with a bias for
    odd S, without for even."""
    for vol in R.DCONV_VOLUMES:
        _run(dtype, f"k1-S{steps}-{_vname(vol)}")


@pytest.mark.parametrize("dil", [1, 2, 3, 4, 6])
@TWO_VOLUMES
@DTYPES
def test_dilated_forward_with_and_without_bias(dtype, vol, dil):
    """k = 3 at the dilations of the ASPP branches and at 1 and 3, 48 rows (two row fragments, the third dead), two channel
    steps per tap.  On 2 x (5, 6, 7) dilation 6 leaves the (centre, centre, *) taps only, and those between x = 0 and x = 6."""
    for b in ("bias", "nobias"):
        _run(dtype, f"k3-d{dil}-{b}-{_vname(vol)}")


@DTYPES
def test_forward_on_degenerate_volumes(dtype):
    """3 x (2, 3, 5): 90 voxels, waves 2 and 3 return early and wave 1 ends inside its first fragment; 1 x (1, 1, 33): only the
    x taps survive and the second fragment holds one voxel."""
    for vol in (R.VOL_TINY, R.VOL_LINE):
        for dil in (1, 2):
            for b in ("bias", "nobias"):
                _run(dtype, f"k3-d{dil}-{b}-{_vname(vol)}")


# ---------------------------------------------------------------------------------------------- row counts
@pytest.mark.parametrize("rows", [4, 16, 36, 96, 100, 132])
@DTYPES
def test_row_counts_into_a_slice_of_a_sentinel_buffer(dtype, rows):
    """rows 4 / 16: a tail at a granule of 4 inside the only fragment; 36: inside the second; 96: exactly NF fragments; 100 and
    132: a second blockIdx.y with one and with two live fragments.  The output is a channel slice (4 sentinel channels on either
    side) and nothing outside it may be written."""
    for vol in (R.VOL_RAGGED, R.VOL_WHOLE):
        _run(dtype, f"rows{rows}-{_vname(vol)}")


# ---------------------------------------------------------------------------------------------- forward as the network runs it
@pytest.mark.parametrize("rows", ["equal", "rows"])
@TWO_VOLUMES
@DTYPES
def test_four_jobs_in_one_launch_over_a_sliced_input(dtype, vol, rows):
    """(k, dil) = (1, 1), (3, 2), (3, 4), (3, 6) as four jobs of one launch writing four slices of one buffer, with 16 rows each
    and with 100 / 16 / 36 / 4 rows (grid.y follows the largest; the other jobs' surplus blocks return).  x is ONE channel slice
    (pitch cin + 16, offset 8) of a buffer filled with 7, read by all four jobs."""
    case, _ = _run(dtype, f"net-{rows}-{_vname(vol)}", views=True)
    assert len({id(j.terms[0].x) for j in case.jobs}) == 1


# ---------------------------------------------------------------------------------------------- input gradient
@pytest.mark.parametrize("name", ["dgrad-four", "dgrad-mixed1", "dgrad-mixed2", "dgrad-mixed3", "dgrad-mixed4"])
@DTYPES
def test_input_gradient_terms_summed_in_the_accumulators(dtype, name):
    """One job of PACK_DGRAD terms: the four branch gradients of the network (dy = four slices of one buffer of 7s), and one to
    four terms that differ in channels (16 / 48 / 32 / KCH), kernel size and dilation (1, 3, 6, 1), dense and sliced."""
    for vol in (R.VOL_RAGGED, R.VOL_WHOLE):
        for views in (True, False):
            _run(dtype, f"{name}-{_vname(vol)}", views=views, gap=4 if views else 0)


# ---------------------------------------------------------------------------------------------- cin_off / cin_cnt
@pytest.mark.parametrize("c1,c2,cout,vol,k,dil", R.DCONV_SPLIT_CASES)
@DTYPES
def test_one_weight_packed_in_two_channel_ranges(dtype, c1, c2, cout, vol, k, dil):
    """pack_weights_direct(w, cin_off = 0, cin_cnt = c1) over x and (cin_off = c1, cin_cnt = c2) over x2 as a two-term job
    == fwd_ref(x, w, x2 = x2)."""
    from brats21_amd import ops
    n, size = vol
    x, x2, w, bias, y_ref = R.dconv_split_case(c1, c2, cout, n, size, k, dil, R.OUT_BOUND[dtype])
    wd = w.to(_dev())
    terms = [(_dv(x, dtype), ops.pack_weights_direct(wd, dtype, ops.PACK_FWD, 0, c1), k, dil),
             (_dv(x2, dtype), ops.pack_weights_direct(wd, dtype, ops.PACK_FWD, c1, c2), k, dil)]
    y = torch.full((n, *size, cout), SENTINEL, dtype=dtype, device=_dev())
    ops.dconv_run([(terms, bias.to(_dev()), y)], n, *size, dtype)
    R.assert_exact(y, y_ref, dtype, what="two channel ranges of one weight")
    # (cin_off alone: the tail range without a count)
    assert torch.equal(ops.pack_weights_direct(wd, dtype, ops.PACK_FWD, c1), terms[1][1])


# ---------------------------------------------------------------------------------------------- repeatability and sensitivity
@DTYPES
def test_two_runs_give_identical_bits(dtype):
    case = _case(dtype, "net-rows-2x5x6x7")
    a, _ = _launch(case, dtype, views=True)
    b, _ = _launch(case, dtype, views=True)
    assert torch.equal(a, b)
    _check(case, a, dtype, what="first run")


@DTYPES
def test_one_zeroed_weight_fragment_fails_the_comparison(dtype):
    """The smallest unit the kernel can lose is one 16-byte load: one tap, one group of 8 (f32: 4) channels, one row.  Zeroing
    ONE such fragment of a packed-weight buffer (one whose weights are not all zero) must make assert_exact raise -- in the
    16-bit types too, whose cases are built so that the store rounds nothing.  No kernel is changed."""
    case = _case(dtype, "k3-d2-bias-2x5x6x7")
    buf, packs = _launch(case, dtype)
    _check(case, buf, dtype, what="intact weights")
    frags = packs[0, 0].clone().view(-1, 16)
    live = (frags != 0).any(1).nonzero().flatten()
    assert live.numel() > 16
    frags[live[live.numel() // 2]] = 0
    assert int((frags.view(-1) != packs[0, 0]).sum()) <= 16
    bad, _ = _launch(case, dtype, packed={(0, 0): frags.view(-1)})
    with pytest.raises(AssertionError, match="entries differ"):
        _check(case, bad, dtype, what="one fragment zeroed")
    # the damage is confined to the one row of that fragment
    rows_hit = (bad.float() != buf.float()).any(0).any(0).any(0).any(0).sum()
    assert int(rows_hit) == 1


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_through_ops_come_before_any_launch():
    from brats21_amd import ops
    from brats21_amd._lib import BratsHipError
    dev, (n, size) = _dev(), R.VOL_TINY

    def act(c, dtype=BF, fill=1.0):
        return torch.full((n, *size, c), fill, dtype=dtype, device=dev)

    def pack(rows, cin, k=1, dtype=BF, mode=None):
        return ops.pack_weights_direct(torch.ones((rows, cin, k, k, k), device=dev), dtype, ops.PACK_FWD if mode is None else mode)

    out = act(64, fill=SENTINEL)
    x16, w = act(16), pack(32, 16)
    good = ([(x16, w, 1, 1)], None, out[..., :32])
    refused = {
        "five jobs": lambda: ops.dconv_run([good] * 5, n, *size, BF),
        "no job": lambda: ops.dconv_run([], n, *size, BF),
        "five terms": lambda: ops.dconv_run([([(x16, w, 1, 1)] * 5, None, out[..., :32])], n, *size, BF),
        "no term": lambda: ops.dconv_run([([], None, out[..., :32])], n, *size, BF),
        "cin 24 in bf16, packing": lambda: pack(32, 24),
        "cin 24 in fp16, packing": lambda: pack(32, 24, dtype=FH),
        "cin 12 in f32, packing": lambda: pack(32, 12, dtype=F32),
        "cout 24 in bf16, packing for the input gradient": lambda: pack(24, 32, mode=ops.PACK_DGRAD),
        "cin 24 in bf16, running": lambda: ops.dconv_run([([(act(24), w, 1, 1)], None, out[..., :32])], n, *size, BF),
        "cin 12 in f32, running": lambda: ops.dconv_run([([(act(12, F32), pack(32, 8, dtype=F32), 1, 1)], None,
                                                             act(32, F32, SENTINEL))], n, *size, F32),
        "rows 30": lambda: ops.dconv_run([([(x16, pack(30, 16), 1, 1)], None, out[..., :30])], n, *size, BF),
        "weights packed for other rows": lambda: ops.dconv_run([([(x16, w, 1, 1)], None, out)], n, *size, BF),
        "weights packed for another cin": lambda: ops.dconv_run([([(act(32), w, 1, 1)], None, out[..., :32])], n, *size, BF),
        "weights packed for another kernel size": lambda: ops.dconv_run([([(x16, w, 3, 1)], None, out[..., :32])], n, *size, BF),
        "weights packed for another type": lambda: ops.dconv_run([([(x16, pack(32, 16, dtype=F32), 1, 1)], None, out[..., :32])], n, *size, BF),
        "ksize 2": lambda: ops.dconv_run([([(x16, w, 2, 1)], None, out[..., :32])], n, *size, BF),
        "ksize 2, packing": lambda: pack(32, 16, k=2),
        "dilation 0": lambda: ops.dconv_run([([(x16, pack(32, 16, 3), 3, 0)], None, out[..., :32])], n, *size, BF),
        "output of another volume": lambda: ops.dconv_run([good], n, size[0], size[1], size[2] + 1, BF),
        "input of another type": lambda: ops.dconv_run([([(act(16, FH), w, 1, 1)], None, out[..., :32])], n, *size, BF),
        "bias of another length": lambda: ops.dconv_run([([(x16, w, 1, 1)], torch.zeros(16, device=dev), out[..., :32])], n, *size, BF),
    }
    for what, call in refused.items():
        with pytest.raises(BratsHipError):
            call()
            pytest.fail(f"{what}: not refused")
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()), "a refused call wrote to its output"
    ops.dconv_run([good], n, *size, BF)   # the valid call the refusals were derived from
    assert bool((out[..., :32] == 16).all()) and bool((out[..., 32:] == SENTINEL).all())


# ---------------------------------------------------------------------------------------------- the ASPP stage of the network
class _Host(torch.nn.Module):
    """What _Ctx needs of a model: parameters (for the gradients' names), training mode, no gradient sink."""

    def __init__(self, aspp):
        super().__init__()
        self.aspp = aspp
        self._grad_sink = None


@pytest.mark.parametrize("nb,cin,q,n,size", R.ASPP_CASES, ids=[f"{c[0]}-branches-{_vname(c[3:])}" for c in R.ASPP_CASES])
@DTYPES
def test_aspp_stage_beyond_four_branches(dtype, nb, cin, q, n, size):
    """SimpleASPPEVO with 4 (the control), 5 and 9 branches through the network's own _aspp_fwd / _aspp_bwd and pass context:
    more than four branches split into launches of four, and the input gradient's partials -- each rounded to the storage type --
    are added by torch.  acat, dx, every dW and every db equal their references bit for bit; in 16 bits every partial and the
    running total stay within the range of exact integers (asserted on the reference), so the split sum rounds nothing."""
    from brats21_amd import ops
    from brats21_amd.networks import equiunet_assp as ea
    bound = R.OUT_BOUND[dtype]
    c = R.aspp_case(nb, cin, q, n, size, bound)
    run = torch.zeros_like(c.dx)
    for part in c.dx_parts:
        run = run + part
        R.require_within(part, bound, "partial input gradient")
        R.require_within(run, bound, "running sum of the partials")
    R.require_within(c.acat, bound, "acat")
    aspp = ea.SimpleASPPEVO(cin, q, c.ks, c.dils)
    with torch.no_grad():
        for conv, w, b in zip(aspp.convs, c.ws, c.bs):
            assert conv.weight.shape == w.shape
            conv.weight.copy_(w)
            conv.bias.copy_(b)
    host = _Host(aspp).to(_dev()).train()
    cx = ea._Ctx(host, dtype, will_bwd=True)
    launches = []
    real = ops.dconv_run

    def counted(jobs, *a):
        launches.append((len(jobs), [len(t) for t, _, _ in jobs]))
        return real(jobs, *a)

    x = _dv(c.x, dtype)
    acat = torch.full((n, *size, nb * q), SENTINEL, dtype=dtype, device=_dev())
    ops.dconv_run = counted
    try:
        saved = ea._aspp_fwd(cx, aspp, x, acat)
        dx = ea._aspp_bwd(cx, aspp, saved, _dv(c.dy, dtype))
    finally:
        ops.dconv_run = real
    torch.cuda.synchronize()
    groups = [min(4, nb - j0) for j0 in range(0, nb, 4)]
    assert launches == [(g, [1] * g) for g in groups] + [(1, [g]) for g in groups]
    R.assert_exact(acat, c.acat, dtype, what="acat")
    R.assert_exact(dx, c.dx, dtype, what="dx")
    names = cx.names
    for i, conv in enumerate(aspp.convs):
        R.assert_exact(cx.grads[names[conv.weight]], c.dws[i], what=f"dW of branch {i} (k {c.ks[i]}, dilation {c.dils[i]})")
        R.assert_exact(cx.grads[names[conv.bias]], c.dbs[i], what=f"db of branch {i}")
