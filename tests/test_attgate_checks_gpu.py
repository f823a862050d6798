"""Bad calls of ops.attgate_fwd / ops.attgate_bwd are refused before anything is launched: the stand-in-library method of
tests/test_ops_checks_gpu.py (every entry point with a stream parameter is recorded, not called) on the two wrappers, which live in
brats21_amd/_attgate.py and are therefore not in that file's table.  One valid call each at [2, 8, 8, 8, 16] bf16 with f_int = 8 must
record exactly the expected entry points; then every tensor argument is corrupted, one corruption at a time -- wrong dtype, a partner
of another storage dtype, one sample or one channel vector fewer, a permuted view, a CPU tensor, small operands one element short or
non-contiguous, a wrong out= dtype -- and each must raise with nothing recorded."""
import pytest
import torch

from brats21_amd import _lib, ops
from test_ops_checks_gpu import _StandIn, T, corruptions

pytestmark = pytest.mark.gpu

N, D, C, FI = 2, 8, 16, 8
BF = torch.bfloat16
SHAPES = ((FI, C, 1, 1, 1), (FI,), (FI,), (FI,), (FI, C, 1, 1, 1), (FI,), (FI,), (FI,), (1, FI, 1, 1, 1), (1,), (1,), (1,))
FWD = (["brats_conv3d_pack_weights", "brats_conv3d_fwd", "brats_gn_finalize"] * 2
       + ["brats_attgate_psi_fwd", "brats_attgate_bn1", "brats_attgate_apply_fwd"])
FWD_EVAL = ["brats_conv3d_pack_weights", "brats_conv3d_fwd"] * 2 + ["brats_attgate_psi_fwd", "brats_attgate_bn1", "brats_attgate_apply_fwd"]
BWD = (["brats_attgate_apply_bwd", "brats_attgate_bn1_bwd", "brats_attgate_psi_bwd_stats", "brats_attgate_psi_bwd_finalize",
        "brats_attgate_psi_bwd_apply", "brats_conv3d_wgrad_shift", "brats_channel_dot", "brats_conv3d_wgrad_shift", "brats_channel_dot"]
       + ["brats_conv3d_pack_weights", "brats_conv3d_fwd"] * 2 + ["brats_attgate_dx"])


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


def _act(c=C):
    return torch.zeros((N, D, D, D, c), dtype=BF, device="cuda")


def _f(*shape):
    return torch.zeros(shape, dtype=torch.float32, device="cuda")


def _params():
    return {f"p{i}": T("vec", _f(*s)) for i, s in enumerate(SHAPES)}


def _table():
    tb = {}
    prm = _params()
    run = {f"r{i}": T("vec", _f(k)) for i, k in enumerate((FI, FI, FI, FI, 1, 1))}

    def fwd(g, x, out, **k):
        return ops.attgate_fwd(g, x, [k[f"p{i}"] for i in range(12)], "relu", out=out)

    def fwd_eval(g, x, out, **k):
        return ops.attgate_fwd(g, x, [k[f"p{i}"] for i in range(12)], "relu", training=False, out=out, running=[k[f"r{i}"] for i in range(6)])
    # (g carries the block's f_g: a channel vector fewer is caught by W_g's size)
    tb["attgate_fwd"] = (fwd, dict(g=T("act", _act()), x=T("act", _act()), out=T("out", _act()), **prm), FWD)
    tb["attgate_fwd(eval)"] = (fwd_eval, dict(g=T("act", _act()), x=T("act", _act()), out=T("out", _act()), **prm, **run), FWD_EVAL)
    _, sv, _ = ops.attgate_fwd(_act(), _act(), [a.t for a in prm.values()], "relu")
    fields = {"sg": T("act", sv.g), "sx": T("act", sv.x), "g1raw": T("act", sv.g1raw), "x1raw": T("act", sv.x1raw), "q": T("vec", sv.q),
              "ss_g": T("vec", sv.ss_g), "ss_x": T("vec", sv.ss_x), "mr_g": T("vec", sv.mr_g), "mr_x": T("vec", sv.mr_x),
              "st1": T("vec", sv.st1)}

    def bwd(dout, **k):
        s = ops.AttGateSaved()
        s.g, s.x, s.act, s.training = k["sg"], k["sx"], "relu", True
        for f in ("g1raw", "x1raw", "q", "ss_g", "ss_x", "mr_g", "mr_x", "st1"):
            setattr(s, f, k[f])
        return ops.attgate_bwd(dout, s, [k[f"p{i}"] for i in range(12)])
    tb["attgate_bwd"] = (bwd, dict(dout=T("act", _act()), **fields, **prm), BWD)
    return tb


_TABLE = {}


@pytest.mark.parametrize("name", ["attgate_fwd", "attgate_fwd(eval)", "attgate_bwd"])
def test_valid_call_is_launched_and_every_corruption_refused(name, standin):
    if not _TABLE:
        _TABLE.update(_table())
    call, args, expect = _TABLE[name]
    del standin.calls[:]
    good = {k: a.t for k, a in args.items()}
    call(**good)
    assert standin.calls == expect
    bad = []
    for label, a in args.items():
        for what, t in corruptions(a, partners=True).items():
            del standin.calls[:]
            try:
                call(**{**good, label: t})
            except (_lib.BratsHipError, ValueError):
                if standin.calls:
                    bad.append(f"{label}/{what}: raised after {standin.calls}")
            else:
                bad.append(f"{label}/{what}: accepted, recorded {standin.calls}")
    assert not bad, f"{name}: " + "; ".join(bad)


def test_the_wrappers_are_re_exports_of_their_own_module():
    assert ops.attgate_fwd.__module__ == ops.attgate_bwd.__module__ == ops.AttGateSaved.__module__ == "brats21_amd._attgate"
    for bad in ("none", "prelu", "gelu"):
        with pytest.raises(_lib.BratsHipError):
            ops.attgate_fwd(_act(), _act(), [a.t for a in _params().values()], bad)
    with pytest.raises(_lib.BratsHipError):
        ops.attgate_fwd(_act(), _act(), [a.t for a in _params().values()], "relu", training=False)
    with pytest.raises(_lib.BratsHipError):
        ops.attgate_bwd(_act(), None, [a.t for a in _params().values()])
