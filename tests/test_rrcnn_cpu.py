"""CPU side of brats21_amd.networks.RRCNNblock: the float64 restatement (tests/_rrcnn_ref.py) against the fixtures made from the
reference's own class (tests/golden/rrcnn_*.npz), the schedule of ops.rrcnn_fwd / rrcnn_bwd restated in float64 (manual_backward)
against autograd of the restatement, the state-dict contract, the constructor / CPU-tensor errors, and the two new ABI entries."""
import ctypes

import numpy as np
import pytest
import torch

import _rrcnn_ref as R


def _lat(a, step):
    return a[:, :, ::step, ::step, ::step]


@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_restatement_matches_the_reference_in_float64(case):
    """out, dx and every parameter gradient of the restatement against the reference class in float64: 1e-12 (of the tensor's
    maximum where that exceeds 1)."""
    z, meta = R.golden(case)
    assert (meta["ch_in"], meta["ch_out"], meta["norm"], meta["act"], meta["t"], tuple(meta["dims"])) == case
    out, dx, _, grads = R.fixture_run64(case)
    lat = meta["lattice"]
    assert float(np.abs(_lat(out, lat["out64"]).numpy() - z["out64"]).max()) <= 1e-12 * max(1.0, float(np.abs(z["out64"]).max()))
    assert float(np.abs(_lat(dx, lat["dx"]).numpy() - z["dx64"]).max()) <= 1e-12 * max(1.0, float(np.abs(z["dx64"]).max()))
    for k in meta["keys"]:
        assert float(np.abs(grads[k].numpy() - z["grad64:" + k]).max()) <= 1e-12 * max(1.0, float(np.abs(z["grad64:" + k]).max())), k
    # the float32 results of the reference lie within the recorded errors of the restatement
    assert float(np.abs(z["out"] - out.numpy()).max()) <= float(z["ref_err_out"]) * (1 + 1e-6)


@pytest.mark.parametrize("two", [False, True], ids=["one_source", "two_sources"])
@pytest.mark.parametrize("t", [1, 2, 3])
@pytest.mark.parametrize("norm,act", [("group", "relu"), ("instance", "leakyrelu"), ("group", "mish")])
def test_manual_backward_matches_autograd(norm, act, t, two):
    """The schedule of ops.rrcnn_fwd / rrcnn_bwd in float64 -- stacked S / Y / DY, the dz chain, one sum per tensor with several
    readers, the weight gradient over the stacked batch -- gives what autograd gives for the restatement: 1e-10 of each tensor's
    maximum.  (A 3x3x3 bias under instance norm has a gradient that is zero in exact arithmetic: it is held to 1e-10 of the maximum
    of the unit's norm-shift gradient, the channel sum over the same voxels.)"""
    dims = (2, 4, 6, 8)
    sd = R.weights(R.shapes_of(16 if two else 8, 16))
    x, x2, g = R.image(8, dims), (R.image(8, dims, seed=5) if two else None), R.upstream(16, dims)
    want = R.run64(sd, x, g, norm, act, t, x2)
    got = R.manual_backward(sd, x, g, norm, act, t, x2)
    for a, b in zip(want[:3], got[:3]):
        assert (a is None) == (b is None)
        if a is not None:
            assert float((a - b).abs().max()) <= 1e-10 * float(a.abs().max())
    assert list(got[3]) != [] and set(got[3]) == set(want[3])
    for k, a in want[3].items():
        scale = float(a.abs().max())
        if k.endswith("conv.0.bias") and norm == "instance":
            scale = float(want[3][k.replace("conv.0.bias", "conv.1.bias")].abs().max())
        assert float((a - got[3][k]).abs().max()) <= 1e-10 * scale, k


@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_state_dict_is_the_references(case):
    z, meta = R.golden(case)
    m = R.build(case[0], case[1], case[2], case[3], case[4], load=False)
    sd = m.state_dict()
    assert list(sd) == meta["keys"] and [list(v.shape) for v in sd.values()] == meta["shapes"]
    assert [n for n, _ in m.named_parameters()] == meta["keys"]
    assert meta["keys"] == ["RCNN.0.conv.0.weight", "RCNN.0.conv.0.bias", "RCNN.0.conv.1.weight", "RCNN.0.conv.1.bias",
                            "RCNN.1.conv.0.weight", "RCNN.1.conv.0.bias", "RCNN.1.conv.1.weight", "RCNN.1.conv.1.bias",
                            "Conv_1x1.weight", "Conv_1x1.bias"]
    assert list(R.shapes_of(case[0], case[1]).items()) == list(R.fixture_shapes(case).items())
    res = m.load_state_dict(R.weights(R.fixture_shapes(case)), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(m.Conv_1x1.weight.detach(), R.weights(R.fixture_shapes(case))["Conv_1x1.weight"])


def test_initialisation_is_kaiming_fan_out_with_default_biases():
    torch.manual_seed(3)
    from brats21_amd.networks import RRCNNblock
    m = RRCNNblock(32, 64)
    w = m.RCNN["0"].conv["0"].weight.detach()
    assert abs(float(w.std()) / (2.0 / (64 * 27)) ** 0.5 - 1) < 0.05  # fan_out = Cout * 27
    assert abs(float(m.Conv_1x1.weight.detach().std()) / (2.0 / 64) ** 0.5 - 1) < 0.1
    b = m.RCNN["1"].conv["0"].bias.detach()
    assert float(b.abs().max()) <= 1.0 / (64 * 27) ** 0.5 and float(b.abs().max()) > 0  # nn.Conv3d's default: U(+-1 / sqrt(fan_in))
    assert bool((m.RCNN["0"].conv["1"].weight == 1).all()) and bool((m.RCNN["0"].conv["1"].bias == 0).all())
    assert m.storage == torch.float32 and m.t == 2


def test_constructor_and_cpu_tensor_errors():
    from brats21_amd._lib import BratsHipError
    from brats21_amd.networks import RRCNNblock
    for norm in ("batch", "bcn", "none"):
        with pytest.raises(NotImplementedError, match=f"--norm {norm} is not built"):
            RRCNNblock(8, 16, norm_layer=norm)
    with pytest.raises(NotImplementedError, match="group\\|instance"):
        RRCNNblock(8, 16, norm_layer="layer")
    with pytest.raises(NotImplementedError, match="prelu is not built"):
        RRCNNblock(8, 16, act="prelu")
    with pytest.raises(NotImplementedError, match="relu\\|leakyrelu\\|elu\\|swish\\|mish"):
        RRCNNblock(8, 16, act="gelu")
    for t in (0, -1, 1.5):
        with pytest.raises(ValueError, match="t must be an integer >= 1"):
            RRCNNblock(8, 16, t=t)
    with pytest.raises(NotImplementedError, match="multiple of 8"):
        RRCNNblock(8, 12)
    with pytest.raises(NotImplementedError, match="1 .. 16 or a multiple of 8"):
        RRCNNblock(20, 16)
    for cin in (1, 3, 4, 8, 13, 16, 24, 96):
        assert RRCNNblock(cin, 16).ch_in == cin
    m = RRCNNblock(4, 16)
    with pytest.raises(BratsHipError, match="GPU only"):
        m(torch.zeros(1, 4, 4, 4, 4))


def test_new_symbols_are_exported_and_reject_bad_arguments():
    """brats_affine_act_add_fwd / brats_grad_sum: declared, exported, ABI version still 7; NULL pointers and misaligned C / pitches
    return BRATS_E_ARG (-1) before anything is dereferenced, with the entry's name in brats_last_error()."""
    from brats21_amd import _lib
    names = _lib.declared_symbols()
    assert "brats_affine_act_add_fwd" in names and "brats_grad_sum" in names
    assert _lib._parse_header()["brats_affine_act_add_fwd"] == ("i", "pippipiiifpiiip")
    assert _lib._parse_header()["brats_grad_sum"] == ("i", "pipipipiipiiiiip")
    assert _lib._header_abi_version() == 7
    l = _lib.lib()
    assert l.brats_abi_version() == 7
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for dtype in (_lib.F32, _lib.BF16, _lib.F16):
        for args in ((None, 16, p, p, 16, p, 16), (p, 16, None, p, 16, p, 16), (p, 16, p, None, 16, p, 16), (p, 16, p, p, 16, None, 16)):
            assert l.brats_affine_act_add_fwd(*args, dtype, _lib.ACT_RELU, 0.01, None, 1, 1, 16, None) == -1
            assert b"affine_act_add_fwd" in l.brats_last_error()
        for c, pitches in ((6, (16, 16, 16)), (16, (18, 16, 16)), (16, (16, 18, 16)), (16, (16, 16, 18)), (16, (16, 8, 16))):
            assert l.brats_affine_act_add_fwd(p, pitches[0], p, p, pitches[1], p, pitches[2], dtype, _lib.ACT_RELU, 0.01, None, 1, 1, c,
                                              None) == -1
            assert b"affine_act_add_fwd" in l.brats_last_error()
        assert l.brats_grad_sum(None, 16, p, 16, None, 0, None, 0, 2, p, 16, dtype, 1, 1, 16, None) == -1 and b"grad_sum" in l.brats_last_error()
        assert l.brats_grad_sum(p, 16, p, 16, None, 0, None, 0, 3, p, 16, dtype, 1, 1, 16, None) == -1 and b"grad_sum" in l.brats_last_error()
        assert l.brats_grad_sum(p, 16, p, 16, None, 0, None, 0, 2, None, 16, dtype, 1, 1, 16, None) == -1 and b"grad_sum" in l.brats_last_error()
        for nsrc in (0, 1, 5):
            assert l.brats_grad_sum(p, 16, p, 16, p, 16, p, 16, nsrc, p, 16, dtype, 1, 1, 16, None) == -1 and b"grad_sum" in l.brats_last_error()
        assert l.brats_grad_sum(p, 16, p, 18, None, 0, None, 0, 2, p, 16, dtype, 1, 1, 16, None) == -1 and b"grad_sum" in l.brats_last_error()
        assert l.brats_grad_sum(p, 16, p, 16, None, 0, None, 0, 2, p, 18, dtype, 1, 1, 16, None) == -1 and b"grad_sum" in l.brats_last_error()
        assert l.brats_grad_sum(p, 16, p, 16, None, 0, None, 0, 2, p, 16, dtype, 1, 1, 6, None) == -1 and b"grad_sum" in l.brats_last_error()
