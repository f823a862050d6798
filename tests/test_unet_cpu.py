"""-m "not gpu": Unet's contract without a GPU.  tests/_unet_ref.py (the float64 restatement the GPU tests are held against)
reproduces tests/golden/unet_w8_*.npz -- the reference's own Unet class, run by tests/golden/make_golden_unet.py -- to 1e-12 where the
fixtures hold float64 and within the recorded float32 error of the reference elsewhere, and agrees with the reference class directly
where its source is present; brats21_amd.networks.Unet has the fixtures' state-dict names, shapes and order, loads them with
strict=True, comes out of get_model("modified_unet") and refuses what it does not build; the four nearest-neighbour entry points are
declared, bound and refuse bad arguments."""
import argparse
import contextlib
import copy
import ctypes
import io

import numpy as np
import pytest
import torch

import _unet_ref as R


@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_restatement_reproduces_the_reference_fixture(case):
    z, meta = R.golden(case)
    heads, loss, grads = R.fixture_run64(case)
    names = meta["keys"]
    assert names == list(grads) and len(names) == 76 and meta["scales"] == list(R.SCALES)
    assert np.array_equal(z["x"], R.image().numpy()), "the committed input is the regenerated one"
    # float64 entries: the reference class in float64
    assert abs(loss - float(z["loss64"])) <= 1e-12
    assert float(np.abs(heads[0].numpy()[:, :, ::2, ::2, ::2] - z["d1_64"]).max()) <= 1e-12
    norms = np.array([float(grads[n].norm()) for n in names])
    assert float(np.abs(norms - z["grad_norms64"]).max()) <= 1e-12 * max(1.0, float(z["grad_norms64"].max()))
    for k in (k for k in z.files if k.startswith("grad64:")):
        assert float(np.abs(grads[k[7:]].numpy() - z[k]).max()) <= 1e-12 * max(1.0, float(np.abs(z[k]).max())), k
    # float32 entries: within the reference's own recorded float32 error (the fixture's entries ARE that error's other side)
    for i, s in enumerate(R.SCALES):
        h = heads[i].numpy()
        assert h.shape == (R.BATCH, 3, *R.SIZE)
        assert float(np.abs(h[:, :, ::s, ::s, ::s] - z[f"d{i + 1}"]).max()) <= float(z["ref_err_heads"]) * (1 + 1e-6)
    assert abs(loss - float(z["loss"])) <= float(z["ref_err_loss"]) * (1 + 1e-6) + 1e-15
    live = [i for i, n in enumerate(names) if norms[i] > 1e-9]
    assert float(np.abs(z["grad_norms"][live] / norms[live] - 1).max()) <= float(z["ref_err_gnorm_rel"]) * (1 + 1e-6)
    for k in (k for k in z.files if k.startswith("grad:")):
        g = grads[k[5:]].numpy()
        if np.abs(g).max() > 1e-9:
            assert float(np.abs(g - z[k]).max() / np.abs(g).max()) <= float(z["ref_err_grad_small"]) * (1 + 1e-6), k
        else:  # zero in exact arithmetic (a convolution bias in front of a per-channel normalisation)
            assert k.endswith(".bias") and float(np.abs(z[k]).max()) <= float(z["ref_err_grad_dead"])
    # the room under the bars of tests/test_unet_gpu.py the generator asserted
    assert float(z["ref_err_heads"]) < 2.5e-4 and float(z["ref_err_loss"]) < 2.5e-5
    assert float(z["ref_err_gnorm_rel"]) < 2e-3 and float(z["ref_err_grad_small"]) < 2e-3
    dead = [n for i, n in enumerate(names) if i not in live]
    conv_bias = [n for n in names if n.endswith(("conv.0.bias", "conv.3.bias", "up.1.bias"))]
    assert len(conv_bias) == 17
    if case[0] == "group":  # (8 groups of ONE channel in the 8-wide units: a per-channel normalisation there)
        assert dead == [n for n in conv_bias if n.split(".")[0] in ("Conv1", "Up2", "Up_conv2")]
    else:
        assert dead == conv_bias


@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_restatement_matches_the_reference_class(case):
    from oracle import refshim
    if not refshim.reference_available():
        pytest.skip("the reference source is not on this machine")
    refshim.install()
    refshim._mod("monai.networks.nets", DynUNet=None)  # (networks/unet_family.py:503 imports the name)
    from networks.unet_family import Unet as Ref
    norm, act = case
    with contextlib.redirect_stdout(io.StringIO()):
        m = Ref(4, 3, [R.WIDTH * 2 ** i for i in range(4)], norm_layer=norm, act=act, deep_supervision=True).double()
    shapes = R.fixture_shapes(case)
    assert list(m.state_dict()) == list(shapes) and [tuple(v.shape) for v in m.state_dict().values()] == list(shapes.values())
    m.load_state_dict({k: v.double() for k, v in R.weights(shapes).items()}, strict=True)
    m.train()
    res = m(R.image().double())
    loss = R.ds_loss(res, R.target().double())
    loss.backward()
    heads, loss64, grads = R.fixture_run64(case)
    assert abs(float(loss.detach()) - loss64) <= 1e-12
    for a, b in zip(res, heads):
        assert float((a.detach() - b).abs().max()) <= 1e-12
    for k, p in m.named_parameters():
        assert float((p.grad - grads[k]).abs().max()) <= 1e-12 * max(1.0, float(grads[k].abs().max())), k


@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_module_state_dict_is_the_references(case):
    _, meta = R.golden(case)
    m = R.build(case, load=False)
    sd = m.state_dict()
    assert list(sd.keys()) == meta["keys"]
    assert [list(v.shape) for v in sd.values()] == meta["shapes"]
    want = R.weights(R.fixture_shapes(case))
    m.load_state_dict(want, strict=True)
    assert all(torch.equal(m.state_dict()[k], want[k]) for k in want)
    assert [n for n, _ in m.named_parameters()] == meta["keys"], "every key is a parameter (neither norm has buffers)"
    m2 = copy.deepcopy(m)
    assert all(torch.equal(a, b) and a is not b for a, b in zip(m.state_dict().values(), m2.state_dict().values()))
    assert m2.precision == "fp32" and m2.Up4.units[0].conv is m2.Up4.up["1"] and m2.Up4.units[0].conv is not m.Up4.up["1"]
    # without deep supervision the three deep heads' six keys are gone
    assert list(R.build(case, deep_supervision=False, load=False).state_dict()) == meta["keys"][:-6]


def test_initialisation_is_kaiming_fan_out():
    torch.manual_seed(0)
    m = R.build(load=False)
    sd = m.state_dict()
    w = sd["Conv4.conv.3.weight"]
    assert abs(float(w.std()) / (2.0 / (64 * 27)) ** 0.5 - 1) < 0.05
    b = sd["Conv4.conv.3.bias"]  # nn.Conv3d's default: U(-1 / sqrt(fan_in), 1 / sqrt(fan_in))
    assert 0 < float(b.abs().max()) <= (64 * 27) ** -0.5
    assert float(sd["Conv4.conv.4.weight"].min()) == 1.0 and float(sd["Conv4.conv.4.bias"].abs().max()) == 0.0


def _namespace(**kw):
    ns = dict(model="modified_unet", width=8, norm="group", act="relu", num_classes=3, dropout=0)
    ns.update(kw)
    return argparse.Namespace(**ns)


def test_get_model_builds_it_and_keeps_its_errors():
    from brats21_amd import BratsHipError, get_model
    from brats21_amd.networks import Unet
    with contextlib.redirect_stdout(io.StringIO()):
        m = get_model(_namespace())
        big = get_model(_namespace(width=48, norm="instance", num_classes=5))
    assert isinstance(m, Unet) and m.deep_supervision and m.features == [8, 16, 32, 64]
    assert list(m.state_dict()) == R.golden(R.CASES[0])[1]["keys"] == list(big.state_dict())
    assert big.state_dict()["Up4.up.1.weight"].shape == (192, 384, 3, 3, 3) and big.state_dict()["outconv4.weight"].shape == (5, 384, 1, 1, 1)
    for name in ("r2unet", "r2attunet", "att_unet", "att_equiunet", "equiunet_assp_evo_ref", "nnunet", "equiunet_reff"):
        with pytest.raises(NameError, match="Not Supported Model"):
            get_model(_namespace(model=name))
    with pytest.raises(BratsHipError, match="GPU only"):
        m(torch.zeros(1, 4, 16, 16, 16))
    copy.deepcopy(m)


def _make(**kw):
    from brats21_amd.networks import Unet
    args = dict(img_ch=4, output_ch=3, features=[8, 16, 32, 64])
    args.update(kw)
    with contextlib.redirect_stdout(io.StringIO()):
        return Unet(**args)


def test_refusals():
    for norm in ("batch", "bcn", "none"):
        with pytest.raises(NotImplementedError, match=norm):
            _make(norm_layer=norm)
    with pytest.raises(NotImplementedError, match="layer"):
        _make(norm_layer="layer")
    with pytest.raises(NotImplementedError, match="prelu"):
        _make(act="prelu")
    with pytest.raises(NotImplementedError, match="gelu"):
        _make(act="gelu")
    for act in ("relu", "leakyrelu", "elu", "swish", "mish"):
        _make(act=act, norm_layer="instance")
    with pytest.raises(NotImplementedError, match="multiples of 8"):
        _make(features=[4, 8, 16, 32])
    with pytest.raises(NotImplementedError, match="inplanes <= 16"):
        _make(img_ch=17)
    with pytest.raises(NotImplementedError, match="num_classes <= 16"):
        _make(output_ch=17)
    m = _make()
    x = torch.zeros(1, 4, 16, 16, 16)
    m.conv_fp8 = "fwd"
    with pytest.raises(NotImplementedError, match="e4m3"):
        m(x)


def test_nearest_entry_points_are_declared_and_refuse_bad_arguments():
    from brats21_amd import _lib
    sigs = _lib._parse_header()
    assert sigs["brats_upsample_nearest_fwd"] == ("i", "pipi" + "i" * 7 + "p")
    assert sigs["brats_upsample_nearest_bwd"] == ("i", "pipipi" + "i" * 7 + "p")
    assert sigs["brats_planes_nearest_fwd"] == sigs["brats_planes_nearest_bwd"] == ("i", "pp" + "i" * 5 + "p")
    l = _lib.lib()
    assert l.brats_abi_version() == 7 == _lib._header_abi_version()
    for n in ("brats_upsample_nearest_fwd", "brats_upsample_nearest_bwd", "brats_planes_nearest_fwd", "brats_planes_nearest_bwd"):
        assert getattr(l, n).argtypes is not None and len(getattr(l, n).argtypes) == len(sigs[n][1])
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def fwd(x, y, dtype=_lib.BF16, c=8, scale=2, pitch=None):
        return l.brats_upsample_nearest_fwd(x, pitch or c, y, pitch or c, dtype, 1, c, 1, 1, 1, scale, None)

    def bwd(dy, dx, dtype=_lib.BF16, c=8, scale=2, pitch=None):
        return l.brats_upsample_nearest_bwd(dy, pitch or c, None, 0, dx, pitch or c, dtype, 1, c, 1, 1, 1, scale, None)

    for fn, name in ((fwd, b"upsample_nearest_fwd"), (bwd, b"upsample_nearest_bwd")):
        assert fn(None, p) == -1 and name in l.brats_last_error()
        assert fn(p, None) == -1 and name in l.brats_last_error()
        for scale in (1, 3, 4):
            assert fn(p, p, scale=scale) == -2 and name in l.brats_last_error() and b"scale" in l.brats_last_error()
        assert fn(p, p, c=12) == -2 and b"multiple of 8" in l.brats_last_error()
        assert fn(p, p, dtype=_lib.F32, c=6) == -2 and b"multiple of 4" in l.brats_last_error()
        assert fn(p, p, dtype=7) == -2 and b"dtype" in l.brats_last_error()
        assert fn(p, p, c=16, pitch=8) == -1 and b"pitch" in l.brats_last_error()
    for fn, name in ((l.brats_planes_nearest_fwd, b"planes_nearest_fwd"), (l.brats_planes_nearest_bwd, b"planes_nearest_bwd")):
        assert fn(None, p, 1, 1, 1, 1, 2, None) == -1 and name in l.brats_last_error()
        assert fn(p, None, 1, 1, 1, 1, 2, None) == -1 and name in l.brats_last_error()
        for scale in (0, 1, 3, 16):
            assert fn(p, p, 1, 1, 1, 1, scale, None) == -2 and name in l.brats_last_error() and b"scale" in l.brats_last_error()
        assert fn(p, p, 0, 1, 1, 1, 2, None) == -1 and name in l.brats_last_error()
