"""-m "not gpu": AttEquiUnet's contract without a GPU.  tests/_att_ref.py (the float64 restatement the GPU tests are held against)
reproduces tests/golden/att_w16_instance_relu.npz -- the reference's own AttEquiUnet class, run by tests/golden/make_golden_att.py
-- to 1e-12 where the fixture holds float64 and within the recorded float32 error of the reference elsewhere, and agrees with the
reference class directly where its source is present; brats21_amd.networks.AttEquiUnet has the fixture's state-dict names, shapes
and order, loads it with strict=True, and refuses what it does not build; the three pooled gate passes are declared, bound and
refuse bad arguments."""
import contextlib
import copy
import ctypes
import io
import json
import os

import numpy as np
import pytest
import torch

import _att_ref as R
from oracle import synth


@pytest.fixture(scope="module")
def golden(golden_dir):
    z = np.load(os.path.join(golden_dir, R.FNAME), allow_pickle=False)
    return z, json.loads(str(z["meta"]))


@pytest.fixture(scope="module")
def run64():
    return R.run64(R.weights(), R.image(), synth.nested_spheres(1, R.SIZE))


def test_restatement_reproduces_the_reference_fixture(golden, run64):
    z, meta = golden
    heads, loss, grads = run64
    names = json.loads(str(z["grad_names"]))
    assert names == list(grads) == meta["keys"] and len(names) == 103
    # float64 entries: the reference class in float64
    assert abs(loss - float(z["loss64"])) <= 1e-12
    assert float(np.abs(heads[0].numpy()[:, :, ::2, ::2, ::2] - z["logits64"]).max()) <= 1e-12
    norms = np.array([float(grads[n].norm()) for n in names])
    assert float(np.abs(norms - z["grad_norms64"]).max()) <= 1e-12 * max(1.0, float(z["grad_norms64"].max()))
    for k in (k for k in z.files if k.startswith("grad64:")):
        assert float(np.abs(grads[k[7:]].numpy() - z[k]).max()) <= 1e-12 * max(1.0, float(np.abs(z[k]).max())), k
    # float32 entries: within the reference's own recorded float32 error (the fixture's entries ARE that error's other side)
    assert float(np.abs(heads[0].numpy() - z["logits"]).max()) <= float(z["ref_err_logits"]) * (1 + 1e-6)
    for i in range(4):
        assert float(np.abs(heads[1 + i].numpy()[:, :, ::2, ::2, ::2] - z[f"deep{i}"]).max()) <= float(z["ref_err_deep"]) * (1 + 1e-6)
    assert abs(loss - float(z["loss"])) <= float(z["ref_err_loss"]) * (1 + 1e-6) + 1e-15
    assert float(np.abs(z["grad_norms"] / norms - 1).max()) <= float(z["ref_err_gnorm_rel"]) * (1 + 1e-6)
    for k in (k for k in z.files if k.startswith("grad:")):
        g = grads[k[5:]].numpy()
        assert float(np.abs(g - z[k]).max() / np.abs(g).max()) <= float(z["ref_err_grad_small"]) * (1 + 1e-6), k
    # the room under the bars of tests/test_att_gpu.py the generator asserted
    assert float(z["ref_err_logits"]) < 2.5e-4 and float(z["ref_err_deep"]) < 2.5e-4 and float(z["ref_err_loss"]) < 2.5e-5
    assert float(z["ref_err_gnorm_rel"]) < 2e-3 and float(z["ref_err_grad_small"]) < 2e-3
    assert all(n > 0 for n in norms), "a parameter without gradient tests nothing"


def test_restatement_matches_the_reference_class(run64):
    from oracle import refshim
    if not refshim.reference_available():
        pytest.skip("the reference source is not on this machine")
    refshim.install()
    from networks.equiunet2020 import AttEquiUnet as Ref
    with contextlib.redirect_stdout(io.StringIO()):
        m = Ref(4, 3, [R.WIDTH * 2 ** i for i in range(4)], norm_layer=R.NORM, act=R.ACT, deep_supervision=True).double()
    sd = R.weights()
    assert list(m.state_dict()) == list(sd) == list(R.state_shapes())
    m.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
    m.train()
    res = m(R.image().double())
    loss = R.ds_loss(res, synth.nested_spheres(1, R.SIZE).double())
    loss.backward()
    heads, loss64, grads = run64
    assert abs(float(loss.detach()) - loss64) <= 1e-12
    for a, b in zip(R.heads(res), heads):
        assert float((a.detach() - b).abs().max()) <= 1e-12
    for k, p in m.named_parameters():
        assert float((p.grad - grads[k]).abs().max()) <= 1e-12 * max(1.0, float(grads[k].abs().max())), k


def test_module_state_dict_is_the_references(golden):
    _, meta = golden
    m = R.build()
    sd = m.state_dict()
    assert list(sd.keys()) == meta["keys"] == list(R.state_shapes()) and len(sd) == 103
    assert [list(v.shape) for v in sd.values()] == meta["shapes"]
    want = R.weights()
    m.load_state_dict(want, strict=True)
    assert all(torch.equal(m.state_dict()[k], want[k]) for k in want)
    assert [n for n, _ in m.named_parameters()] == meta["keys"], "every key is a parameter (instance norm has no buffers)"
    m2 = copy.deepcopy(m)
    assert all(torch.equal(a, b) and a is not b for a, b in zip(m.state_dict().values(), m2.state_dict().values()))
    assert m2.fold_gate_pool is True and m2.precision == "fp32"
    # without deep supervision the four heads' eight keys are gone
    assert len(R.build(deep_supervision=False).state_dict()) == 95
    # the flagship width
    from brats21_amd.networks import AttEquiUnet
    with contextlib.redirect_stdout(io.StringIO()):
        big = AttEquiUnet(4, 3, [48, 96, 192, 384], norm_layer="instance", deep_supervision=True)
    assert list(big.state_dict()) == meta["keys"]
    assert big.state_dict()["bottom_2.1.ChannelGate.mlp.1.weight"].shape == (12, 192)


def test_initialisation_is_kaiming_fan_out():
    torch.manual_seed(0)
    sd = R.build().state_dict()
    w = sd["encoder4.UBlock.ConvBnRelu2.conv.weight"]
    assert abs(float(w.std()) / (2.0 / (128 * 27)) ** 0.5 - 1) < 0.05
    w = sd["bottom.CBAM.ChannelGate.mlp.3.weight"]  # [128, 8]: fan_out 128
    assert abs(float(w.std()) / (2.0 / 128) ** 0.5 - 1) < 0.15
    assert float(sd["bottom.CBAM.SpatialGate.spatial.bn.weight"]) == 1.0 and float(sd["bottom_2.0.bn.bias"].abs().max()) == 0.0


def _make(**kw):
    from brats21_amd.networks import AttEquiUnet
    args = dict(inplanes=4, num_classes=3, features=[16, 32, 64, 128], norm_layer="instance")
    args.update(kw)
    with contextlib.redirect_stdout(io.StringIO()):
        return AttEquiUnet(**args)


def test_refusals():
    from brats21_amd import BratsHipError
    for norm in ("group", "bcn"):
        with pytest.raises(ValueError, match="reference fails"):
            _make(norm_layer=norm)
    with pytest.raises(NotImplementedError, match="gate"):
        _make(norm_layer="batch")
    with pytest.raises(NotImplementedError):
        _make(norm_layer=None)
    for feats in ([8, 16, 32, 64], [24, 48, 96, 192], [128, 256, 512, 1024]):
        with pytest.raises(NotImplementedError, match="C // 16 >= 1, C % 8 == 0 and C <= 512"):
            _make(features=feats)
    with pytest.raises(ValueError):
        _make(dropout=1.0)
    x = torch.zeros(1, 4, 16, 16, 16)
    m = _make()
    m.precision = "fp16"
    with pytest.raises(NotImplementedError, match="fp16"):
        m(x)
    m.precision = "bf16"
    m.conv_fp8 = "fwd"
    with pytest.raises(NotImplementedError, match="e4m3"):
        m(x)
    m.conv_fp8 = None
    with pytest.raises(BratsHipError, match="GPU only"):
        m(x)


def test_pooled_gate_entry_points_are_declared_and_refuse_bad_arguments():
    from brats21_amd import _lib
    names = ("brats_cbam_apply_pool", "brats_cbam_bwd_reduce_pool", "brats_cbam_bwd_apply_pool")
    assert all(n in _lib.declared_symbols() for n in names)
    l = _lib.lib()
    assert l.brats_abi_version() == 7
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def apply_pool(x, dtype, c, d, h, w):
        return l.brats_cbam_apply_pool(x, c, p, p, p, p, p, p, c, p, c, None, dtype, 1, c, d, h, w, None)

    def reduce_pool(dpooled, dtype, c, d, h, w, idx=p):
        return l.brats_cbam_bwd_reduce_pool(None, 0, dpooled, c, idx, p, c, p, p, p, p, p, p, p, p, p, dtype, 1, c, d, h, w, None)

    def bwd_apply_pool(dpooled, dtype, c, d, h, w, idx=p):
        return l.brats_cbam_bwd_apply_pool(None, 0, dpooled, c, idx, p, p, p, p, p, p, p, p, p, p, c, dtype, 1, c, d, h, w, None)

    for fn, name in ((apply_pool, b"cbam_apply_pool"), (reduce_pool, b"cbam_bwd_reduce_pool"), (bwd_apply_pool, b"cbam_bwd_apply_pool")):
        assert fn(p, _lib.F16, 16, 2, 2, 2) == -2 and b"fp16" in l.brats_last_error() and name in l.brats_last_error()
        assert fn(p, _lib.F32, 20, 2, 2, 2) == -2 and b"multiple of 8" in l.brats_last_error()
        assert fn(None, _lib.BF16, 16, 2, 2, 2) == -1 and name in l.brats_last_error()
        assert fn(p, _lib.F32, 16, 2, 3, 2) == -1 and b"even" in l.brats_last_error() and name in l.brats_last_error()
    for fn, name in ((reduce_pool, b"cbam_bwd_reduce_pool"), (bwd_apply_pool, b"cbam_bwd_apply_pool")):
        assert fn(p, _lib.F32, 16, 2, 2, 2, idx=None) == -1 and b"window-index" in l.brats_last_error() and name in l.brats_last_error()
