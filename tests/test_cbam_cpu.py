"""-m "not gpu": the CBAM block's contract without a GPU.  tests/_cbam_ref.py (the float64 restatement the GPU tests are held
against) reproduces tests/golden/cbam.npz -- the reference's own CBAM class, run by tests/golden/make_golden_cbam.py -- to 1e-12
in the value and every gradient, the integer tie case included, and agrees with the reference class directly where its source is
present; brats21_amd.networks.CBAM has the fixture's state-dict names, shapes and order, loads it with strict=True, and refuses
what it does not build."""
import argparse
import copy
import json
import os

import numpy as np
import pytest
import torch

import _cbam_ref as R


@pytest.fixture(scope="module")
def golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "cbam.npz"))
    meta = json.loads(str(z["meta"]))
    assert meta["keys"] == list(R.KEYS)
    return z, meta


def case_tensors(z, name):
    sd = {k: torch.from_numpy(z[f"{name}/sd/{k}"]) for k in R.KEYS}
    return sd, torch.from_numpy(z[f"{name}/x"]), torch.from_numpy(z[f"{name}/dout"])


@pytest.mark.parametrize("name", ["c16", "c48", "tie"])
def test_restatement_reproduces_the_reference_fixture(golden, name):
    z, meta = golden
    sd, x, dout = case_tensors(z, name)
    assert list(x.shape) == meta["cases"][name] and x.dtype == torch.float64
    out, dx, grads = R.run(sd, x, dout)
    assert float((out - torch.from_numpy(z[f"{name}/out"])).abs().max()) <= 1e-12
    assert float((dx - torch.from_numpy(z[f"{name}/dx"])).abs().max()) <= 1e-12
    for k in R.KEYS:
        assert float((grads[k] - torch.from_numpy(z[f"{name}/grad/{k}"])).abs().max()) <= 1e-12, k


def test_tie_case_holds_both_kinds_of_tie(golden):
    z, _ = golden
    _, x, _ = case_tensors(z, "tie")
    assert bool((x == x.round()).all())
    flat = x.flatten(2)
    assert bool(((flat == flat.max(2, keepdim=True)[0]).sum(2) > 1).any())  # equal maxima over the voxels of a channel
    assert bool(((x == x.max(1, keepdim=True)[0]).sum(1) > 1).any())        # equal maxima over the channels of a voxel
    # the gradient of a maximum goes to the FIRST of equal maxima, which a mirrored input shows: with the spatial path switched
    # off (convolution weight 0, so g is a constant) and a live MLP, dx of the flipped input is not the flipped dx
    sd, x, dout = case_tensors(z, "tie")
    sd = dict(sd)
    sd[R.KEYS[0]] = torch.ones_like(sd[R.KEYS[0]])
    sd[R.KEYS[2]] = torch.full_like(sd[R.KEYS[2]], 0.01)   # a live MLP, so that dmax is not zero
    sd[R.KEYS[4]] = torch.zeros_like(sd[R.KEYS[4]])
    _, dx, _ = R.run(sd, x, dout)
    _, dx_flip, _ = R.run(sd, x.flip(2, 3, 4), dout.flip(2, 3, 4))
    assert float((dx - dx_flip.flip(2, 3, 4)).abs().max()) > 1e-6  # first-index routing is not flip-symmetric


def test_restatement_matches_the_reference_class():
    from oracle import refshim
    if not refshim.reference_available():
        pytest.skip("the reference source is not on this machine")
    import contextlib
    import io
    refshim.install()
    from networks.equiunet2020 import CBAM as RefCBAM
    from networks.factory import get_norm_layer
    g = torch.Generator().manual_seed(3)
    with contextlib.redirect_stdout(io.StringIO()):
        m = RefCBAM(32, norm_layer=get_norm_layer("instance")).double()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    assert list(sd.keys()) == list(R.KEYS)
    x = torch.randn((2, 32, 3, 4, 9), generator=g, dtype=torch.float64)
    dout = torch.randn(x.shape, generator=g, dtype=torch.float64)
    xx = x.clone().requires_grad_(True)
    y = m(xx)
    y.backward(dout)
    out, dx, grads = R.run(sd, x, dout)
    assert float((out - y.detach()).abs().max()) <= 1e-12 and float((dx - xx.grad).abs().max()) <= 1e-12
    for k, p in m.named_parameters():
        assert float((grads[k] - p.grad).abs().max()) <= 1e-12, k


def test_module_state_dict_is_the_references(golden):
    from brats21_amd.networks import CBAM
    z, _ = golden
    for name, c in (("c16", 16), ("c48", 48)):
        m = CBAM(c)
        sd = m.state_dict()
        assert list(sd.keys()) == list(R.KEYS)
        want = {k: torch.from_numpy(z[f"{name}/sd/{k}"]).float() for k in R.KEYS}
        assert all(tuple(sd[k].shape) == tuple(want[k].shape) == tuple(R.shapes(c)[k]) for k in R.KEYS)
        m.load_state_dict(want, strict=True)
        assert all(torch.equal(m.state_dict()[k], want[k]) for k in R.KEYS)
        assert all(isinstance(p, torch.nn.Parameter) for p in m.parameters()) and len(list(m.parameters())) == 7
        m2 = copy.deepcopy(m)
        assert all(torch.equal(a, b) and a is not b for a, b in zip(m.state_dict().values(), m2.state_dict().values()))
    assert CBAM(64, reduction_ratio=4).state_dict()[R.KEYS[0]].shape == (16, 64)
    assert CBAM(16).storage == torch.float32


def test_initialisation_is_kaiming_fan_out():
    from brats21_amd.networks import CBAM
    torch.manual_seed(0)
    m = CBAM(512, reduction_ratio=2)
    sd = m.state_dict()
    # std = sqrt(2 / fan_out): fan_out = out_features of a Linear, out_channels * 343 of the convolution
    assert abs(float(sd[R.KEYS[0]].std()) / (2.0 / 256) ** 0.5 - 1) < 0.05
    assert abs(float(sd[R.KEYS[2]].std()) / (2.0 / 512) ** 0.5 - 1) < 0.05
    assert abs(float(sd[R.KEYS[4]].std()) / (2.0 / 343) ** 0.5 - 1) < 0.2
    assert float(sd[R.KEYS[5]]) == 1.0 and float(sd[R.KEYS[6]]) == 0.0


def test_refusals():
    from brats21_amd import BratsHipError
    from brats21_amd.networks import CBAM
    for norm, exc in (("group", ValueError), ("bcn", ValueError), ("batch", NotImplementedError), ("layer", ValueError)):
        with pytest.raises(exc):
            CBAM(16, norm_layer=norm)
    with pytest.raises(NotImplementedError, match="att_equiunet"):
        CBAM(16, norm_layer="batch")
    with pytest.raises(ValueError, match="num_groups"):
        CBAM(16, norm_layer="group")
    for pools in (["avg"], ["max", "avg"], ["avg", "max", "lp"]):
        with pytest.raises(NotImplementedError):
            CBAM(16, pool_types=pools)
    CBAM(16, pool_types=["avg", "max"])
    for c, r in ((20, 4), (520, 16), (8, 16), (1024, 16)):
        with pytest.raises(NotImplementedError, match="512"):
            CBAM(c, reduction_ratio=r)
    with pytest.raises(BratsHipError):
        CBAM(16)(torch.zeros(1, 16, 4, 4, 4))  # no CPU fallback


def test_library_refuses_fp16_and_bad_arguments():
    import ctypes
    from brats21_amd import _lib
    l = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    rc = l.brats_cbam_pool(p, 16, p, p, p, _lib.F16, 1, 16, 1, 1, 1, None)
    assert rc == -2 and b"fp16" in l.brats_last_error()
    rc = l.brats_cbam_pool(None, 16, p, p, p, _lib.BF16, 1, 16, 1, 1, 1, None)
    assert rc == -1 and b"cbam_pool" in l.brats_last_error()
    rc = l.brats_cbam_apply(p, 16, p, p, p, p, p, p, 16, _lib.F32, 1, 20, 2, 2, 2, None)
    assert rc == -2 and b"multiple of 8" in l.brats_last_error()
    rc = l.brats_cbam_bwd_gate(None, p, p, p, p, p, p, p, p, p, p, p, p, p, p, p, p, 1, 16, 1, None)
    assert rc == -1 and b"cbam_bwd_gate" in l.brats_last_error()
    assert l.brats_cbam_tiles(128, 128, 128) == 32 * 16 * 4 and l.brats_cbam_tiles(1, 1, 65) == 3
    assert l.brats_cbam_blocks(_lib.BF16, 48, 128, 128, 128) == 1024 and l.brats_cbam_blocks(_lib.F32, 16, 1, 1, 65) == 1
    assert l.brats_cbam_blocks(_lib.F16, 48, 8, 8, 8) == 0


def test_att_equiunet_is_still_not_built():
    from brats21_amd import get_model
    with pytest.raises(NameError):
        get_model(argparse.Namespace(model="att_equiunet", width=8, norm="instance", act="relu", num_classes=3, dropout=0))
