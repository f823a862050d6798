"""-m "not gpu": the attention gate's contract without a GPU.  tests/_attgate_ref.py (the float64 restatement the GPU tests are held
against) reproduces tests/golden/attgate_*.npz -- the reference's own AttentionBlock, run by tests/golden/make_golden_attgate.py --
to 1e-12; the schedule of ops.attgate_fwd / ops.attgate_bwd restated in float64 agrees with autograd of the restatement to 1e-10;
brats21_amd.networks.AttentionBlock has the reference's 21 state-dict names in order, loads a fixture with strict=True, initialises
as the enclosing networks do, and refuses what it does not build; the new entry points are declared and refuse bad arguments."""
import argparse
import copy
import ctypes

import pytest
import torch

import _attgate_ref as R


def _rel(a, b, den=None):
    den = b if den is None else den
    return float((a.double() - b.double()).abs().max() / den.double().abs().max())


@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_restatement_reproduces_the_reference_fixture(case):
    z, meta = R.golden(case)
    assert meta["keys"] == R.KEYS and meta["params"] == R.PARAMS
    assert {k: tuple(s) for k, s in zip(meta["keys"], meta["shapes"])} == R.shapes_of(*case[:3])
    r = R.fixture_run64(case)
    for name in ("out", "dg", "dx"):
        assert _rel(r[name], torch.from_numpy(z[name + "64"])) <= 1e-12, name
    for k in R.PARAMS:
        w = torch.from_numpy(z["grad64:" + k])
        den = torch.from_numpy(z["grad64:" + R.DEAD[k]]) if k in R.DEAD else w
        assert _rel(r["grads"][k], w, den) <= 1e-12, k
    for k in R.BUFFERS:
        w = torch.from_numpy(z["buf64:" + k])
        assert (int(r["buffers"][k]) == int(w) == 1) if k.endswith("tracked") else _rel(r["buffers"][k], w) <= 1e-12, k
    sd, g, x, dout = R.fixture_inputs(case)
    ev = R.run({**sd, **r["buffers"]}, g, x, dout, torch.float64, case[3], False, parts=("out",))
    assert _rel(ev["out"], torch.from_numpy(z["out_eval64"])) <= 1e-12
    # the float32 arrays are the same class's: within the recorded error of the float64 ones
    assert _rel(torch.from_numpy(z["out"]), r["out"]) == pytest.approx(float(z["ref_err_out"]), rel=1e-6)
    assert all(float(z[f"ref_bf16_dev_{n}"]) > 0 for n in ("out", "dg", "dx"))


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("act", ["relu", "leakyrelu", "elu", "swish", "mish"])
def test_the_backward_schedule_agrees_with_autograd(act, training):
    """Recompute of s and p, the shared sum of ds, the deferred dout * alpha, the plane without b_psi: 1e-10 of each tensor's
    maximum; the three convolution biases ahead of a training-mode BatchNorm (zero in exact arithmetic) against the maximum of the
    matching BatchNorm-bias gradient."""
    sd, g, x, dout = R.seeded((2, 24, 16, 12, 3, 4, 5), 7, b_psi=3.0)
    ref = R.run(sd, g, x, dout, torch.float64, act, training)
    got = R.manual_backward(sd, g, x, dout, act, training)
    for name in ("out", "dg", "dx"):
        assert _rel(got[name], ref[name]) <= 1e-10, name
    for k in R.PARAMS:
        den = ref["grads"][R.DEAD[k]] if (training and k in R.DEAD) else ref["grads"][k]
        assert tuple(got["grads"][k].shape) == tuple(ref["grads"][k].shape), k
        assert _rel(got["grads"][k], ref["grads"][k], den) <= 1e-10, k
    if training:
        assert all(float(ref["grads"][k].abs().max()) <= 1e-10 * float(ref["grads"][R.DEAD[k]].abs().max()) for k in R.DEAD)
    else:
        assert all(float(ref["grads"][k].abs().max()) > 0 for k in R.DEAD)


def test_every_gpu_shape_finds_a_seed():
    for name in R.SHAPES:
        R.pick(name)
    for act in ("leakyrelu", "elu", "swish", "mish"):
        R.pick("odd", act)
    R.pick("odd", b_psi=3.0, b_g=2.0)
    R.pick("odd", training=False)


def test_module_state_dict_is_the_references():
    for case in R.CASES:
        _, meta = R.golden(case)
        m = R.build(*case[:4])
        sd = m.state_dict()
        assert list(sd.keys()) == meta["keys"] == R.KEYS and len(sd) == 21
        assert [list(v.shape) for v in sd.values()] == meta["shapes"]
        assert [k for k, _ in m.named_parameters()] == R.PARAMS and [k for k, _ in m.named_buffers()] == R.BUFFERS
        assert sd["psi.1.num_batches_tracked"].dtype == torch.long
        want = R.fixture_inputs(case)[0]
        m.load_state_dict(want, strict=True)
        assert all(torch.equal(m.state_dict()[k], want[k]) for k in R.KEYS)
        m2 = copy.deepcopy(m)
        assert all(torch.equal(a, b) and a is not b for a, b in zip(m.state_dict().values(), m2.state_dict().values()))
        assert m.storage == torch.float32 and m.training and not m.eval().training
    with pytest.raises(RuntimeError):
        R.build(16, 16, 8).load_state_dict({**R.fixture_inputs(R.CASES[0])[0], "relu.weight": torch.ones(1)}, strict=True)


def test_initialisation_is_that_of_the_enclosing_networks():
    torch.manual_seed(0)
    m = R.build(512, 256, 384)
    sd = m.state_dict()
    # kaiming-normal, fan_out = out_channels of a 1x1x1 convolution: std = sqrt(2 / fan_out)
    assert abs(float(sd["W_g.0.weight"].std()) / (2.0 / 384) ** 0.5 - 1) < 0.05
    assert abs(float(sd["W_x.0.weight"].std()) / (2.0 / 384) ** 0.5 - 1) < 0.05
    assert abs(float(sd["psi.0.weight"].std()) / 2.0 ** 0.5 - 1) < 0.2
    # nn.Conv3d's default bias: uniform in +- 1 / sqrt(fan_in)
    assert float(sd["W_g.0.bias"].abs().max()) <= 512 ** -0.5 and float(sd["W_g.0.bias"].std()) > 0.3 * 512 ** -0.5
    assert float(sd["psi.0.bias"].abs().max()) <= 384 ** -0.5
    for b in ("W_g", "W_x"):
        assert abs(float(sd[b + ".1.weight"].mean()) - 1) < 0.01 and abs(float(sd[b + ".1.weight"].std()) / 0.02 - 1) < 0.2
        assert float(sd[b + ".1.bias"].abs().max()) == 0.0
        assert float(sd[b + ".1.running_mean"].abs().max()) == 0.0 and bool((sd[b + ".1.running_var"] == 1).all())
    assert abs(float(sd["psi.1.weight"]) - 1) < 0.1 and float(sd["psi.1.bias"]) == 0.0 and int(sd["psi.1.num_batches_tracked"]) == 0


def test_refusals():
    from brats21_amd import BratsHipError
    from brats21_amd.networks import AttentionBlock
    with pytest.raises(NotImplementedError, match="prelu"):
        AttentionBlock(16, 16, 8, "prelu")
    with pytest.raises(NotImplementedError):
        AttentionBlock(16, 16, 8, "gelu")
    for f_g, f_l in ((12, 16), (16, 20), (0, 16), (1032, 16), (16, 2048)):
        with pytest.raises(NotImplementedError, match="multiple of 8"):
            AttentionBlock(f_g, f_l, 8)
    for f_int in (0, -8, 513, 2.5):
        with pytest.raises(NotImplementedError, match="f_int"):
            AttentionBlock(16, 16, f_int)
    for f_int in (1, 3, 8, 12, 512):
        assert AttentionBlock(16, 16, f_int).f_int == f_int
    AttentionBlock(1024, 1024, 512)
    m = AttentionBlock(16, 8, 4)
    with pytest.raises(BratsHipError, match="GPU only"):
        m(torch.zeros(1, 16, 4, 4, 4), torch.zeros(1, 8, 4, 4, 4))  # no CPU fallback


def test_library_declares_the_passes_and_refuses_bad_arguments():
    from brats21_amd import _lib
    names = ["brats_attgate_blocks", "brats_attgate_psi_fwd", "brats_attgate_bn1", "brats_attgate_apply_fwd", "brats_attgate_apply_bwd",
             "brats_attgate_bn1_bwd", "brats_attgate_psi_bwd_stats", "brats_attgate_psi_bwd_finalize", "brats_attgate_psi_bwd_apply",
             "brats_attgate_dx"]
    assert set(names) <= set(_lib.declared_symbols())
    sigs = _lib._parse_header()
    assert sigs["brats_attgate_psi_fwd"] == ("i", "pipipppppiifiiip") and sigs["brats_attgate_bn1"] == ("i", "pidpppppfpp")
    assert sigs["brats_attgate_dx"] == ("i", "pipipppiiiiip") and sigs["brats_attgate_blocks"] == ("i", "iiii")
    assert _lib._header_abi_version() == 7
    l = _lib.lib()
    assert l.brats_abi_version() == 7
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    B, F, H = _lib.BF16, _lib.F32, _lib.F16

    def refused(rc, code, name):
        assert rc == code and name.encode() in l.brats_last_error(), (rc, l.brats_last_error())
    # NULL pointers
    refused(l.brats_attgate_psi_fwd(None, 8, p, 8, p, p, p, p, p, B, 1, 0.01, 1, 8, 8, None), -1, "attgate_psi_fwd")
    refused(l.brats_attgate_bn1(None, 1, 8.0, p, p, p, None, None, 1e-5, p, None), -1, "attgate_bn1")
    refused(l.brats_attgate_bn1(p, 1, 8.0, p, p, p, p, None, 1e-5, p, None), -1, "attgate_bn1")
    refused(l.brats_attgate_apply_fwd(p, 8, None, p, p, 8, B, 1, 8, 8, None), -1, "attgate_apply_fwd")
    refused(l.brats_attgate_apply_bwd(p, 8, p, 8, p, p, p, None, H, 1, 8, 8, None), -1, "attgate_apply_bwd")
    refused(l.brats_attgate_bn1_bwd(p, 1, 8.0, 1, None, None), -1, "attgate_bn1_bwd")
    refused(l.brats_attgate_psi_bwd_stats(p, 8, p, 8, p, p, p, p, p, p, p, p, None, p, B, 1, 0.01, 1, 8, 8, None), -1, "attgate_psi_bwd_stats")
    refused(l.brats_attgate_psi_bwd_finalize(p, 1, 8, 8.0, 1, p, None, None), -1, "attgate_psi_bwd_finalize")
    refused(l.brats_attgate_psi_bwd_apply(p, 8, p, 8, p, p, p, p, p, p, p, p, p, p, None, 8, p, 8, B, 1, 0.01, 1, 8, 8, None), -1,
            "attgate_psi_bwd_apply")
    refused(l.brats_attgate_dx(p, 8, None, 8, p, p, p, 8, F, 1, 8, 8, None), -1, "attgate_dx")
    # C or a pitch that is no multiple of the channel vector (8 in 16-bit storage, 4 in f32), a pitch below C
    refused(l.brats_attgate_psi_fwd(p, 12, p, 12, p, p, p, p, p, B, 1, 0.01, 1, 8, 12, None), -1, "attgate_psi_fwd")
    refused(l.brats_attgate_apply_fwd(p, 8, p, p, p, 12, H, 1, 8, 8, None), -1, "attgate_apply_fwd")
    refused(l.brats_attgate_apply_fwd(p, 6, p, p, p, 8, F, 1, 8, 6, None), -1, "attgate_apply_fwd")
    refused(l.brats_attgate_apply_bwd(p, 16, p, 8, p, p, p, p, B, 1, 8, 16, None), -1, "attgate_apply_bwd")
    refused(l.brats_attgate_psi_bwd_stats(p, 8, p, 4, p, p, p, p, p, p, p, p, p, p, B, 1, 0.01, 1, 8, 8, None), -1, "attgate_psi_bwd_stats")
    refused(l.brats_attgate_psi_bwd_apply(p, 8, p, 8, p, p, p, p, p, p, p, p, p, p, p, 8, p, 10, F, 1, 0.01, 1, 8, 8, None), -1,
            "attgate_psi_bwd_apply")
    refused(l.brats_attgate_dx(p, 8, p, 8, p, p, p, 4, B, 1, 8, 8, None), -1, "attgate_dx")
    refused(l.brats_attgate_psi_fwd(p, 8, p, 8, p, p, p, p, p, B, 9, 0.01, 1, 8, 8, None), -1, "attgate_psi_fwd")
    refused(l.brats_attgate_bn1_bwd(p, 0, 8.0, 1, p, None), -1, "attgate_bn1_bwd")
    # beyond the limits: 256 channel vectors, the split-precision codes
    refused(l.brats_attgate_apply_fwd(p, 1028, p, p, p, 1028, F, 1, 8, 1028, None), -2, "attgate_apply_fwd")
    refused(l.brats_attgate_dx(p, 2056, p, 2056, p, p, p, 2056, B, 1, 8, 2056, None), -2, "attgate_dx")
    refused(l.brats_attgate_psi_fwd(p, 8, p, 8, p, p, p, p, p, _lib.X3_BF16, 1, 0.01, 1, 8, 8, None), -2, "attgate_psi_fwd")
    assert l.brats_attgate_blocks(F, 1028, 1, 8) == -2 and l.brats_attgate_blocks(B, 12, 1, 8) == -1
    # the limits themselves, and the workgroup counts the partials are sized by
    assert l.brats_attgate_blocks(F, 1024, 2, 64) > 0 and l.brats_attgate_blocks(B, 512, 1, 2 ** 31 - 1) == 2048
    assert l.brats_attgate_blocks(B, 24, 2, 128 ** 3) == 2048 and l.brats_attgate_blocks(F, 8, 1, 65) == 1
    assert l.brats_attgate_blocks(H, 48, 1, 16 ** 3) == 25  # 42 voxel lanes x 4 voxels per workgroup and step


def test_the_networks_that_use_the_gate_are_still_not_built():
    from brats21_amd import get_model
    for name in ("att_unet", "r2attunet"):
        with pytest.raises(NameError):
            get_model(argparse.Namespace(model=name, width=8, norm="group", act="relu", num_classes=3, dropout=0))
