"""-m "not gpu": AttUnet's and R2AttUnet's contract without a GPU.  tests/_attunet_ref.py (the float64 restatement the GPU tests are
held against) reproduces tests/golden/attunet_w8_*.npz and r2attunet_w8_*.npz -- the reference's own classes, run by
tests/golden/make_golden_attunet.py -- to 1e-12 where the fixtures hold float64 (training-mode heads, loss, gradients and BatchNorm
buffers; eval-mode heads) and within the recorded float32 error of the reference elsewhere; brats21_amd.networks.AttUnet / R2AttUnet
have the fixtures' state-dict names, shapes and order (139 / 153 keys), load them with strict=True and refuse what they do not
build; get_model still does not know the names; brats_attgate_dx_unpool is declared, exported, bound and refuses bad arguments."""
import argparse
import contextlib
import copy
import ctypes
import io

import numpy as np
import pytest
import torch

import _attunet_ref as R

KIND_CASES = [(k, c) for k in R.KINDS for c in R.CASES]
KC_IDS = [f"{k}-{i}" for k in R.KINDS for i in R.IDS]


@pytest.mark.parametrize("kind,case", KIND_CASES, ids=KC_IDS)
def test_restatement_reproduces_the_reference_fixture(kind, case):
    z, meta = R.golden(kind, case)
    heads, loss, grads, buffers = R.fixture_run64(kind, case)
    keys = meta["keys"]
    names = [k for k in keys if not R.is_buffer(k)]
    assert (len(keys), len(names)) == R.NKEYS[kind] and names == list(grads) and meta["kind"] == kind
    assert meta["scales"] == list(R.SCALES) and meta["t"] == R.T and meta["seed"] == 28 and meta["gain"] == R.GAIN.get((kind, case), 1.2)
    assert "x" not in z.files, "the input regenerates from the seed"
    # float64 entries: the reference class in float64 (scaled as tests/test_r2unet_cpu.py scales them)
    assert abs(loss - float(z["loss64"])) <= 1e-12
    assert float(np.abs(heads[0].numpy()[:, :, ::2, ::2, ::2] - z["d1_64"]).max()) <= 1e-12
    norms = np.array([float(grads[n].norm()) for n in names])
    assert float(np.abs(norms - z["grad_norms64"]).max()) <= 1e-12 * max(1.0, float(z["grad_norms64"].max()))
    g64 = [k for k in z.files if k.startswith("grad64:")]
    assert g64
    for k in g64:
        assert float(np.abs(grads[k[7:]].numpy() - z[k]).max()) <= 1e-12 * max(1.0, float(np.abs(z[k]).max())), k
    bufs = [k for k in keys if R.is_buffer(k)]
    assert len(bufs) == 27 and sorted(buffers) == sorted(bufs)
    for k in bufs:
        assert float(np.abs(buffers[k].double().numpy() - z["buf64:" + k]).max()) <= 1e-12, k
    ev = R.fixture_run64(kind, case, training=False)[0]
    assert float(np.abs(ev[0].numpy()[:, :, ::2, ::2, ::2] - z["eval_d1_64"]).max()) <= 1e-12
    # float32 entries: within the reference's own recorded float32 error (the fixture's entries ARE that error's other side)
    for i, s in enumerate(R.SCALES):
        h = heads[i].numpy()
        assert h.shape == (R.BATCH, 3, *R.SIZE)
        assert float(np.abs(h[:, :, ::s, ::s, ::s] - z[f"d{i + 1}"]).max()) <= float(z["ref_err_heads"]) * (1 + 1e-6)
        assert float(np.abs(ev[i].numpy()[:, :, ::s, ::s, ::s] - z[f"eval_d{i + 1}"]).max()) <= float(z["ref_err_eval"]) * (1 + 1e-6)
    assert abs(loss - float(z["loss"])) <= float(z["ref_err_loss"]) * (1 + 1e-6) + 1e-15
    live = [i for i, n in enumerate(names) if norms[i] > 1e-9]
    assert float(np.abs(z["grad_norms"][live] / norms[live] - 1).max()) <= float(z["ref_err_gnorm_rel"]) * (1 + 1e-6)
    for k in (k for k in z.files if k.startswith("grad:")):
        g = grads[k[5:]].numpy()
        if np.abs(g).max() > 1e-9:
            assert float(np.abs(g - z[k]).max() / np.abs(g).max()) <= float(z["ref_err_grad_small"]) * (1 + 1e-6), k
        else:  # zero in exact arithmetic (a convolution bias in front of a per-channel normalisation or a training-mode BatchNorm)
            assert k.endswith(".bias") and float(np.abs(z[k]).max()) <= float(z["ref_err_grad_dead"])
    for k in bufs:
        if k.endswith("num_batches_tracked"):
            assert int(z["buf:" + k]) == int(buffers[k]) == 1
        else:
            assert float(np.abs(buffers[k].numpy() - z["buf:" + k]).max()) <= float(z["ref_err_buf:" + k]) * (1 + 1e-6) + 1e-15, k
    # the room under the bars of tests/test_attunet_gpu.py the generator asserted
    assert float(z["ref_err_heads"]) < 2.5e-4 and float(z["ref_err_loss"]) < 2.5e-5
    assert float(z["ref_err_gnorm_rel"]) < 2e-3 and float(z["ref_err_grad_small"]) < 2e-3
    # zero in exact arithmetic: the family's convolution biases in front of a per-channel normalisation, and the three convolution
    # biases of every gate (in front of a training-mode BatchNorm)
    dead = [n for i, n in enumerate(names) if i not in live]
    gate_bias = [f"{g}.{b}.0.bias" for g in R.GATES for b in ("W_g", "W_x", "psi")]
    assert [n for n in dead if n.startswith("Att")] == gate_bias
    family = [n for n in dead if not n.startswith("Att")]
    conv_bias = [n for n in names if n.endswith(("conv.0.bias", "conv.3.bias", "up.1.bias")) and not n.startswith("Att")]
    if case[0] == "group":  # (8 groups of ONE channel in the 8-wide units: a per-channel normalisation there)
        assert family == [n for n in conv_bias if n.split(".")[0] in ("Conv1", "RRCNN1", "Up2", "Up_conv2", "Up_RRCNN2")]
        assert len(family) == 5
    else:
        assert family == conv_bias and len(family) == 17  # (7 blocks of two units and the 3 UpConv units, in both networks)


@pytest.mark.parametrize("kind,case", KIND_CASES, ids=KC_IDS)
def test_module_state_dict_is_the_references(kind, case):
    _, meta = R.golden(kind, case)
    nkeys, nparams = R.NKEYS[kind]
    m = R.build(kind, case, load=False)
    sd = m.state_dict()
    assert list(sd.keys()) == meta["keys"] and len(sd) == nkeys
    assert [list(v.shape) for v in sd.values()] == meta["shapes"]
    names = [k for k in meta["keys"] if not R.is_buffer(k)]
    assert [n for n, _ in m.named_parameters()] == names and len(names) == nparams
    assert [n for n, _ in m.named_buffers() if not n.startswith("_dropout")] == [k for k in meta["keys"] if R.is_buffer(k)]
    # the reference's order: Up4, Att4, the decoder block, Up3, ...
    tops = []
    for k in meta["keys"]:
        if k.split(".")[0] not in tops:
            tops.append(k.split(".")[0])
    dec = ("Up_conv", "Up_RRCNN")[kind == "r2attunet"]
    assert tops[4:13] == ["Up4", "Att4", dec + "4", "Up3", "Att3", dec + "3", "Up2", "Att2", dec + "2"]
    want = R.fixture_weights(kind, case)
    m.load_state_dict(want, strict=True)
    assert all(torch.equal(m.state_dict()[k], want[k]) for k in want)
    assert (m.Att4.f_g, m.Att4.f_l, m.Att4.f_int) == (32, 32, 16) and (m.Att3.f_int, m.Att2.f_int) == (8, 4) and m.Att2.act == case[1]
    m2 = copy.deepcopy(m)
    assert all(torch.equal(a, b) and a is not b for a, b in zip(m.state_dict().values(), m2.state_dict().values()))
    assert m2.precision == "fp32" and m2.Up4.units[0].conv is m2.Up4.up["1"] and m2.Up4.units[0].conv is not m.Up4.up["1"]
    # without deep supervision the three deep heads' six keys are gone
    plain = R.build(kind, case, deep_supervision=False, load=False)
    assert list(plain.state_dict()) == meta["keys"][:-6]
    # train() / eval() on the network reach the gates
    assert m.training and m.Att3.training
    m.eval()
    assert not m.training and not any(g.training for g in (m.Att4, m.Att3, m.Att2))
    m.train()
    assert all(g.training for g in (m.Att4, m.Att3, m.Att2))


def test_the_reference_prints_are_kept():
    from brats21_amd.networks import AttUnet, R2AttUnet
    for cls in (AttUnet, R2AttUnet):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            cls(4, 3, [8, 16, 32, 64])
        assert buf.getvalue().splitlines() == [f"{cls.__name__} features: [8, 16, 32, 64]", "initialize network with kaiming"]


@pytest.mark.parametrize("model", ["att_unet", "r2attunet", "attunet", "r2att_unet"])
def test_get_model_still_does_not_know_the_names(model):
    from brats21_amd import get_model
    ns = argparse.Namespace(model=model, width=8, norm="group", act="relu", num_classes=3, dropout=0)
    with pytest.raises(NameError, match="Not Supported Model"):
        get_model(ns)


def _make(kind, **kw):
    from brats21_amd.networks import AttUnet, R2AttUnet
    args = dict(img_ch=4, output_ch=3, features=[8, 16, 32, 64])
    args.update(kw)
    with contextlib.redirect_stdout(io.StringIO()):
        return (AttUnet if kind == "attunet" else R2AttUnet)(**args)


@pytest.mark.parametrize("kind", R.KINDS)
def test_refusals(kind):
    from brats21_amd import BratsHipError
    for norm in ("batch", "bcn", "none"):
        with pytest.raises(NotImplementedError, match=norm):
            _make(kind, norm_layer=norm)
    with pytest.raises(NotImplementedError, match="layer"):
        _make(kind, norm_layer="layer")
    with pytest.raises(NotImplementedError, match="prelu"):
        _make(kind, act="prelu")
    with pytest.raises(NotImplementedError, match="gelu"):
        _make(kind, act="gelu")
    for act in ("relu", "leakyrelu", "elu", "swish", "mish"):
        _make(kind, act=act, norm_layer="instance")
    if kind == "r2attunet":
        for t in (0, -1, 1.5):
            with pytest.raises(ValueError, match="t must be an integer >= 1"):
                _make(kind, t=t)
    else:
        with pytest.raises(TypeError):
            _make(kind, t=2)
    with pytest.raises(NotImplementedError, match="multiples of 8"):
        _make(kind, features=[4, 8, 16, 32])
    with pytest.raises(ValueError, match="four widths"):
        _make(kind, features=[8, 16, 32])
    with pytest.raises(NotImplementedError, match="inplanes <= 16"):
        _make(kind, img_ch=17)
    with pytest.raises(NotImplementedError, match="num_classes <= 16"):
        _make(kind, output_ch=17)
    with pytest.raises(NotImplementedError, match="AttentionBlock: f_int"):  # the gate's own limit: Att4 would have f_int = 520 > 512
        _make(kind, features=[8, 520, 8, 8])
    m = _make(kind)
    x = torch.zeros(1, 4, 16, 16, 16)
    with pytest.raises(BratsHipError, match="GPU only"):
        m(x)
    for precision in ("x3", "fp16x3", "bf16x3", "x3fwd", "x3bwd"):
        m.precision = precision
        with pytest.raises(NotImplementedError, match="split-precision"):
            m(x)
    m.precision = "auto"
    m.conv_fp8 = "fwd"
    with pytest.raises(NotImplementedError, match="e4m3"):
        m(x)


def test_the_new_entry_point_is_declared_exported_and_refuses_bad_arguments():
    from brats21_amd import _lib
    name = "brats_attgate_dx_unpool"
    sigs = _lib._parse_header()
    # dout, dopitch, t, tpitch, q, st1, argmax, d_pooled, dppitch, out, opitch, dtype, N, C, D, H, W, stream
    assert sigs[name] == ("i", "pipi" + "ppp" + "pipi" + "iiiiii" + "p")
    assert name in _lib.declared_symbols()
    l = _lib.lib()
    assert l.brats_abi_version() == 7 == _lib._header_abi_version()
    fn = getattr(l, name)
    assert fn.argtypes is not None and len(fn.argtypes) == len(sigs[name][1]) == 18
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for sym in (name, name + "_bf16", name + "_f16"):  # the public entry and its two storage builds
        assert getattr(raw, sym) is not None
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    args = ("dout", "t", "q", "st1", "argmax", "d_pooled", "out")

    def call(dtype=_lib.BF16, c=8, dims=(2, 2, 2), n=1, pitches=None, **ptrs):
        a = {k: ptrs.get(k, p) for k in args}
        dp, tp, pp, op = pitches or (c, c, c, c)
        return fn(a["dout"], dp, a["t"], tp, a["q"], a["st1"], a["argmax"], a["d_pooled"], pp, a["out"], op, dtype, n, c, *dims, None)

    def refused(rc, code, *words):
        msg = l.brats_last_error()
        return rc == code and b"attgate_dx_unpool" in msg and all(w in msg for w in words)

    for arg in args:
        assert refused(call(**{arg: None}), -1, b"null"), arg
    for dtype in (_lib.BF16, _lib.F16, _lib.F32):
        vw = 4 if dtype == _lib.F32 else 8
        assert refused(call(dtype=dtype, c=vw + 2), -1, b"multiple of %d" % vw)
        for i in range(4):  # a misaligned pitch, a pitch below C
            assert refused(call(dtype=dtype, c=vw, pitches=[vw + (2 if j == i else 0) for j in range(4)]), -1, b"pitch")
            assert refused(call(dtype=dtype, c=2 * vw, pitches=[vw if j == i else 2 * vw for j in range(4)]), -1, b"pitch")
        assert refused(call(dtype=dtype, c=257 * vw), -2, b"beyond")
        for dims in ((3, 2, 2), (2, 3, 2), (2, 2, 3), (0, 2, 2)):
            assert refused(call(dtype=dtype, c=vw, dims=dims), -1, b"even")
        assert refused(call(dtype=dtype, c=vw, n=0), -1)
        assert refused(call(dtype=dtype, c=vw, n=65536), -1, b"65535")
    assert refused(call(dtype=7), -2, b"dtype")
