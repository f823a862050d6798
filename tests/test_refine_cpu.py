"""CPU checks of the refinement stage (``--model equiunet_ref``): the plain-torch restatement tests/_refine_ref.py equals the
reference's own class (tests/golden/refine_*.npz), the module's state dict is the reference's key by key, the factory and the
loss helpers handle the nested output, and the new entry points are declared."""
import argparse
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

import _refine_ref as R
from oracle import synth


def _golden(golden_dir, case):
    return np.load(os.path.join(golden_dir, R.fname(case)), allow_pickle=False)


@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_restatement_equals_the_reference_golden(golden_dir, case):
    """f32 on the fixture's closed-form weights: both heads, the deep heads and the six-head loss; the float64 evaluation is
    within the recorded ref_err_* of them."""
    g = _golden(golden_dir, case)
    meta = json.loads(str(g["meta"]))
    norm, act = case
    sd = synth.fill_state_dict(R.state_shapes(R.WIDTH, 4, 3, act, norm))
    assert list(sd) == meta["keys"] and [list(v.shape) for v in sd.values()] == meta["shapes"]
    x, t = R.image(), synth.nested_spheres(1, R.SIZE)
    with torch.no_grad():
        res = R.forward(sd, x, act=act, norm=norm)
        res64 = R.forward({k: v.double() if v.is_floating_point() else v for k, v in sd.items()}, x.double(), act=act, norm=norm)
    heads, heads64 = R.flat(res), R.flat(res64)
    zs = meta["out_z_stride"]
    want = [g["refined"], g["out"]] + [g[f"deep{i}"] for i in range(4)]
    cut = [lambda a: a, lambda a: a[:, :, ::zs]] + [lambda a: a[:, :, ::2, ::2, ::2]] * 4
    for h, h64, w, c in zip(heads, heads64, want, cut):
        assert np.abs(c(h.numpy()) - w).max() < 1e-4
    assert float((heads64[0].float() - torch.from_numpy(g["refined"])).abs().max()) <= float(g["ref_err_refined"]) + 1e-6
    assert abs(float(R.ds_loss(res, t)) - float(g["loss"])) < 1e-5
    assert float(np.abs(g["refined"][:, :, ::zs] - g["out"]).max()) > 1e-2, "the stage changes the logits"


@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_state_dict_is_the_references(golden_dir, case):
    meta = json.loads(str(_golden(golden_dir, case)["meta"]))
    m = R.build(case, load=False)
    sd = m.state_dict()
    assert list(sd.keys()) == meta["keys"]
    assert [list(v.shape) for v in sd.values()] == meta["shapes"]
    assert len(sd) == 92 and list(sd)[-2:] == ["refunet.conv_d0.weight", "refunet.conv_d0.bias"]
    # strict load of a reference-shaped checkpoint
    m.load_state_dict(synth.fill_state_dict(R.state_shapes(R.WIDTH, 4, 3, case[1], case[0])), strict=True)


def test_stage_is_registered_last_and_keeps_the_dropout_streams():
    """The units of the network without the stage keep their dropout stream ids; the stage's nine follow."""
    from brats21_amd.networks import EquiUnet
    with contextlib.redirect_stdout(io.StringIO()):
        plain = EquiUnet(4, 3, [8, 16, 32, 64], norm_layer="group", act="relu", deep_supervision=True, dropout=0.1)
        ref = R.build(load=False, dropout=0.1)
    names_plain = {n: plain._unit_ids[mod] for n, mod in plain.named_modules() if mod in plain._unit_ids}
    names_ref = {n: ref._unit_ids[mod] for n, mod in ref.named_modules() if mod in ref._unit_ids}
    assert all(names_ref[n] == i for n, i in names_plain.items())
    assert sorted(i for n, i in names_ref.items() if n.startswith("refunet.")) == list(range(len(names_plain), len(names_plain) + 9))


def test_kaiming_init_covers_the_two_end_convolutions():
    torch.manual_seed(0)
    m = R.build(load=False, width=16)
    # kaiming-normal, fan_out = cout * 27: std = sqrt(2 / fan_out)
    for conv in (m.refunet.conv0, m.refunet.conv_d0):
        w = conv.weight.detach()
        want = (2.0 / (w.shape[0] * 27)) ** 0.5
        assert 0.8 * want < float(w.std()) < 1.2 * want
        bound = 1.0 / (w.shape[1] * 27) ** 0.5  # torch's default bias init
        assert float(conv.bias.detach().abs().max()) <= bound


def _ns(model):
    return argparse.Namespace(model=model, width=8, norm="group", act="relu", num_classes=3, dropout=0)


def test_get_model_builds_the_stage():
    from brats21_amd import get_model
    from brats21_amd.networks.equiunet import RefUnet
    with contextlib.redirect_stdout(io.StringIO()):
        m = get_model(_ns("equiunet_ref"))
        plain = get_model(_ns("equiunet"))
    assert m.refinement and isinstance(m.refunet, RefUnet) and m.deep_supervision
    assert not plain.refinement and not hasattr(plain, "refunet")
    with pytest.raises((NameError, NotImplementedError, AttributeError)):
        get_model(_ns("equiunet_assp_evo_ref"))
    with pytest.raises(NameError):
        get_model(_ns("equiunet_reff"))


def test_loss_helpers_average_six_heads_on_nested_outputs():
    """Pure-torch DiceLoss path on CPU tensors: ([refined, out], [deep x 4]) -> the mean over the six heads in that order, the
    refined head returned as the output; [refined, out] without deep supervision -> the mean over the two."""
    from brats21_amd.losses import DiceLoss, deep_supervision_loss, flatten_heads
    g = torch.Generator().manual_seed(1)
    heads = [torch.randn((1, 3, 8, 8, 8), generator=g) for _ in range(6)]
    t = (torch.rand((1, 3, 8, 8, 8), generator=g) > 0.5).float()
    crit = DiceLoss()
    each = [crit(h, t) for h in heads]
    nested = ([heads[0], heads[1]], heads[2:])
    assert [id(h) for h in flatten_heads(nested)] == [id(h) for h in heads]
    loss, first = deep_supervision_loss(crit, nested, t)
    assert first is heads[0] and torch.equal(loss, torch.stack(each).mean())
    loss2, first2 = deep_supervision_loss(crit, [heads[0], heads[1]], t)
    assert first2 is heads[0] and torch.equal(loss2, torch.stack(each[:2]).mean())
    # the outputs of the network without the stage are treated as before
    loss3, first3 = deep_supervision_loss(crit, (heads[1], heads[2:]), t)
    assert first3 is heads[1] and torch.equal(loss3, torch.stack(each[1:]).mean())
    loss4, first4 = deep_supervision_loss(crit, heads[1], t)
    assert first4 is heads[1] and torch.equal(loss4, each[1])


def test_prepared_loss_flattens_too():
    from brats21_amd.losses import deep_supervision_prepared_loss

    class Crit:
        def prepare(self, target):
            return target * 2.0

        def __call__(self, h, prep):
            return (h - prep).abs().mean()

    g = torch.Generator().manual_seed(2)
    heads = [torch.randn((1, 3, 4, 4, 4), generator=g) for _ in range(6)]
    t = torch.randn((1, 3, 4, 4, 4), generator=g)
    loss, first = deep_supervision_prepared_loss(Crit(), ([heads[0], heads[1]], heads[2:]), t)
    assert first is heads[0] and torch.equal(loss, torch.stack([(h - 2.0 * t).abs().mean() for h in heads]).mean())


def test_inferers_first_digs_to_the_refined_head():
    from brats21_amd.inferers import _first
    a, b, c = torch.zeros(1), torch.ones(1), torch.ones(2)
    assert _first(([a, b], [c])) is a and _first([a, b]) is a and _first((b, [c])) is b and _first(c) is c


def test_new_symbols_are_declared_and_the_abi_version_stands():
    from brats21_amd import _lib
    names = _lib.declared_symbols()
    for sym in ("brats_conv3d_narrow_packed_bytes", "brats_conv3d_narrow_pack", "brats_conv3d_narrow_fwd"):
        assert sym in names
    sigs = _lib._parse_header()
    assert sigs["brats_conv3d_narrow_packed_bytes"] == ("z", "ii")
    assert sigs["brats_conv3d_narrow_pack"] == ("i", "ppiiip")
    assert sigs["brats_conv3d_narrow_fwd"] == ("i", "pii" + "pppp" + "iiiiii" + "p")
    assert _lib._header_abi_version() == 7
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.lib()
        assert lib.brats_abi_version() == _lib._header_abi_version()
        frag = lambda c: 2 * (c // 8) * 7 * 64 * 8 * 2                              # the bf16 and the fp16 MFMA fragments
        assert lib.brats_conv3d_narrow_packed_bytes(48, 3) == 48 * 27 * 4 * 4 + frag(48)      # class tile 4
        assert lib.brats_conv3d_narrow_packed_bytes(8, 16) == 8 * 27 * 16 * 4 + frag(8)
        assert lib.brats_conv3d_narrow_packed_bytes(12, 3) == 0 and lib.brats_conv3d_narrow_packed_bytes(8, 17) == 0


def test_input_rule_is_named_before_anything_runs_on_the_gpu():
    """(the divisible-by-16 rule itself is checked on the GPU: tests/test_refine_gpu.py::test_refused_configurations)"""
    from brats21_amd._lib import BratsHipError
    m = R.build(load=False)
    with pytest.raises(BratsHipError):
        m(torch.zeros(1, 4, 32, 32, 32))  # a CPU tensor: no fallback
