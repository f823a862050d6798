"""-m "not gpu": EquiUnet / EquiUnetASSPEvo with input-channel and class counts other than BraTS' (4, 3) -- construction, the
state dict against the oracle's shape functions and the fixtures of tests/golden/make_golden_general.py, the refusals, and the
CPU oracle pinned at the new shapes against those fixtures (the bars of tests/test_oracle_golden.py)."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import _general_cases as G
from oracle import synth, unet

TOL = 2e-5  # tests/test_oracle_golden.py: fp32 CPU vs fp32 CPU, same ATen kernels, different op grouping


def _golden(golden_dir, case):
    return np.load(os.path.join(golden_dir, G.fname(case)), allow_pickle=False)


@pytest.mark.parametrize("case", G.CASES, ids=G.IDS)
def test_constructs_with_the_reference_state_dict(golden_dir, case):
    m = G.build(case, load=False)
    want = G.shapes(case)
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert list(got) == list(want) and all(got[k] == tuple(want[k]) for k in want)
    meta = json.loads(str(_golden(golden_dir, case)["meta"]))
    assert list(got) == meta["keys"] and [list(s) for s in got.values()] == meta["shapes"]
    assert (meta["inplanes"], meta["num_classes"]) == case[2:] and m.inplanes == case[2]
    m.load_state_dict(synth.fill_state_dict(want), strict=True)
    twin = copy.deepcopy(m)
    assert twin.inplanes == m.inplanes
    for (ka, a), (kb, b) in zip(m.state_dict().items(), twin.state_dict().items()):
        assert ka == kb and torch.equal(a, b) and (a.dim() == 0 or a.data_ptr() != b.data_ptr())


@pytest.mark.parametrize("model", ["equiunet", "equiunet_assp_evo"])
@pytest.mark.parametrize("k", [5, 16])
def test_get_model_takes_num_classes(model, k):
    from brats21_amd import get_model
    m = get_model(G.namespace(model, 16, k))
    head = m.outconv if model == "equiunet" else m.out_conv
    assert head.weight.shape[0] == k and m.inplanes == 4
    assert all(h[0].weight.shape[0] == k for n, h in m.named_children() if n.startswith("deep"))


@pytest.mark.parametrize("net", ["equiunet", "assp"])
def test_refusals_name_the_limit(net):
    def make(c, k, width=16):
        return G.build((net, width, c, k), load=False)

    with pytest.raises(NotImplementedError, match="num_classes <= 16"):
        make(4, 17)
    with pytest.raises(NotImplementedError, match="inplanes <= 16"):
        make(17, 3)
    with pytest.raises((NotImplementedError, ValueError)):
        make(0, 3)
    with pytest.raises((NotImplementedError, ValueError)):
        make(4, 0)
    with pytest.raises(NotImplementedError, match="multiples of"):
        make(4, 3, width=12 if net == "equiunet" else 24)
    make(16, 16)  # the limits themselves construct


def test_input_padding():
    """The NDHWC network input: 8 or 16 channels in the 16-bit and split-precision modes, 4, 8 or 16 in exact f32."""
    from brats21_amd import ops
    from brats21_amd.networks._program import input_cpad
    for c in range(1, 17):
        assert input_cpad(c, torch.bfloat16) == input_cpad(c, torch.float16) == (8 if c <= 8 else 16)
        assert input_cpad(c, torch.float32) == (4 if c <= 4 else 8 if c <= 8 else 16)
        with ops.split_precision(ops.X3F):
            assert input_cpad(c, torch.float32) == (8 if c <= 8 else 16)


@pytest.mark.parametrize("case", G.CASES, ids=G.IDS)
def test_oracle_matches_reference_at_the_new_shapes(golden_dir, case):
    g = _golden(golden_dir, case)
    sd = {k: v.requires_grad_(True) for k, v in synth.fill_state_dict(G.shapes(case)).items()}
    out = G.oracle_forward(case)(sd, G.image(case))
    loss = unet.deep_supervision_loss(out, G.nested_targets(1, case[3]))
    loss.backward()
    assert tuple(out[0].shape) == (1, case[3], *G.SIZE)
    np.testing.assert_allclose(out[0].detach().numpy(), g["logits"], atol=TOL, rtol=0)
    for i, d in enumerate(out[1]):
        np.testing.assert_allclose(d.detach().numpy()[:, :, ::2, ::2, ::2], g[f"deep{i}"], atol=TOL, rtol=0)
    assert abs(loss.item() - float(g["loss"])) < 1e-6
    names = json.loads(str(g["grad_names"]))
    norms = np.array([float(sd[k].grad.double().norm()) for k in names])
    np.testing.assert_allclose(norms, g["grad_norms"], rtol=2e-4, atol=1e-9)
    if case[0] == "equiunet":  # (test_oracle_golden.py compares the small gradients of this network element by element)
        for k in g.files:
            if k.startswith("grad:"):
                np.testing.assert_allclose(sd[k[5:]].grad.numpy(), g[k], atol=1e-6, rtol=1e-4)
    # the bars of the GPU tests have room: the reference's own f32 error against the f64 oracle, recorded with the case
    assert float(g["ref_err_logits"]) < 1e-4 and float(g["ref_err_deep"]) < 1e-4 and float(g["ref_err_loss"]) < 1e-5
    assert float(g["ref_err_grad_rel"]) < 2e-4
