"""No GPU: the golden fixture of tests/golden/make_golden_agc.py (the reference's AGC, torch's clip_grad_norm_) against the
float64 restatement tests/_agc_ref.py that the GPU tests use, and the host side of brats21_amd.optim.AGC / clip_grad_norm_ and
definer.make_optimizer."""
import argparse
import ast
import os

import numpy as np
import pytest
import torch

import _agc_ref as R

RTOL = 1e-5  # the bar of tests/test_gradclip_gpu.py (derived there)


def load_case(golden_dir, name):
    """-> (params, grads, max_norm, clipping, eps, reference outputs f32, float64 outputs rounded to f32, z) with None for the
    parameter without a gradient; shared with the GPU test."""
    z = np.load(os.path.join(golden_dir, "agc.npz"))
    n = len(z["shapes"])
    params = [torch.from_numpy(z[f"param{i}"]) for i in range(n)]
    assert [tuple(p.shape) for p in params] == [ast.literal_eval(str(s)) for s in z["shapes"]]
    src = str(z["grad_source"][list(z["cases"]).index(name)])
    mul, key = (2.0, src[1:]) if src.startswith("2") else (1.0, src)
    grads = [torch.from_numpy(z[f"grad_{key}{i}"]) * mul if z["has_grad"][i] else None for i in range(n)]
    opt = lambda v: None if float(v) < 0 else float(v)  # noqa: E731
    max_norm, clipping, eps = opt(z[f"{name}__max_norm"]), opt(z[f"{name}__clipping"]), opt(z[f"{name}__eps"])
    ref, f64 = [], []
    for i in range(n):
        if not z["has_grad"][i]:
            ref.append(None), f64.append(None)
        elif name == "d":  # no clipping: the output is the input (asserted by the generator)
            ref.append(grads[i]), f64.append(grads[i])
        else:
            ref.append(torch.from_numpy(z[f"{name}__out{i}"]))
            f64.append(torch.from_numpy(z[f"{name}__out{i}__f64"]) if clipping is not None
                       else (grads[i].double() * float(z[f"{name}__clip_coef__f64"])).float())
    return params, grads, max_norm, clipping, eps, ref, f64, z


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_reference_result_matches_the_float64_restatement(golden_dir, name):
    params, grads, max_norm, clipping, eps, ref, f64, z = load_case(golden_dir, name)
    live = [i for i, g in enumerate(grads) if g is not None]
    assert len(live) == len(grads) - 1
    out, total, coef, trig, ratio = R.clip_then_agc([params[i] for i in live], [grads[i] for i in live], max_norm, clipping,
                                                    eps if eps is not None else 0.0)
    for k, i in enumerate(live):
        assert torch.equal(out[k].float(), f64[i]), (name, i)           # the stored float64 side is this module's
        np.testing.assert_allclose(ref[i].numpy(), out[k].float().numpy(), rtol=RTOL, atol=0)
    if max_norm is not None:
        np.testing.assert_allclose(float(z[f"{name}__total_norm"]), float(total), rtol=RTOL, atol=0)
        assert float(total) == float(z[f"{name}__total_norm__f64"])
        assert (float(coef) < 1) == (name != "d")
    if clipping is not None:
        for t, r in zip(trig, ratio):
            assert not bool(((r >= 0.95) & (r <= 1.05)).any())
            if t.numel() > 1:
                assert 4 * int(t.sum()) >= t.numel() and 4 * int((~t).sum()) >= t.numel()
        i, u = (int(v) for v in z["zero_grad_unit"])
        assert float(grads[i][u].abs().max()) == 0 and not bool(trig[live.index(i)][u])
    if name == "b":  # the max(grad_norm, 1e-6) branch is reached
        assert sum(int((t & (R.unitwise_norm(grads[i].double()).reshape(-1) < 1e-6)).sum()) for t, i in zip(trig, live)) > 10


def test_unit_layout_is_unitwise_norms():
    from brats21_amd.optim import unit_layout
    assert unit_layout((5, 24, 3, 3, 3)) == (5, 648, 1)
    assert unit_layout((4, 3, 2, 2)) == (4, 12, 1)
    assert unit_layout((6, 10)) == (10, 6, 10)
    assert unit_layout((1, 8, 1)) == (8, 1, 8)
    assert unit_layout((7,)) == (1, 7, 1) and unit_layout(()) == (1, 1, 1) and unit_layout((1, 16, 1, 1, 1)) == (1, 16, 1)
    with pytest.raises(ValueError, match="Wrong input dimensions"):
        unit_layout((2, 2, 2, 2, 2, 2))
    assert unit_layout((2, 3, 2, 2, 2, 2), agc=False) == (2, 48, 1)  # global-norm clipping takes any rank, as torch does
    for shape in [(5, 24, 3, 3, 3), (6, 10), (1, 8, 1), (7,), (3, 4, 5, 6)]:
        assert unit_layout(shape)[0] == R.unitwise_norm(torch.ones(shape)).numel()


def test_agc_constructor_errors_and_shared_state():
    from brats21_amd.optim import AGC
    m = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.Linear(4, 2))
    sgd = torch.optim.SGD(m.parameters(), lr=0.1, momentum=0.9)
    with pytest.raises(ValueError, match="Invalid clipping value"):
        AGC(m.parameters(), sgd, clipping=-1.0)
    with pytest.raises(ValueError, match="Invalid eps value"):
        AGC(m.parameters(), sgd, eps=-1e-3)
    with pytest.raises(ModuleNotFoundError, match="fc"):
        AGC(m.parameters(), sgd, model=m)  # the default ignore_agc names a module this model does not have
    with pytest.raises(ValueError, match="Wrong input dimensions"):
        AGC([torch.nn.Parameter(torch.zeros(2, 2, 2, 2, 2, 2))], sgd)
    agc = AGC(m.parameters(), sgd)
    assert agc.param_groups is sgd.param_groups and agc.state is sgd.state
    assert agc.clipping == 1e-2 and agc.eps == 1e-3 and agc.optim is sgd
    assert isinstance(agc, torch.optim.Optimizer)
    assert not agc._step_supports_amp_scaling and not agc.capturable
    assert AGC(m.parameters(), torch.optim.Adam(m.parameters(), capturable=True)).capturable
    # state_dict / load_state_dict / zero_grad pass through; load_state_dict replaces the wrapped optimizer's objects
    for p in m.parameters():
        p.grad = torch.ones_like(p)
    sgd.step()
    sd = agc.state_dict()
    assert sd["state"].keys() == sgd.state_dict()["state"].keys() and len(sd["state"]) == 4
    agc.load_state_dict(sd)
    assert agc.param_groups is sgd.param_groups and agc.state is sgd.state
    agc.zero_grad()
    assert all(float(p.grad.abs().max()) == 0 for p in m.parameters())
    agc.zero_grad(set_to_none=True)
    assert all(p.grad is None for p in m.parameters())
    sched = torch.optim.lr_scheduler.StepLR(agc, step_size=1, gamma=0.5)  # a scheduler drives the wrapped optimizer's groups
    sched.step()
    assert sgd.param_groups[0]["lr"] == 0.05


def test_agc_materialises_generator_params_and_takes_model_parameters_once():
    from brats21_amd.optim import AGC

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.body = torch.nn.Sequential(torch.nn.Conv3d(2, 3, 3), torch.nn.Conv3d(3, 3, 1))
            self.fc = torch.nn.Linear(3, 2)

    m = Net()
    sgd = torch.optim.SGD(m.parameters(), lr=0.1)
    agc = AGC(m.parameters(), sgd)  # a generator, as at the reference's call site
    first = list(agc.agc_params[0]["params"])
    assert len(first) == 6 and all(a is b for a, b in zip(first, m.parameters()))
    agc.step()  # (no gradients: nothing to clip, the wrapped optimizer steps)
    agc.step()
    assert len(agc.agc_params[0]["params"]) == 6 and all(a is b for a, b in zip(agc.agc_params[0]["params"], first))
    # model=: the reference collects module.parameters() of every module but the ignored ones (the root included): each once
    agc = AGC(None, sgd, model=m)
    got = agc.agc_params[0]["params"]
    assert len(got) == len({id(p) for p in got}) == 6 and {id(p) for p in got} == {id(p) for p in m.parameters()}
    with pytest.raises(ModuleNotFoundError, match="head"):
        AGC(None, sgd, model=m, ignore_agc=["head"])


def test_cpu_tensors_raise():
    from brats21_amd._lib import BratsHipError
    from brats21_amd.optim import AGC, clip_grad_norm_
    p = torch.nn.Parameter(torch.ones(4, 3))
    p.grad = torch.ones(4, 3)
    with pytest.raises(BratsHipError, match="GPU"):
        clip_grad_norm_([p], 1.0)
    with pytest.raises(BratsHipError, match="GPU"):
        AGC([p], torch.optim.SGD([p], lr=0.1)).step()
    with pytest.raises(NotImplementedError):
        clip_grad_norm_([p], 1.0, norm_type=1.0)
    with pytest.raises(NotImplementedError):
        clip_grad_norm_([p], 1.0, error_if_nonfinite=True)
    q = torch.nn.Parameter(torch.ones(3))  # no gradient anywhere: torch returns a zero norm
    assert float(clip_grad_norm_([q], 1.0)) == 0.0


def test_new_symbols_are_declared_and_the_abi_version_stays():
    from brats21_amd import _lib
    names = _lib.declared_symbols()
    assert "brats_gradclip" in names and "brats_gradclip_chunk" in names
    assert _lib._parse_header()["brats_gradclip"] == ("i", "pipipippfffppp")
    assert _lib._header_abi_version() == 7


def test_clip_record_matches_the_header_struct():
    import re
    from brats21_amd import _lib, optim
    txt = open(_lib.HEADER_PATH).read()
    body = re.search(r"typedef struct \{([^}]*)\} brats_gradclip_tensor;", txt).group(1)
    fields = [f.strip().split()[-1].lstrip("*") for f in body.split(";") if f.strip()]
    assert fields == list(optim._CLIP_REC.names) and optim._CLIP_REC.itemsize == 40


def test_make_optimizer_names_keywords_and_errors():
    from brats21_amd.definer import make_optimizer
    from brats21_amd.optim import Ranger2020
    m = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.Linear(4, 2))
    m[1].bias.requires_grad_(False)  # the factory takes the trainable parameters only
    ns = dict(learning_rate=3e-4, weight_decay=1e-5, use_gc=True, use_gcnorm=False, normloss=False, normloss_factor=1e-4,
              gc_conv_only=False)
    for name, cls, want in (("sgd", torch.optim.SGD, {"momentum": 0.9}),
                            ("adam", torch.optim.Adam, {"betas": (0.9, 0.999), "eps": 1e-8}),
                            ("adamw", torch.optim.AdamW, {"betas": (0.9, 0.999), "eps": 1e-8}),
                            ("ranger", Ranger2020, {"alpha": 0.5, "k": 6, "N_sma_threshhold": 5, "betas": (.95, 0.999), "eps": 1e-5})):
        opt = make_optimizer(argparse.Namespace(optimizer=name, **ns), m)
        assert type(opt) is cls
        g = opt.param_groups[0]
        assert g["lr"] == 3e-4 and g["weight_decay"] == 1e-5 and len(g["params"]) == 3
        for k, v in want.items():
            assert g[k] == v, (name, k)
    opt = make_optimizer(argparse.Namespace(optimizer="ranger", **dict(ns, use_gc=False, gc_conv_only=True, use_gcnorm=True)), m)
    assert (opt.use_gc, opt.gc_conv_only, opt.use_gcnorm) == (False, True, True)
    for name in ("ranger21", "novograd"):
        with pytest.raises(NotImplementedError):
            make_optimizer(argparse.Namespace(optimizer=name, **ns), m)
    with pytest.raises(NameError, match="Not Supported Optimizer"):
        make_optimizer(argparse.Namespace(optimizer="lion", **ns), m)
