"""The (inplanes, num_classes) cases of tests/golden/make_golden_general.py and the two test files that read its fixtures
(test_general_channels_cpu.py, test_general_channels_gpu.py): what a case is, its closed-form inputs, and how its network is
built -- stated once, so that the generator and the tests cannot drift apart."""
import argparse
import contextlib
import io
import warnings

import numpy as np
import torch

from oracle import synth, unet

SIZE = (16, 16, 16)
# (network, width, inplanes, num_classes): one-channel CT with five labels, two modalities with the most classes the head kernels
# take, more modalities than one 16-byte channel vector holds; the same two ends for the EvoNorm network
CASES = [("equiunet", 8, 1, 5), ("equiunet", 8, 2, 16), ("equiunet", 8, 9, 7), ("assp", 16, 1, 5), ("assp", 16, 3, 16)]
IDS = [f"{net}_c{c}_k{k}" for net, _, c, k in CASES]
# BraTS' own shape at the same width and size: the yardstick of the 16-bit deviation test (the committed (4, 3) fixtures of
# this network are 32^3 and 64^3)
BRATS_CASE = ("equiunet", 8, 4, 3)


def fname(case):
    net, width, c, k = case
    return f"general_{net}_w{width}_c{c}_k{k}.npz"


def features(case):
    return [case[1] * m for m in (1, 2, 4, 8)]


def shapes(case):
    net, width, c, k = case
    fn = unet.equiunet_state_shapes if net == "equiunet" else unet.assp_evo_state_shapes
    return fn(width, inplanes=c, num_classes=k)


def oracle_forward(case):
    return unet.equiunet_forward if case[0] == "equiunet" else unet.assp_evo_forward


def image(case, n=1, size=SIZE):
    return synth.closed_form_image(n, case[2], size)


def nested_targets(n, k, size=SIZE):
    """[n, k, D, H, W] {0, 1} f32: k nested spheres of radii linspace(0.8, 0.2, k) around synth.nested_spheres' centre on the
    [-1, 1]^3 grid (synth.nested_spheres itself gives three channels only)."""
    d, h, w = size
    zz, yy, xx = np.meshgrid(np.linspace(-1, 1, d), np.linspace(-1, 1, h), np.linspace(-1, 1, w), indexing="ij")
    r2 = (zz - 0.1) ** 2 + (yy + 0.05) ** 2 + (xx - 0.15) ** 2
    t = np.stack([(r2 <= r * r).astype(np.float32) for r in np.linspace(0.8, 0.2, k)], 0)
    return torch.from_numpy(t)[None].repeat(n, 1, 1, 1, 1).contiguous()


def build(case, deep_supervision=True, load=True):
    """brats21_amd's network of the case (on the CPU, f32 precision mode), the closed-form weights loaded."""
    from brats21_amd.networks import EquiUnet
    from brats21_amd.networks.equiunet_assp import EquiUnetASSPEvo
    net, _, c, k = case
    cls = EquiUnet if net == "equiunet" else EquiUnetASSPEvo
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = cls(c, k, features(case), norm_layer="group", act="relu", deep_supervision=deep_supervision, dropout=0)
    if load:
        sd = synth.fill_state_dict(shapes(case))
        m.load_state_dict({k: sd[k] for k in m.state_dict()}, strict=True)  # (without deep supervision: no deep-head keys)
    m.precision = "fp32"
    return m


def namespace(model="equiunet", width=8, num_classes=3):
    return argparse.Namespace(model=model, width=width, norm="group", act="relu", num_classes=num_classes, dropout=0)
