"""-m "not gpu": the workspace sizes of the weight-gradient entry points against the Python mirror of the host rules
(tests/_conv_exact_ref.py), swept over layers and volumes on both sides of every rule: nlane 1 ... 8, the 512-workgroup
split rule with and without its cap, the all-taps blocks rule taken and refused, one and two sources, padded channel counts.
The size functions run without a device (the library then plans for 256 compute units); a launcher writes exactly the slabs
its plan counts, and the plan is what the size functions return, so a rule changed in one place and not the other fails here.

The split-precision sizes are asserted against the layout [3 groups of 16-bit slabs | hi, lo of every operand], every region
rounded up to 256 bytes, built from the 16-bit sizes of the same library."""
import contextlib

import pytest
import torch

import _conv_exact_ref as R
from brats21_amd import _lib

CHANNELS = [  # c1, c2, cout
    (8, 0, 48), (16, 0, 48), (8, 0, 64), (48, 0, 48),
    (48, 48, 48), (96, 0, 96), (96, 96, 48), (64, 0, 64),
    (32, 32, 128), (192, 0, 192), (384, 0, 384), (384, 384, 192),
    (24, 0, 40), (16, 48, 32), (48, 0, 8), (768, 0, 192),
]
VOLUMES = [  # n, d, h, w
    (1, 4, 4, 16), (2, 5, 6, 18), (2, 16, 16, 64), (1, 8, 8, 16),
    (1, 16, 16, 16), (2, 16, 16, 16), (2, 32, 32, 32), (2, 32, 64, 64),
    (2, 64, 64, 64), (2, 128, 128, 128), (1, 36, 52, 240), (3, 10, 32, 64),
]
DTYPES = [(_lib.BF16, True), (_lib.F32, False)]  # code, 16-bit operands


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


def _layers(bits16):
    """The f32 kernels take 16-byte pieces of 4 channels."""
    return [c for c in CHANNELS if bits16 or all(v % 4 == 0 for v in c)]


@contextlib.contextmanager
def _switch(setter, mode):
    old = setter(mode)
    try:
        yield
    finally:
        setter(old)


def _x3_align(b):
    return (b + 255) // 256 * 256


def _x3_layout(slab16, vox, channels):
    return _x3_align(3 * slab16) + 2 * sum(_x3_align(vox * c * 2) for c in channels if c > 0)


@pytest.mark.parametrize("mode", [0, 1])
def test_wgrad_ws_bytes_is_the_mirrored_plan(mode):
    l, ncu = _lib.lib(), _ncu()
    with _switch(l.brats_conv3d_set_wgrad_alltaps, mode):
        for code, bits16 in DTYPES:
            for c1, c2, cout in _layers(bits16):
                for n, d, h, w in VOLUMES:
                    want = max(R.wgrad_plan(bits16, dil, c1, c2, cout, n, d, h, w, mode, ncu)["ws_bytes"] for dil in (1, 2))
                    got = l.brats_conv3d_wgrad_ws_bytes(code, 3, n, d, h, w, c1, c2, cout)
                    assert got == want, (mode, code, c1, c2, cout, n, d, h, w, got, want)


def test_wgrad_shift_ws_bytes_is_the_mirrored_plan():
    l = _lib.lib()
    for code, bits16 in DTYPES:
        for k in (1, 3):
            for c1, c2, cout in _layers(bits16):
                cin = c1 + c2
                for n, d, h, w in VOLUMES:
                    want = R.wgrad_shift_plan(bits16, k, cin, cout, n, d, h, w)["ws_bytes"]
                    got = l.brats_conv3d_wgrad_shift_ws_bytes(code, k, n, d, h, w, cin, cout)
                    assert got == want, (code, k, cin, cout, n, d, h, w, got, want)
    assert l.brats_conv3d_wgrad_shift_ws_bytes(_lib.BF16, 2, 1, 8, 8, 16, 48, 48) == 0
    assert l.brats_conv3d_wgrad_ws_bytes(_lib.BF16, 1, 1, 8, 8, 16, 48, 0, 48) == 0


@pytest.mark.parametrize("x3", [_lib.X3_BF16, _lib.X3_F16])
def test_split_precision_ws_bytes_is_the_carve_up(x3):
    l = _lib.lib()
    b16 = _lib.BF16 if x3 == _lib.X3_BF16 else _lib.F16
    for c1, c2, cout in CHANNELS:
        for n, d, h, w in VOLUMES:
            vox = n * d * h * w
            for k in (1, 3):
                slab = l.brats_conv3d_wgrad_shift_ws_bytes(b16, k, n, d, h, w, c1 + c2, cout)
                got = l.brats_conv3d_wgrad_shift_ws_bytes(x3, k, n, d, h, w, c1 + c2, cout)
                assert got == _x3_layout(slab, vox, (c1 + c2, cout)), (k, c1 + c2, cout, n, d, h, w)
            with _switch(l.brats_conv3d_set_x3_wgrad_fused, 0):  # (the fused form's slabs have no mirror)
                for mode in (0, 1):
                    with _switch(l.brats_conv3d_set_wgrad_alltaps, mode):
                        slab = l.brats_conv3d_wgrad_ws_bytes(b16, 3, n, d, h, w, c1, c2, cout)
                        got = l.brats_conv3d_wgrad_ws_bytes(x3, 3, n, d, h, w, c1, c2, cout)
                        assert got == _x3_layout(slab, vox, (c1, c2, cout)), (mode, c1, c2, cout, n, d, h, w)
