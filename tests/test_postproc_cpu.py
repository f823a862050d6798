"""-m "not gpu": the label post-processing of get_post_transforms (--cleaning_areas / --replace_value): the C ABI exports
its entry points (ABI 7), the CPU restatement tests/_postproc_ref.py reproduces the reference's golden vectors
(tests/golden/postproc.npz, made by tests/golden/make_golden_postproc.py), and the Python classes reject bad arguments."""
import argparse
import ctypes
import os

import numpy as np
import pytest
import torch

import _postproc_ref as ref
from brats21_amd import _lib

NEW_SYMBOLS = ("brats_cc_ws_bytes", "brats_cc_filter", "brats_rare_fill_ws_bytes", "brats_rare_fill")


def test_postproc_symbols_exported_and_abi_7():
    l = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert n in _lib.declared_symbols()
        assert hasattr(l, n), f"{n} not exported"
    lib = _lib.lib()
    assert lib.brats_abi_version() == 7
    assert lib.brats_cc_ws_bytes(2, 160, 240, 240) >= 2 * 160 * 240 * 240 * 8
    assert lib.brats_rare_fill_ws_bytes(1, 4, 5, 6) >= 256 * 4 + 4 * 5 * 6 * 2
    assert lib.brats_cc_ws_bytes(0, 4, 5, 6) == 0
    # argument errors are reported, never dereferenced
    assert lib.brats_cc_filter(None, 1, 4, 4, 4, 0, None, None) == -1 and b"cc_filter" in lib.brats_last_error()
    assert lib.brats_rare_fill(None, 1, 4, 4, 4, 3, 0, None, None) == -1 and b"rare_fill" in lib.brats_last_error()
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.brats_cc_filter(p, 1, 4, 4, 4, -2, p, None) == -1
    assert lib.brats_rare_fill(p, 1, 4, 4, 4, -1, 0, p, None) == -1
    assert lib.brats_rare_fill(p, 1, 40000, 1, 1, 0, 0, p, None) == -2


def test_reference_restatement_matches_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "postproc.npz"))
    for name in ("clean_a", "clean_tie"):
        for t in (None, 0, 1, 10, 20):
            np.testing.assert_array_equal(ref.clean(g[name], t), g[f"{name}_t{'none' if t is None else t}"], err_msg=f"{name} {t}")
    for axis in (0, 1, 2):
        for kind in ("one", "two", "zero", "none", "allr"):
            tag = f"rare_{kind}_ax{axis}"
            out, ties = ref.replace(g[tag], int(g[tag + "_t"]), axis)
            np.testing.assert_array_equal(ties, g[tag + "_ties"], err_msg=tag)
            moved = ties != 0
            np.testing.assert_array_equal(out[~moved], g[tag + "_out"][~moved], err_msg=tag)
            assert np.all((ties[moved] >> out[moved]) & 1), tag
    prob = g["chain_prob"].astype(np.float32)
    for c in (0, 1):
        for r in (0, 1):
            tag = f"chain_c{c}r{r}"
            seg, ties = ref.chain(prob, 0.5, 20, bool(c), 300, bool(r))
            seg = ref.remove_background(g["chain_img"], seg)
            np.testing.assert_array_equal(ties[0], g[tag + "_ties"], err_msg=tag)
            if not ties.any():
                np.testing.assert_array_equal(seg, g[tag], err_msg=tag)
            else:
                same = (seg == g[tag]).all(1)[0]
                assert np.all(same | (ties[0] != 0)), tag


def test_constructor_argument_errors():
    from brats21_amd.evaluate import Evaluator, KeepLargestConnectedComponent, ReplaceWithClosestValue, get_post_transforms
    for bad in ("20", 2.5, True):
        with pytest.raises(TypeError):
            KeepLargestConnectedComponent(bad)
        with pytest.raises(TypeError):
            ReplaceWithClosestValue([3], thresh=bad)
    for axis in (3, -1, 1.0, "2", None):
        with pytest.raises(ValueError):
            ReplaceWithClosestValue([3], thresh=20, axis=axis)
    assert KeepLargestConnectedComponent().threshold is None and KeepLargestConnectedComponent(20).threshold == 20
    r = ReplaceWithClosestValue(labels=[3], thresh=300)
    assert (r.labels, r.thresh, r.axis) == ([3], 300, 2)
    with pytest.raises(TypeError):
        get_post_transforms(argparse.Namespace(cleaning_areas=True, cleaning_areas_threshold=2.5))
    with pytest.raises(TypeError):
        get_post_transforms(argparse.Namespace(replace_value=True, replace_value_threshold="300"))
    with pytest.raises(TypeError):
        Evaluator(torch.nn.Identity(), cleaning_areas_threshold=1.5, use_graph=False)
    with pytest.raises(ValueError):
        KeepLargestConnectedComponent(20)(torch.zeros(2, 3, 4, 5))
