"""-m "not gpu": the validation metrics of utils/metrics.py (Dice, Hausdorff distance 95, sensitivity, specificity): the C ABI
exports the Hausdorff entry points, the numpy restatement tests/_metrics_ref.py reproduces the reference's golden vectors
(tests/golden/metrics.npz, made by tests/golden/make_golden_metrics.py) bit for bit, and the drop-ins of
brats21_amd.metrics reject bad arguments before any device work."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _metrics_ref as ref
from brats21_amd import _lib, metrics

RAW = {"raw_p95": (95, False, True), "raw_max": (None, False, True), "raw_p95_directed": (95, True, True),
       "raw_max_directed_nobg": (None, True, False), "raw_p50_nobg": (50, False, False)}


def test_hausdorff_symbols_exported():
    l = ctypes.CDLL(_lib.LIB_PATH)
    for n in ("brats_hausdorff_ws_bytes", "brats_hausdorff"):
        assert n in _lib.declared_symbols()
        assert hasattr(l, n), f"{n} not exported"
    lib = _lib.lib()
    v = 160 * 240 * 240
    assert lib.brats_hausdorff_ws_bytes(3, 160, 240, 240) >= 3 * v * (1 + 2 * 2 * 4)
    assert lib.brats_hausdorff_ws_bytes(0, 4, 5, 6) == 0
    assert lib.brats_hausdorff_ws_bytes(1, 4, 5, 4096) == 0
    # argument errors are reported, never dereferenced
    assert lib.brats_hausdorff(None, None, 1, 4, 4, 4, 95.0, 0, None, None, None) == -1
    assert b"hausdorff" in lib.brats_last_error()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.brats_hausdorff(p, p, 1, 4, 4, 4, 100.5, 0, p, p, None) == -1
    assert lib.brats_hausdorff(p, p, 1, 4, 4, 4, float("nan"), 0, p, p, None) == -1
    assert lib.brats_hausdorff(p, p, 1, 4, 4, 4096, 95.0, 0, p, p, None) == -2


def test_reference_restatement_matches_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "metrics.npz"))
    assert len(g["cases"]) >= 10
    for name in g["cases"]:
        p, t = ref.load_case(g, name)
        res, cm = ref.metrics(p, t)
        assert list(res) == ["Dice", "Hausdorff_Distance95", "Sensitivity", "Specificity"]
        for k, v in res.items():
            w = g[f"{name}__{k}"]
            assert v.dtype == w.dtype == np.float32 and v.shape == w.shape, (name, k)
            np.testing.assert_array_equal(v, w, err_msg=f"{name} {k}")
        w = g[f"{name}__confusion"]
        assert cm.dtype == w.dtype and cm.shape == w.shape
        np.testing.assert_array_equal(cm, w, err_msg=f"{name} confusion")
        for k, (pct, directed, bg) in RAW.items():
            np.testing.assert_array_equal(ref.hausdorff(p, t, pct, directed, bg), g[f"{name}__{k}"], err_msg=f"{name} {k}")


def test_golden_covers_the_degenerate_cases(golden_dir):
    g = np.load(os.path.join(golden_dir, "metrics.npz"))
    assert np.isnan(g["voxels__Hausdorff_Distance95"][0, 1])        # union of one voxel: no edges, NaN kept
    assert g["empty__Hausdorff_Distance95"][0, 0] == ref.WORST_HAUSDORFF
    assert np.isnan(g["empty__raw_p95"][0, 0]) and np.isinf(g["empty__raw_max"][0, 0])
    assert g["empty__Dice"][0, 2] == 1 and g["empty__Hausdorff_Distance95"][0, 2] == 0


def test_slab_keeps_only_its_rim():
    m = np.zeros((5, 6, 7), np.float32)
    m[2, 1:5, 1:6] = 1
    e, _ = ref.edges(m, m)
    assert e.sum() == 4 * 5 - 2 * 3 and not e[2, 2:4, 2:5].any()
    one = np.zeros((5, 6, 7), np.float32)
    one[1, 2, 3] = 1
    assert not ref.edges(one, one)[0].any()


def test_drop_in_argument_errors():
    with pytest.raises(NotImplementedError, match="roc_auc"):
        metrics.get_metric_callable(["dice", "roc_auc"])
    with pytest.raises(NotImplementedError, match="surface_distance"):
        metrics.get_metric_callable(["surface_distance"])
    with pytest.raises(NotImplementedError, match="not implemented"):
        metrics.get_metric_callable(["jaccard"])
    with pytest.raises(NotImplementedError, match="precision"):
        metrics.get_metric_callable(["precision"])
    with pytest.raises(TypeError):
        metrics.get_metric_callable("dice")
    d = metrics.get_metric_callable(["dice", "hausdorff_distance95", "sensitivity", "specificity"])
    assert [v for v in d.values()] == [["Dice"], ["Hausdorff_Distance95"], ["Sensitivity", "Specificity"]]
    x = torch.zeros(1, 3, 4, 4, 4)
    with pytest.raises(ValueError):
        metrics.compute_metric_tensor(x, torch.zeros(1, 3, 4, 4, 5), d)
    with pytest.raises(ValueError):
        metrics.compute_metric_tensor(x[0], x[0], d)
    # CPU tensors: the GPU-only entry points refuse them, as evaluate's do
    with pytest.raises(_lib.BratsHipError):
        metrics.hausdorff_distance(x, x)
    with pytest.raises(_lib.BratsHipError):
        metrics.brats_metrics(x, x)
    with pytest.raises(ValueError):
        metrics.brats_metrics(x, x, ("dice", "hd"))
    assert metrics.set_labels([2, 0, 1]) == {"0": 0, "1": 1, "2": 2}
    assert list(metrics.set_labels({"b": 2, "a": 1})) == ["a", "b"]
    assert metrics.WORST_HAUSDORFF == float(ref.WORST_HAUSDORFF)
