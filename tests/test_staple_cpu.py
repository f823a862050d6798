"""No GPU: closed forms of the numpy restatement of ITK's STAPLE filter (tests/_staple_ref.py, the oracle of tests/test_staple_gpu.py),
the declaration and binding of the brats_staple_* entry points, and the argument checks of ops.staple / StaplePacker /
perform_staple_on_brats_multi_channel / Evaluator(perform_staple=) that run before any device work.

The iteration count is ITK's GetElapsedIterations(): the index of the iteration whose M-step no longer moved any p / q by more
than 1e-7, or max_iterations.  One rater, identical raters and the two degenerate channels (nobody marks it / everybody fills
it) all stop in the iteration of index 1 -- the loop body has then run twice."""
import numpy as np
import pytest
import torch

import _staple_ref as R

SHAPE = (13, 18, 21)


def test_one_rater_and_identical_raters_return_the_input_in_one_iteration():
    d = R.make_raters(SHAPE, 1, 11)
    for raters in (d, np.repeat(d, 4, axis=0)):
        w, p, q, it, g = R.staple(raters)
        assert it == 1
        np.testing.assert_array_equal(R.fused_mask(w), d[0].astype(bool))
        np.testing.assert_array_equal(p, 1.0)
        np.testing.assert_array_equal(q, 1.0)
        assert g == d[0].sum() / d[0].size


@pytest.mark.parametrize("value", [0, 1])
def test_a_channel_nobody_marks_or_everybody_fills_gives_nan_weights_and_an_empty_mask(value):
    w, p, q, it, g = R.staple(np.full((5,) + SHAPE, value, dtype=np.uint8))
    assert np.isnan(w).all() and not R.fused_mask(w, 0.5).any() and not R.fused_mask(w, 0.0).any()
    assert it == 1 and g == float(value)  # (two passes of the loop body: iterations 0 and 1)


def test_one_empty_rater_among_five():
    d = R.make_raters(SHAPE, 5, 12)
    d[2] = 0
    w, p, q, it, g = R.staple(d)
    assert p[2] == 0.0 and q[2] == 1.0
    assert np.isfinite(w).all() and np.isfinite(p).all() and np.isfinite(q).all()
    assert 0 < R.fused_mask(w).sum() < w.size


def test_max_iterations_is_a_cap():
    d = R.make_raters(SHAPE, 5, 13)
    free = R.staple(d)[3]
    assert free > 3
    assert R.staple(d, max_iterations=3)[3] == 3 and R.staple(d, max_iterations=1)[3] == 1
    assert R.staple(d, max_iterations=free + 5)[3] == free


def test_weights_depend_on_the_decision_pattern_only():
    d = R.make_raters(SHAPE, 5, 14)
    w = R.staple(d)[0].ravel()
    code = (d.reshape(5, -1).astype(np.int64) << np.arange(5)[:, None]).sum(0)
    for c in np.unique(code):
        assert np.unique(w[code == c]).size == 1


@pytest.mark.parametrize("raters", [5, 32, 33, 64, 65, 70])
def test_the_synthetic_raters_cannot_be_fused_by_a_vote(raters):
    """What the GPU parity test relies on: on its inputs (channel 0 here) STAPLE's mask is not the majority vote."""
    d = R.make_raters(SHAPE, raters, 100 + raters)
    w = R.staple(d)[0]
    vote = 2 * d.sum(0, dtype=np.int64) > raters
    assert (R.fused_mask(w) != vote).any()


# ---- header and binding -----------------------------------------------------------------------------------------------
NAMES = ["brats_staple_blocks", "brats_staple_pack", "brats_staple_init", "brats_staple_iterate", "brats_staple_apply"]


def test_entry_points_are_declared_bound_and_the_abi_number_matches_the_header():
    from brats21_amd import _lib
    assert set(NAMES) <= set(_lib.declared_symbols())
    lib = _lib.lib()
    assert lib.brats_abi_version() == _lib._header_abi_version()
    for n in NAMES:
        assert getattr(lib, n).argtypes is not None
    assert len(lib.brats_staple_iterate.argtypes) == 12 and len(lib.brats_staple_apply.argtypes) == 10
    # the workspace query needs no device: one row of partial sums per workgroup, 512 at most, 0 beyond the supported size
    assert lib.brats_staple_blocks(13 * 18 * 21) == 20 and lib.brats_staple_blocks(40 * 48 * 56) == 420
    assert 1 <= lib.brats_staple_blocks(240 * 240 * 160) <= 512
    assert lib.brats_staple_blocks(2 ** 31) == 0 and lib.brats_staple_blocks(0) == 0


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """R = 0, R > 256 and V >= 2^31 are BRATS_E_UNSUPPORTED with a message; the checks come before the first launch."""
    import ctypes
    from brats21_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_double * 16)()
    ptr = ctypes.addressof(buf)
    for r, v in ((0, 100), (257, 100), (4, 2 ** 31)):
        assert lib.brats_staple_init(ptr, ptr, 256, ptr, ptr, 1, r, v, None) == -2
        assert lib.brats_staple_iterate(ptr, ptr, 256, ptr, ptr, ptr, 1, r, v, 10, 1, None) == -2
        assert lib.brats_staple_apply(ptr, ptr, 1, r, v, 0.5, ptr, 0, None, None) == -2
        assert b"supported" in lib.brats_last_error()
    assert lib.brats_staple_apply(ptr, ptr, 1, 4, 100, 1.5, ptr, 0, None, None) == -1
    assert lib.brats_staple_iterate(ptr, ptr, 256, ptr, ptr, ptr, 1, 4, 100, 0, 1, None) == -1
    assert lib.brats_staple_pack(ptr, 0, ptr, ptr, 4, 1, 1, 100, 40, None) == -1   # rater outside the words
    assert lib.brats_staple_pack(ptr, 0, ptr, ptr, 300, 1, 9, 100, 0, None) == -2  # more than 256 raters


# ---- Python layer -----------------------------------------------------------------------------------------------------
def _maps(n, shape=(1, 3, 4, 5, 6)):
    return [torch.zeros(shape) for _ in range(n)]


def test_ops_staple_checks_its_arguments_and_refuses_cpu_tensors():
    from brats21_amd import ops
    from brats21_amd._lib import BratsHipError
    with pytest.raises(BratsHipError, match="GPU only"):
        ops.staple(_maps(3))
    for bad in (-0.1, 1.5, float("nan"), "0.5", None):
        with pytest.raises(ValueError, match="threshold"):
            ops.staple(_maps(3), threshold=bad)
    with pytest.raises(ValueError, match="0 raters"):
        ops.staple([])
    with pytest.raises(ValueError, match="257 raters"):
        ops.staple(_maps(257, (1, 1, 2, 2, 2)))
    with pytest.raises(ValueError, match="different shapes"):
        ops.staple(_maps(2) + _maps(1, (1, 3, 4, 5, 7)))
    with pytest.raises(ValueError, match=r"\[N, C, D, H, W\]"):
        ops.staple(_maps(2, (3, 4, 5, 6)))
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError, match="max_iterations"):
            ops.staple(_maps(3), max_iterations=bad)
    with pytest.raises(ValueError, match="chunk"):
        ops.staple(_maps(3), chunk=0)


def test_staple_packer_checks_its_arguments_and_refuses_cpu_tensors():
    from brats21_amd import ops
    from brats21_amd._lib import BratsHipError
    with pytest.raises(BratsHipError, match="GPU only"):
        ops.StaplePacker((1, 3, 4, 5, 6), 4, "cpu")
    for bad in (0, 257, 2.0):
        with pytest.raises(ValueError, match="max_raters"):
            ops.StaplePacker((1, 3, 4, 5, 6), bad)
    with pytest.raises(ValueError, match=r"\[N, C, D, H, W\]"):
        ops.StaplePacker((3, 4, 5, 6), 4)
    with pytest.raises(ValueError, match="2\\^31"):
        ops.StaplePacker((1, 1, 2048, 1024, 1024), 4)
    pk = ops.StaplePacker((1, 3, 4, 5, 6), 4)  # (nothing is allocated before the first add)
    with pytest.raises(BratsHipError, match="GPU only"):
        pk.add(torch.zeros(1, 3, 4, 5, 6))
    with pytest.raises(ValueError, match="shape"):
        pk.add(torch.zeros(1, 3, 4, 5, 7))
    with pytest.raises(ValueError, match="no rater"):
        ops.staple(pk)
    assert pk.raters == 0 and pk.bits is None


def test_perform_staple_on_brats_multi_channel_checks_its_arguments():
    from brats21_amd.evaluate import perform_staple_on_brats_multi_channel as fuse
    from brats21_amd._lib import BratsHipError
    for bad in (-0.5, 1.01):
        with pytest.raises(ValueError, match="threshold_value"):
            fuse(_maps(3), threshold_value=bad)
    with pytest.raises(ValueError, match="0 raters"):
        fuse([])
    with pytest.raises(ValueError, match="257 raters"):
        fuse(_maps(257, (1, 1, 2, 2, 2)))
    with pytest.raises(ValueError, match="one shape"):
        fuse(_maps(2) + _maps(1, (1, 3, 4, 5, 7)))
    with pytest.raises(ValueError, match="one shape"):
        fuse(_maps(2, (3, 4, 5, 6)))
    if not torch.cuda.is_available():  # CPU inputs are copied to the GPU and back: without one there is nothing to run on
        with pytest.raises(BratsHipError, match="GPU only"):
            fuse(_maps(3))


def test_evaluator_checks_the_staple_arguments():
    from brats21_amd import tta
    from brats21_amd.evaluate import Evaluator
    model = torch.nn.Identity()
    for bad in (-0.1, 1.1, "half", None):
        with pytest.raises(ValueError, match="staple_threshold"):
            Evaluator(model, staple_threshold=bad, use_graph=False)
    with pytest.raises(ValueError, match="272 raters"):
        Evaluator([model] * 17, tta_transforms=tta.get_tta_transforms(), perform_staple=True, use_graph=False)
    ev = Evaluator([model] * 16, tta_transforms=tta.get_tta_transforms(), perform_staple=True, staple_threshold=0.3, use_graph=False)
    assert ev.perform_staple and ev.raters == 256 and ev.staple_threshold == 0.3
    assert not Evaluator(model, use_graph=False).perform_staple
