"""-m gpu: the validation metrics of utils/metrics.py on the GPU (brats21_amd/metrics.py, csrc/metrics.hip) against the
reference's golden vectors (tests/golden/metrics.npz), the numpy restatement tests/_metrics_ref.py on seeded small
volumes, and an independent brute-force torch check on BraTS-sized volumes."""
import argparse
import importlib.util
import os

import numpy as np
import pytest
import torch

import _metrics_ref as ref
from brats21_amd import _lib, metrics
from oracle import synth, unet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW = {"raw_p95": (95, False, True), "raw_max": (None, False, True), "raw_p95_directed": (95, True, True),
       "raw_max_directed_nobg": (None, True, False), "raw_p50_nobg": (50, False, False)}


def _timer():
    spec = importlib.util.spec_from_file_location("time_metrics", os.path.join(ROOT, "scripts", "time_metrics.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _hd_close(got, want, what=""):
    """within 1 float32 ulp, NaN / inf exactly where the expected value has them"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN pattern {got} vs {want}"
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin & ~nan], want[~fin & ~nan]), what
    ulp = np.spacing(np.abs(want[fin]))
    assert np.all(np.abs(got[fin] - want[fin]) <= ulp), f"{what}: {got} vs {want}"


def test_goldens_through_compute_metric_tensor(golden_dir):
    g = np.load(os.path.join(golden_dir, "metrics.npz"))
    fns = metrics.get_metric_callable(["dice", "hausdorff_distance95", "sensitivity", "specificity"])
    for name in g["cases"]:
        p, t = ref.load_case(g, name)
        res, cm = metrics.compute_metric_tensor(torch.from_numpy(p), torch.from_numpy(t), fns)  # CPU in, numpy out
        assert sorted(res) == sorted(["Dice", "Hausdorff_Distance95", "Sensitivity", "Specificity"])
        for k, v in res.items():
            w = g[f"{name}__{k}"]
            assert isinstance(v, np.ndarray) and v.dtype == w.dtype and v.shape == w.shape, (name, k)
            if k == "Hausdorff_Distance95":
                _hd_close(v, w, f"{name} {k}")
            else:
                np.testing.assert_array_equal(v, w, err_msg=f"{name} {k}")
        w = g[f"{name}__confusion"]
        assert cm.dtype == w.dtype and cm.shape == w.shape
        np.testing.assert_array_equal(cm, w, err_msg=name)
        pd, td = torch.from_numpy(p).to(DEV), torch.from_numpy(t).to(DEV)
        for k, (pct, directed, bg) in RAW.items():
            got = metrics.hausdorff_distance(pd, td, pct, directed, bg)
            assert got.dtype == torch.float32 and got.is_cuda
            _hd_close(got.cpu().numpy(), g[f"{name}__{k}"].astype(np.float32), f"{name} {k}")


def _random_pair(rng, shape, n=1):
    def vol():
        kind = rng.integers(4)
        if kind == 0:
            return rng.random(shape) < rng.uniform(0.005, 0.3)
        z, y, x = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
        m = np.zeros(shape, bool)
        for _ in range(rng.integers(1, 4)):
            c = [rng.uniform(0, s) for s in shape]
            m |= ((z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2) <= rng.uniform(1, 6) ** 2
        if kind == 2:
            m[:, :, rng.integers(shape[2])] = False
        if kind == 3:
            m &= rng.random(shape) < 0.8
        return m
    p = np.stack([np.stack([vol() for _ in range(3)]) for _ in range(n)]).astype(np.float32)
    t = np.stack([np.stack([vol() for _ in range(3)]) for _ in range(n)]).astype(np.float32)
    return p, t


@pytest.mark.parametrize("seed", range(4))
def test_random_small_volumes_vs_restatement(seed):
    rng = np.random.default_rng(1000 + seed)
    shape = tuple(int(s) for s in rng.integers(1, 23, 3)) if seed else (12, 17, 21)
    p, t = _random_pair(rng, shape, n=2)
    pd, td = torch.from_numpy(p).to(DEV), torch.from_numpy(t).to(DEV)
    for pct in (95, None, 50, 100):
        for directed in (False, True):
            got = metrics.hausdorff_distance(pd, td, pct, directed).cpu().numpy()
            _hd_close(got, ref.hausdorff(p, t, pct, directed).astype(np.float32), f"{shape} {pct} {directed}")
    res = metrics.brats_metrics(pd, td)
    want, _ = ref.metrics(p, t)
    for k, name in zip(metrics.METRICS, want):
        if k == "hausdorff_distance95":
            _hd_close(res[k].cpu().numpy(), want[name], k)
        else:
            np.testing.assert_array_equal(res[k].cpu().numpy(), want[name], err_msg=k)


# ---- full size: an independent brute-force check in torch -------------------------------------------------------------
def _edges_torch(m, thick):
    """fg ^ erosion(fg) by slicing, 6-neighbour cross, outside = 0, only along the axes in `thick`"""
    fg = m == 1
    pad = torch.nn.functional.pad(fg[None, None].float(), (1, 1, 1, 1, 1, 1))[0, 0] > 0
    inner = fg.clone()
    D, H, W = fg.shape
    for ax in range(3):
        if not thick[ax]:
            continue
        for s in (0, 2):
            sl = [slice(1, D + 1), slice(1, H + 1), slice(1, W + 1)]
            sl[ax] = slice(s, s + fg.shape[ax])
            inner &= pad[tuple(sl)]
    return fg & ~inner


def _sqdist_torch(a, b):
    """exact int64 squared distance of every point of a to the nearest point of b (chunked brute force)"""
    out = torch.empty(len(a), dtype=torch.int64, device=a.device)
    for i in range(0, len(a), 1024):
        d = ((a[i:i + 1024, None, :] - b[None, :, :]) ** 2).sum(-1)
        out[i:i + 1024] = d.min(1).values
    return out


def _hd95_torch(pred, target):
    out = np.empty(pred.shape[:2])
    for n, k in np.ndindex(*pred.shape[:2]):
        p, t = pred[n, k], target[n, k]
        idx = torch.nonzero((p == 1) | (t == 1))
        thick = [bool(v) for v in (idx.max(0).values > idx.min(0).values)]
        ep, et = torch.nonzero(_edges_torch(p, thick)), torch.nonzero(_edges_torch(t, thick))
        assert 0 < len(ep) <= 20000 and 0 < len(et) <= 20000, (len(ep), len(et))
        d1 = np.sqrt(_sqdist_torch(ep, et).cpu().numpy().astype(np.float64))
        d2 = np.sqrt(_sqdist_torch(et, ep).cpu().numpy().astype(np.float64))
        out[n, k] = max(np.percentile(d1, 95), np.percentile(d2, 95))
    return out


def _box_case():
    D, H, W = 160, 240, 240
    p, t = torch.zeros(1, 3, D, H, W), torch.zeros(1, 3, D, H, W)
    p[0, 0, 159, 10:200, 100:240] = 1          # slabs one voxel thick along D, at the far face: a 2-D crop
    t[0, 0, 159, 40:120, 150:239] = 1
    p[0, 1, :, 0, 0] = 1                       # a line along D in a corner vs a scattered few voxels on it
    t[0, 1, 3, 0, 0] = t[0, 1, 100, 0, 0] = t[0, 1, 157, 0, 0] = 1
    p[0, 2, 0:100, 0:50, 0:4] = 1              # a box against three faces of the volume
    t[0, 2, 20:60, 30:80, 2:30] = 1
    return p, t


@pytest.mark.parametrize("kind", ["a", "b", "box"])
def test_full_size_vs_brute_force(kind):
    p, t = _box_case() if kind == "box" else _timer().case(kind)
    pd, td = p.to(DEV), t.to(DEV)
    got = metrics.hausdorff_distance(pd, td, 95).cpu().numpy()
    want = _hd95_torch(pd, td)
    assert np.all(np.abs(got - want) <= 1e-4), (got, want)
    if kind == "b":  # the speckle spans the volume: the union's box is the whole volume
        assert bool((p[:, :, 0, 0, 0] == 1).all()) and bool((p[:, :, -1, -1, -1] == 1).all())


def test_batch_equals_single_calls():
    rng = np.random.default_rng(7)
    p, t = _random_pair(rng, (20, 24, 16), n=2)
    pd, td = torch.from_numpy(p).to(DEV), torch.from_numpy(t).to(DEV)
    both = metrics.brats_metrics(pd, td)
    for i in range(2):
        one = metrics.brats_metrics(pd[i:i + 1], td[i:i + 1])
        for k in metrics.METRICS:
            assert torch.equal(both[k][i:i + 1], one[k]) or torch.equal(both[k][i:i + 1].isnan(), one[k].isnan()), k
    for pct in (95, None):
        both = metrics.hausdorff_distance(pd, td, pct)
        one = torch.cat([metrics.hausdorff_distance(pd[i:i + 1], td[i:i + 1], pct) for i in range(2)])
        assert np.array_equal(both.cpu().numpy(), one.cpu().numpy(), equal_nan=True)


def test_graph_capture_replays_new_data():
    rng = np.random.default_rng(11)
    p0, t0 = _random_pair(rng, (24, 20, 22), n=1)
    p1, t1 = _random_pair(rng, (24, 20, 22), n=1)
    sp, st = torch.from_numpy(p0).to(DEV), torch.from_numpy(t0).to(DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            metrics.brats_metrics(sp, st)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = metrics.brats_metrics(sp, st)
    sp.copy_(torch.from_numpy(p1))
    st.copy_(torch.from_numpy(t1))
    g.replay()
    torch.cuda.synchronize()
    eager = metrics.brats_metrics(torch.from_numpy(p1).to(DEV), torch.from_numpy(t1).to(DEV))
    for k in metrics.METRICS:
        assert np.array_equal(out[k].cpu().numpy(), eager[k].cpu().numpy(), equal_nan=True), k


def _evaluator_case(**kw):
    from brats21_amd import get_model
    from brats21_amd.evaluate import Evaluator
    sd = synth.fill_state_dict(unet.equiunet_state_shapes(8))
    m = get_model(argparse.Namespace(model="equiunet", width=8, norm="group", act="relu", num_classes=3, dropout=0))
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    x = synth.closed_form_image(1, 4, (21, 18, 22), "evalcase")
    x = x * (synth.closed_form("evalmask", (1, 1, 21, 18, 22)) > -0.3)
    tgt = synth.nested_spheres(1, (21, 18, 22))
    ev = Evaluator(m, sliding_window_size=(16, 16, 16), overlap=0.5, amp=False, **kw)
    return ev, x.to(DEV), tgt.to(DEV)


def test_evaluator_default_and_with_metrics():
    from brats21_amd.evaluate import shape_to_divisible
    ev, x, tgt = _evaluator_case()
    base = ev(x, tgt)
    assert sorted(base) == ["dice", "seg"]
    again = ev(x, tgt)
    assert torch.equal(base["dice"], again["dice"]) and torch.equal(base["seg"], again["seg"])
    ev2, _, _ = _evaluator_case(metrics=("dice", "hausdorff_distance95", "sensitivity", "specificity"))
    res = ev2(x, tgt, return_original_shape=False)
    assert sorted(res) == ["dice", "hausdorff_distance95", "seg", "sensitivity", "specificity"]
    assert torch.equal(res["dice"], base["dice"])
    want = metrics.brats_metrics(res["seg"], shape_to_divisible(tgt, k=8)[0])
    for k in metrics.METRICS:
        assert res[k].shape == (1, 3) and res[k].is_cuda
        assert np.array_equal(res[k].cpu().numpy(), want[k].cpu().numpy(), equal_nan=True), k


def test_errors():
    from brats21_amd.evaluate import Evaluator
    x = torch.zeros(1, 3, 8, 8, 8, device=DEV)
    with pytest.raises(_lib.BratsHipError):
        metrics.hausdorff_distance(x.cpu(), x)
    with pytest.raises(_lib.BratsHipError):
        metrics.brats_metrics(x, x.cpu())
    with pytest.raises(ValueError):
        metrics.hausdorff_distance(x, torch.zeros(1, 3, 8, 8, 9, device=DEV))
    with pytest.raises(ValueError):
        metrics.hausdorff_distance(x, x, percentile=101)
    with pytest.raises(ValueError):
        metrics.brats_metrics(x, x, ("dice", "hd99"))
    with pytest.raises(ValueError):
        Evaluator(torch.nn.Identity(), metrics=("dice", "jaccard"))
    with pytest.raises(ValueError):
        metrics.confusion_matrix(x, x[:, :2])
