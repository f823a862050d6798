"""numpy float64 restatement of ITK's STAPLEImageFilter::GenerateData (Warfield et al.), one binary problem, as written down in
DESIGN.md section 6 -- the oracle of tests/test_staple_cpu.py / tests/test_staple_gpu.py and of scripts/time_staple.py.  SimpleITK is
not available to the tests, so this file is a RESTATEMENT of the filter, not a recording of it: nothing executable pins that boundary.

Also the synthetic raters the tests share (``make_raters``)."""
import numpy as np

CONVERGENCE = 1e-14


def staple(decisions, max_iterations=10000):
    """decisions: [R, ...] array of 0 / 1 -> (W float64 in the voxel shape, p [R], q [R], iterations, g).
    iterations is ITK's GetElapsedIterations(): the index of the iteration that converged, or max_iterations."""
    d = np.asarray(decisions).astype(bool)
    r = d.shape[0]
    shape = d.shape[1:]
    d = d.reshape(r, -1)
    v = d.shape[1]
    votes = d.sum(axis=0, dtype=np.int64)
    w = votes.astype(np.float64) / np.float64(r)
    g = np.float64(int(votes.sum())) / np.float64(r * v)  # the exact sum of W's numerators: one rounding
    last_p = np.full(r, -10.0)
    last_q = np.full(r, -10.0)
    p = np.zeros(r)
    q = np.zeros(r)
    iterations = max_iterations
    with np.errstate(all="ignore"):
        for it in range(max_iterations):
            # M-step (ITK adds W where the rater says foreground, 1 - W where it says background)
            one_w = 1.0 - w
            sum_w = w.sum()
            sum_1w = one_w.sum()
            for j in range(r):
                p[j] = np.sum(w, where=d[j]) / sum_w
                q[j] = np.sum(one_w, where=~d[j]) / sum_1w
            # E-step: plain products in rater order
            a = np.ones(v)
            b = np.ones(v)
            for j in range(r):
                a *= np.where(d[j], p[j], 1.0 - p[j])
                b *= np.where(d[j], 1.0 - q[j], q[j])
            w = g * a / (g * a + (1.0 - g) * b)
            moved = False
            for j in range(r):
                if (p[j] - last_p[j]) ** 2 > CONVERGENCE or (q[j] - last_q[j]) ** 2 > CONVERGENCE:  # (a NaN compares false)
                    moved = True
                    break
            last_p[:] = p
            last_q[:] = q
            if not moved:
                iterations = it
                break
    return w.reshape(shape), p.copy(), q.copy(), iterations, float(g)


def fused_mask(w, threshold=0.5):
    with np.errstate(invalid="ignore"):
        return w > threshold  # a NaN is background


def make_raters(shape, raters, seed):
    """[R, *shape] uint8: per rater a sphere of radius 0.3 min(shape), centre jittered by N(0, 1 voxel), radius scaled by
    1 + N(0, 0.1), every voxel flipped with probability 0.01."""
    rng = np.random.default_rng(seed)
    grid = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij")
    centre = [(s - 1) / 2.0 for s in shape]
    out = np.empty((raters,) + tuple(shape), dtype=np.uint8)
    for j in range(raters):
        c = [centre[a] + rng.normal(0.0, 1.0) for a in range(3)]
        rad = 0.3 * min(shape) * (1.0 + rng.normal(0.0, 0.1))
        m = sum((grid[a] - c[a]) ** 2 for a in range(3)) <= rad * rad
        out[j] = m ^ (rng.random(shape) < 0.01)
    return out
