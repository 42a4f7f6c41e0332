"""numpy oracle of the nearest-sample rows as include/ndnet_nearest.h defines
them, and of the baseline's point transform (a helper of test_nearest_cpu.py,
test_nearest_gpu.py and test_pointnet_baseline_gpu.py, not a conftest).

Per cloud, in float32, every operation rounded (numpy does not fuse separate
ufunc calls):

    for i < m:  best = +inf; row = -1
                for t in 0 .. ms:  d = (dx*dx + dy*dy) + dz*dz  with dx = p[i].x - s[t].x, ...
                                   if d < best: best = d; row = t      (false for NaN; ties keep the smaller t)
    rows[i] = -1 for m <= i < n  (dist there keeps what the caller put)
"""
import numpy as np


def nearest_ref(points, samples, count=None, sample_count=None, chunk=512):
    """``(rows int32 [n], dist float32 [n])`` of one cloud: ``points`` ``[n, 3]``
    and ``samples`` ``[S, 3]`` float32.  ``dist`` past ``count`` is NaN (the
    kernel writes nothing there).  Vectorised over chunks of points."""
    points, samples = np.asarray(points), np.asarray(samples)
    assert points.dtype == np.float32 and samples.dtype == np.float32
    n, S = len(points), len(samples)
    m = n if count is None else min(max(int(count), 0), n)
    ms = S if sample_count is None else min(max(int(sample_count), 0), S)
    rows = np.full(n, -1, np.int32)
    dist = np.full(n, np.nan, np.float32)
    dist[:m] = np.inf
    if ms == 0:
        return rows, dist
    s = samples[:ms]
    with np.errstate(invalid="ignore", over="ignore"):
        for i0 in range(0, m, chunk):
            p = points[i0:min(i0 + chunk, m)]
            dx = p[:, None, 0] - s[None, :, 0]
            dy = p[:, None, 1] - s[None, :, 1]
            dz = p[:, None, 2] - s[None, :, 2]
            d = (dx * dx + dy * dy) + dz * dz              # float32 [chunk, ms]
            assert d.dtype == np.float32
            # the first t whose d is below +inf and below every earlier one: NaN and +inf never win
            cand = np.where(d < np.float32(np.inf), d, np.float32(np.inf))
            t = np.argmin(cand, axis=1)                    # numpy: the first minimum
            best = cand[np.arange(len(p)), t]
            hit = best < np.float32(np.inf)
            rows[i0:i0 + len(p)] = np.where(hit, t, -1)
            dist[i0:i0 + len(p)] = best
    return rows, dist


def nearest_loops(points, samples, count=None, sample_count=None):
    """The same, as plain loops written from the definition (slow: small clouds)."""
    points, samples = np.asarray(points), np.asarray(samples)
    T = np.float32
    n, S = len(points), len(samples)
    m = n if count is None else min(max(int(count), 0), n)
    ms = S if sample_count is None else min(max(int(sample_count), 0), S)
    rows = np.full(n, -1, np.int32)
    dist = np.full(n, np.nan, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(m):
            best, row = T(np.inf), -1
            for t in range(ms):
                dx = T(points[i, 0] - samples[t, 0])
                dy = T(points[i, 1] - samples[t, 1])
                dz = T(points[i, 2] - samples[t, 2])
                d = T(T(T(dx * dx) + T(dy * dy)) + T(dz * dz))
                if d < best:
                    best, row = d, t
            rows[i], dist[i] = row, best
    return rows, dist


def lattice_case(side=8, n_samples=37, seed=0):
    """The side^3 integer lattice in a seeded order and ``n_samples`` of its
    points as samples, float32: every squared distance is a small integer and
    most points have several nearest samples."""
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    rng = np.random.default_rng(seed)
    g = g[rng.permutation(len(g))]
    return g, g[rng.choice(len(g), n_samples, replace=False)].copy()


def transform3_ref(points, t1):
    """``ndnet_pn_transform3_run`` of one cloud: ``points`` ``[n, >= 3]`` and
    ``t1`` ``[3, 3]`` float32 -> ``[n, 3]``; every operation rounded, then
    NaN -> 0, +inf -> FLT_MAX, -inf -> -FLT_MAX."""
    points, t1 = np.asarray(points), np.asarray(t1)
    assert points.dtype == np.float32 and t1.dtype == np.float32
    x, y, z = points[:, 0], points[:, 1], points[:, 2]
    fmax = np.finfo(np.float32).max
    out = np.empty((len(points), 3), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(3):
            v = (t1[a, 0] * x + t1[a, 1] * y) + t1[a, 2] * z
            assert v.dtype == np.float32
            v = np.where(np.isnan(v), np.float32(0), v)
            out[:, a] = np.clip(v, -fmax, fmax)
    return out
