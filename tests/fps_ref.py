"""numpy oracle of farthest point sampling as include/ndnet_fps.h defines it
(a helper of test_fps_cpu.py, test_fps_gpu.py and the test_fps_cases files,
not a conftest).

Per cloud, in the points' own dtype, every operation rounded (numpy does not
fuse separate ufunc calls):

    mind[0..m) = +inf
    for t in 0 .. min(n_samples, m):
        indices[t] = cur;  mind[cur] = -1
        d = (dx*dx + dy*dy) + dz*dz  with dx = p[j].x - p[cur].x, ...
        mind = where(d < mind, d, mind)            (false for NaN)
        cur = argmax(mind)                         (numpy: the first maximum)
    indices[t] = -1 for t >= m
"""
import numpy as np


def fps_ref(points, n_samples, count=None, start=0):
    """``(indices int32 [n_samples], mind [m])`` of one cloud ``points``
    ``[n, 3]`` (float32 or float64); only its first ``count`` points exist."""
    points = np.asarray(points)
    assert points.ndim == 2 and points.shape[1] == 3 and points.dtype in (np.float32, np.float64)
    dt = points.dtype
    m = len(points) if count is None else int(count)
    assert 1 <= m <= len(points)
    x, y, z = (np.ascontiguousarray(points[:m, k]) for k in range(3))
    cur = min(max(int(start), 0), m - 1)
    mind = np.full(m, np.inf, dt)
    indices = np.full(int(n_samples), -1, np.int32)
    dx, dy, dz = np.empty(m, dt), np.empty(m, dt), np.empty(m, dt)  # (reused: no allocation per trip)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(min(int(n_samples), m)):
            indices[t] = cur
            mind[cur] = -1
            np.subtract(x, x[cur], out=dx)
            np.subtract(y, y[cur], out=dy)
            np.subtract(z, z[cur], out=dz)
            np.multiply(dx, dx, out=dx)
            np.multiply(dy, dy, out=dy)
            np.multiply(dz, dz, out=dz)
            np.add(dx, dy, out=dx)
            d = np.add(dx, dz, out=dx)  # (dx*dx + dy*dy) + dz*dz
            mind = np.where(d < mind, d, mind)
            cur = int(np.argmax(mind))
    return indices, mind


def fps_loops(points, n_samples, count=None, start=0):
    """The same, as plain loops written from the definition (slow: small clouds)."""
    points = np.asarray(points)
    T = points.dtype.type
    m = len(points) if count is None else int(count)
    cur = min(max(int(start), 0), m - 1)
    mind = [T(np.inf)] * m
    indices = [-1] * int(n_samples)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(min(int(n_samples), m)):
            indices[t] = cur
            mind[cur] = T(-1)
            for j in range(m):
                dx = T(points[j, 0] - points[cur, 0])
                dy = T(points[j, 1] - points[cur, 1])
                dz = T(points[j, 2] - points[cur, 2])
                d = T(T(T(dx * dx) + T(dy * dy)) + T(dz * dz))
                if d < mind[j]:
                    mind[j] = d
            best = 0
            for j in range(1, m):
                if mind[j] > mind[best]:
                    best = j
            cur = best
    return np.array(indices, np.int32), np.array(mind, points.dtype)


def lattice(side=16, seed=0):
    """The side^3 integer lattice in a seeded random order, float64 ``[side^3, 3]``:
    every squared distance is a small integer, exact in float32, and every trip
    of the selection meets ties."""
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    return g[np.random.default_rng(seed).permutation(len(g))]
