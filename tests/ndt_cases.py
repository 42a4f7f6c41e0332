"""An adversarial corpus for the NDT stage: small clouds of the kinds the two
smooth generators (ndnet.synthetic) never produce -- axes that are negative for
every point, a far offset, flat and two-layer clouds, int16 lattices at coarse
steps, lines and planes, a heavy ND beside singletons, a NaN in a live point,
clouds smaller than a wave with k down to 1 -- each with its CPU oracle run.

Shared by tests/test_ndt_cases_cpu.py (the corpus is what it claims to be) and
tests/test_ndt_cases_gpu.py (the HIP path against it).  Clouds are seeded,
cached, read-only float32 [n, 3] with at most 4096 points; every case belongs
to a k group in K_GROUPS, so one ragged plan per group runs all of its clouds.
Every (cloud, k) here was first worked out on the CPU: the oracle mallocs each
bisection grid, and a k the cloud cannot reach sends it to 0.01 m voxels.
"""
import functools
from collections import namedtuple

import numpy as np

N_MAX = 4096
K_GROUPS = (1, 2, 16, 64, 256)
TINY_N = (8, 9, 16, 17, 63, 64, 65, 129, 255, 257)
LATTICE_STEPS = (1, 64, 1024)  # multiples of pack_points' default step
DBL_MIN = float(np.finfo(np.float64).tiny)

Case = namedtuple("Case", "name cloud n k num_classes")  # cloud: the key of cloud(); num_classes: None unlabelled


def _ro(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    a.setflags(write=False)
    return a


def _uniform(n, seed, half=10.0):
    return np.random.default_rng(seed).uniform(-half, half, (n, 3))


def _lattice(kind, mult):
    """uniform_cloud / lidar_cloud (4096 points) through the int16 lattice at
    `mult` times the default step, decoded by the format's numpy oracle."""
    import packed_ref
    from ndnet.packed import pack_points
    from ndnet.synthetic import lidar_cloud, uniform_cloud
    src = {"U": uniform_cloud, "L": lidar_cloud}[kind](N_MAX, 0)[None]
    _, qp = pack_points(src)
    q, qp = pack_points(src, step=np.float32(qp[0, 3].item()) * np.float32(mult))
    return packed_ref.decode(q.numpy(), qp.numpy())[0]


def _lines(n, seed):
    rng = np.random.default_rng(seed)
    a, d = rng.uniform(-8, 8, (12, 3)), rng.normal(size=(12, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    i = rng.integers(0, 12, n)
    return a[i] + d[i] * rng.uniform(-6, 6, (n, 1))


def _planes(n, seed):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-8, 8, (n, 3))
    ax = rng.integers(0, 3, n)
    p[np.arange(n), ax] = np.rint(p[np.arange(n), ax])
    return p


@functools.lru_cache(maxsize=None)
def cloud(key):
    """The read-only float32 [n, 3] cloud of a key (a name, or a (name, parameter) tuple)."""
    from ndnet.synthetic import uniform_cloud
    name, arg = key if isinstance(key, tuple) else (key, None)
    if name == "tiny_n":
        return _ro(_uniform(arg, 100 + arg))
    if name in ("neg_octant", "pos_octant", "neg_y", "neg_y_300"):
        off = {"neg_octant": (-20, -20, -20), "pos_octant": (20, 20, 20), "neg_y": (0, -12, 0),
               "neg_y_300": (0, -300, 0)}[name]
        return _ro(uniform_cloud(2003, 11) + np.array(off, np.float32))
    if name == "far":
        return _ro(_uniform(300, 21, 5.0) + np.array([1e5, -3e4, 2e3]))
    if name == "two_layers":
        rng = np.random.default_rng(31)
        return _ro(np.c_[rng.uniform(-5, 5, (1000, 2)), rng.choice([-1.0, 1.0], 1000)])
    if name in ("flat_neg", "flat_zero"):
        a = _uniform(1000, 41, 5.0)
        a[:, 2] = -1.5 if name == "flat_neg" else 0.0
        return _ro(a)
    if name in ("lattice_U", "lattice_L"):
        return _ro(_lattice(name[-1], arg))
    if name == "lattice_half":
        return _ro(np.random.default_rng(51).integers(-16, 17, (1000, 3)) * 0.5)
    if name == "lines":
        return _ro(_lines(2000, 61))
    if name == "planes":
        return _ro(_planes(2000, 71))
    if name == "blob_singles":
        rng = np.random.default_rng(81)
        return _ro(np.r_[rng.normal(0, 0.2, (3000, 3)), rng.uniform(-9, 9, (96, 3))])
    if name == "one_nan":  # arg: the point count; the NaN sits in point 7, or in the n % 8 tail
        a = _uniform(arg, 91)
        a[7 if arg % 8 == 0 else arg - 1, 1] = np.nan
        return _ro(a)
    if name == "lab":
        return _ro(_uniform(1024, 95))
    raise KeyError(key)


@functools.lru_cache(maxsize=None)
def labels(name):
    """int32 [1024] labels of a labelled case."""
    if name == "lab_alt":  # exact ties in most NDs: the first maximum decides
        a = 1 + np.arange(1024) % 2
    else:
        a = np.random.default_rng(97).integers(0, 41, 1024)
    a = a.astype(np.int32)
    a.setflags(write=False)
    return a


def _cases():
    out = []
    sizes = {"neg_octant": 2003, "pos_octant": 2003, "neg_y": 2003, "neg_y_300": 2003, "far": 300, "two_layers": 1000,
             "flat_neg": 1000, "flat_zero": 1000, "lattice_U": N_MAX, "lattice_L": N_MAX, "lattice_half": 1000,
             "lines": 2000, "planes": 2000, "blob_singles": 3096, "lab": 1024}

    def add(name, key, k, ncls=None):  # (n is stated, not measured: importing this module builds no cloud)
        n = key[1] if key[0] in ("tiny_n", "one_nan") else sizes[key[0] if isinstance(key, tuple) else key]
        out.append(Case(name, key, n, k, ncls))

    for n in TINY_N:
        for k in (1, 2) + ((16,) if n >= 64 else ()):
            add(f"tiny_n{n}", ("tiny_n", n), k)
    for name in ("neg_octant", "pos_octant", "neg_y"):
        add(name, name, 64)
        add(name, name, 256)
    add("far", "far", 16)
    add("far", "far", 64)
    for name in ("neg_y_300", "two_layers", "flat_neg", "flat_zero", "blob_singles"):
        add(name, name, 64)
    for kind in "UL":
        for m in LATTICE_STEPS:
            add(f"lattice_{kind}_x{m}", (f"lattice_{kind}", m), 256)
    for name in ("lattice_half", "lines", "planes"):
        add(name, name, 64)
        add(name, name, 256)
    add("one_nan", ("one_nan", 1000), 64)
    add("one_nan_tail", ("one_nan", 1001), 64)
    add("lab_alt", "lab", 64, 2)
    add("lab_40", "lab", 64, 40)
    return tuple(out)


CASES = _cases()
IDS = tuple(f"{c.name}-k{c.k}" for c in CASES)


def case(name, k):
    return CASES[IDS.index(f"{name}-k{k}")]


def group(k, labelled=False):
    """The cases of a k group that share a plan: the unlabelled ones, or (labelled) each labelled one alone."""
    return tuple(c for c in CASES if c.k == k and (c.num_classes is not None) == labelled)


def case_labels(c):
    return None if c.num_classes is None else labels(c.name)


@functools.lru_cache(maxsize=None)
def oracle_run(c):
    """The CPU oracle's run of a case (every stage exposed), computed once."""
    import time
    import oracle as O
    pts, lb = cloud(c.cloud).astype(np.float64), case_labels(c)
    t0 = time.perf_counter()
    r = O.run(pts, c.k, classes=lb, num_classes=c.num_classes or 0)
    r.seconds = time.perf_counter() - t0  # (the oracle call alone: tests/test_ndt_cases_cpu.py bounds it)
    return r


def padded(cases, pad=np.nan):
    """([B, n_max, 3] float32 with `pad` past each cloud, counts) of a group's cases."""
    n_max = max(c.n for c in cases)
    pts = np.full((len(cases), n_max, 3), pad, np.float32)
    for b, c in enumerate(cases):
        pts[b, :c.n] = cloud(c.cloud)
    return pts, tuple(c.n for c in cases)
