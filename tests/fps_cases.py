"""Named cases for farthest point sampling at the boundaries inside k_fps that
the sizes of test_fps_gpu.py do not visit (a helper of test_fps_cases_cpu.py
and test_fps_cases_gpu.py, not a conftest): the register tier's chunks, the
spill tier past REG_POINTS, exact ties across lanes, waves, slabs, chunks and
tiers, degenerate clouds, clouds shorter than n_samples, and more clouds than
the device has CUs.

Every builder is seeded pure numpy, parameterised by dtype, and takes its sizes
from include/ndnet_fps.h: T threads, C slabs per chunk, LDS and REG points of
the dtype's two storage tiers.  A case is a batch ``points [B, n, 3]`` (read
only, cached), ``S`` samples, optional per-cloud ``counts`` and ``start``, and
its marks -- the indices (``marks``) or pairs of indices (``pairs``) whose fate
the case is about.  Clouds are Gaussian of scale 20; the k-th marked position
lies at radius 1000 (1 + k / 10) in a seeded direction, so the selection
certainly reaches it within 64 samples (test_fps_cases_cpu.py asserts that on
the oracle).
"""
import functools
import os
import re
from collections import namedtuple

import numpy as np

DTYPES = ("float32", "float64")
Case = namedtuple("Case", "name points S counts start marks pairs")


def header_constants():
    """The NDNET_FPS_* integers of include/ndnet_fps.h (test_fps_gpu._header_constants' regex)."""
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ndnet_fps.h")).read()
    return {k: int(v) for k, v in re.findall(r"#define NDNET_FPS_(\w+) (\d+)\n", hdr)}


H = header_constants()
T = H["THREADS"]
Sizes = namedtuple("Sizes", "T C LDS REG")


def sizes(dtype):
    sfx = {"float32": "F32", "float64": "F64"}[np.dtype(dtype).name]
    return Sizes(T, H["CHUNK_SLABS_" + sfx], H["LDS_POINTS_" + sfx], H["REG_POINTS_" + sfx])


def chunk_edge_sizes(dtype):
    z = sizes(dtype)
    ct = z.C * z.T
    return [ct - 1, ct, ct + 1, ct + z.T, ct + z.T + 1, 2 * ct + 1]


def tier_edge_sizes(dtype):
    z = sizes(dtype)
    return [z.LDS + 1, z.REG + 1, z.REG + 4 * z.T + 1]


def spill_size(dtype):
    """Four unrolled spill slabs, one remainder slab and a three-point partial slab."""
    z = sizes(dtype)
    return z.REG + 5 * z.T + 3


def _gauss(seed, n, dtype, B=1, scale=20.0):
    return (np.random.default_rng(seed).standard_normal((B, n, 3)) * scale).astype(dtype)


def _far(seed, k, dtype):
    """The k-th marked position: radius 1000 (1 + k / 10), seeded direction."""
    d = np.random.default_rng([seed, k]).standard_normal(3)
    return (d / np.linalg.norm(d) * (1000.0 * (1 + k / 10))).astype(dtype)


def _case(name, points, S, counts=None, start=None, marks=(), pairs=()):
    points.setflags(write=False)
    return Case(name, points, int(S), None if counts is None else [int(c) for c in counts],
                None if start is None else [int(s) for s in start], tuple(int(i) for i in marks),
                tuple((int(a), int(b)) for a, b in pairs))


def _edge_marks(n):
    """The last point, the first point of the last slab and the last point of the slab before it."""
    q0 = (n - 1) // T * T
    return sorted({n - 1, q0, q0 - 1})


def _marked(name, seed, n, dtype):
    pts = _gauss(seed, n, dtype)
    marks = _edge_marks(n)
    for k, i in enumerate(marks):
        pts[0, i] = _far(seed, k, dtype)
    return _case(name, pts, 64, marks=marks)


@functools.lru_cache(maxsize=None)
def chunk_edge(n, dtype):
    """``n`` at and next to a multiple of the chunk: the picks are forced into the tail chunk's
    last, partly filled slab and onto the last point of the slab before it."""
    assert n in chunk_edge_sizes(dtype)
    return _marked(f"chunk_edge_{n}", 100 + n % 97, n, dtype)


@functools.lru_cache(maxsize=None)
def tier_edge_marked(n, dtype):
    """One point past a storage tier (and past four spill slabs), that point certainly picked."""
    assert n in tier_edge_sizes(dtype)
    return _marked(f"tier_edge_{n}", 200 + n % 97, n, dtype)


def _spill_cloud(dtype):
    z = sizes(dtype)
    pts = _gauss(301, spill_size(dtype), dtype)
    pts[0, z.REG:] *= 4  # the far points are the spill tier's: most picks fall there
    return pts


@functools.lru_cache(maxsize=None)
def spill(dtype):
    """Most of the 64 picks inside the spill tier, the first of them its last but one point."""
    pts = _spill_cloud(dtype)
    n = pts.shape[1]
    return _case("spill", pts, 64, start=[n - 2])


@functools.lru_cache(maxsize=None)
def spill_ragged(dtype):
    """The spill cloud four times in one launch, cut to end in four different places: in the
    spill tier's partial slab, one point into it (that point the start), at the register tier's
    end and inside its last slab."""
    z = sizes(dtype)
    base = _spill_cloud(dtype)
    n = base.shape[1]
    counts = [n, z.REG + 1, z.REG, z.REG - z.T + 1]
    pts = np.repeat(base, 4, axis=0)
    for b, c in enumerate(counts):
        pts[b, c:] = np.nan
    return _case("spill_ragged", pts, 64, counts=counts, start=[n - 2, z.REG, 0, 5])


def tie_pairs(dtype):
    z = sizes(dtype)
    n = spill_size(dtype)
    return [(5, z.REG + 700), (z.LDS + 9, z.REG + 3), (z.LDS - 1, z.LDS), (63, 64), (z.T - 1, n - 1),
            (z.REG - 1, z.REG), (z.REG + 4 * z.T - 1, z.REG + 4 * z.T), (z.C * z.T - 1, z.C * z.T)]


@functools.lru_cache(maxsize=None)
def cross_tier_ties(dtype):
    """Eight pairs of exact duplicates, each pair at a marked position of its own: two lanes of
    one wave, two waves, two slabs of one thread, two chunks, two tiers.  On the trip that takes
    a pair's position both members tie exactly; the smaller index is the pick, and the larger is
    at distance 0 of it from then on."""
    pairs = tie_pairs(dtype)
    assert len({i for p in pairs for i in p}) == 16
    pts = _gauss(401, spill_size(dtype), dtype)
    for k, (a, b) in enumerate(pairs):
        pts[0, a] = pts[0, b] = _far(401, k, dtype)
    return _case("cross_tier_ties", pts, 64, pairs=pairs)


DEGENERATE = {"identical": DTYPES, "nan": DTYPES, "overflow": ("float32",), "offset": ("float32",)}


@functools.lru_cache(maxsize=None)
def degenerate(kind, dtype):
    """1500 points (three slabs, the last partial), 600 samples.  ``identical``: one point 1500
    times; ``nan``: every coordinate NaN -- both are picked in index order.  ``overflow``:
    float32 coordinates of +-1e20, so d between any two different points is +inf (and 0 inside
    an octant).  ``offset``: float32 1e4 + U(0, 1), where d has a few bits left."""
    assert dtype in DEGENERATE[kind]
    n, S = 1500, 600
    pts = _gauss(501, n, dtype)
    if kind == "identical":
        pts[:] = pts[0, 7]
    elif kind == "nan":
        pts[:] = np.nan
    elif kind == "overflow":
        pts = np.where(pts < 0, -1e20, 1e20).astype(dtype)
    else:
        pts = (1e4 + np.random.default_rng(502).uniform(0, 1, (1, n, 3))).astype(dtype)
    return _case("degenerate_" + kind, pts, S)


SHORT_COUNTS = [700, 1, 1500, 2000, 0, -3]
SHORT_STARTS = [0, 0, 1499, 5, 7, 7]


@functools.lru_cache(maxsize=None)
def short(dtype):
    """Clouds shorter than n_samples = 1500, among them counts below 1 (clamped to 1: their
    point 0 is NaN padding, and is read), in one launch with a full one."""
    n, S = 2000, 1500
    pts = _gauss(601, n, dtype, B=len(SHORT_COUNTS))
    for b, c in enumerate(SHORT_COUNTS):
        pts[b, max(c, 0):] = np.nan
    return _case("short", pts, S, counts=SHORT_COUNTS, start=SHORT_STARTS)


def effective(case, b):
    """``(m, start)`` of cloud ``b`` as the header clamps them."""
    n = case.points.shape[1]
    m = n if case.counts is None else min(max(case.counts[b], 1), n)
    s = 0 if case.start is None else min(max(case.start[b], 0), m - 1)
    return m, s


@functools.lru_cache(maxsize=None)
def many_clouds(dtype):
    """300 different clouds of 16 .. 100 points: more workgroups than the device has CUs."""
    B, n, S = 300, 100, 16
    rng = np.random.default_rng(701)
    counts = rng.integers(S, n + 1, B)
    counts[:2] = S, n
    pts = _gauss(702, n, dtype, B=B)
    for b, c in enumerate(counts):
        pts[b, c:] = np.nan
    return _case("many_clouds", pts, S, counts=counts, start=rng.integers(0, S, B))
