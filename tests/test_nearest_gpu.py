"""``ndnet_nearest_sample_run`` and ``ndnet_pn_transform3_run`` on the GPU against
the numpy oracle (tests/nearest_ref.py): rows and distances bit for bit.  The
sizes come from the kernel's two constants, P points per workgroup and L
samples per LDS chunk."""
import ctypes

import numpy as np
import pytest
import torch

from nearest_ref import lattice_case, nearest_ref, transform3_ref


def _consts():
    from ndnet import _lib
    return _lib.NN_TILE_POINTS, _lib.NN_CHUNK_SAMPLES


def _run(pts, smp, counts=None, sample_counts=None, dist_fill=None):
    """nearest_sample on numpy [B, n, 3] / [B, S, 3] -> (rows, dist) numpy; dist pre-set to dist_fill."""
    from ndnet.preprocessing import nearest_sample
    p, s = torch.from_numpy(pts).cuda(), torch.from_numpy(smp).cuda()
    dist = torch.full(p.shape[:2], float("nan") if dist_fill is None else dist_fill, device="cuda")
    out = torch.full(p.shape[:2], -7, dtype=torch.int32, device="cuda")
    rows = nearest_sample(p, s, counts=counts, sample_counts=sample_counts, out=out, dist=dist)
    assert rows is out
    return rows.cpu().numpy(), dist.cpu().numpy()


def _check(pts, smp, counts=None, sample_counts=None):
    rows, dist = _run(pts, smp, counts, sample_counts)
    for b in range(len(pts)):
        r, d = nearest_ref(pts[b], smp[b], None if counts is None else counts[b],
                           None if sample_counts is None else sample_counts[b])
        assert np.array_equal(rows[b], r), b
        assert np.array_equal(dist[b], d, equal_nan=True), b   # NaN past the count: the pre-set value, untouched
    return rows, dist


def test_header_constants_match_the_bindings():
    import os
    import re
    from conftest import REPO
    src = open(os.path.join(REPO, "include", "ndnet_nearest.h")).read()
    vals = {k: int(v) for k, v in re.findall(r"#define (NDNET_NN_\w+) (\d+)", src)}
    assert vals == {"NDNET_NN_TILE_POINTS": _consts()[0], "NDNET_NN_CHUNK_SAMPLES": _consts()[1]}


@pytest.mark.gpu
def test_lattice_with_ties():
    pts, smp = lattice_case()
    rows, dist = _check(pts[None], smp[None])
    assert rows.min() >= 0 and (dist == 0).sum() == 37
    # without out / dist the same rows
    from ndnet.preprocessing import nearest_sample
    again = nearest_sample(torch.from_numpy(pts[None]).cuda(), torch.from_numpy(smp[None]).cuda())
    assert again.dtype == torch.int32 and np.array_equal(again.cpu().numpy(), rows)


@pytest.mark.gpu
def test_tile_and_chunk_edges():
    P, L = _consts()
    rng = np.random.default_rng(1)
    pts = rng.uniform(-50, 50, (2, P + 3, 3)).astype(np.float32)
    smp = rng.uniform(-50, 50, (2, L + 1, 3)).astype(np.float32)
    pts[0, P + 1] = smp[0, L]      # the second chunk's only sample is somebody's nearest
    rows, dist = _check(pts, smp)
    assert rows[0, P + 1] == L and dist[0, P + 1] == 0
    _check(pts[:, :P], smp[:, :L])  # exactly one tile, one chunk
    _check(pts[:1, :1], smp[:1, :1])


@pytest.mark.gpu
def test_ragged_counts_and_padding():
    rng = np.random.default_rng(2)
    counts, sample_counts = [1000, 1, 517], [64, 1, 33]
    pts = rng.uniform(-50, 50, (3, 1000, 3)).astype(np.float32)
    smp = rng.uniform(-50, 50, (3, 64, 3)).astype(np.float32)
    for b in range(3):
        pts[b, counts[b]:] = np.nan if b == 1 else 1e30
        smp[b, sample_counts[b]:] = 1e30 if b == 1 else np.nan
    rows, dist = _run(pts, smp, counts, sample_counts, dist_fill=-123.0)
    for b in range(3):
        r, d = nearest_ref(pts[b], smp[b], counts[b], sample_counts[b])
        m = counts[b]
        assert np.array_equal(rows[b], r) and (rows[b, m:] == -1).all() and rows[b, :m].max() < sample_counts[b]
        assert np.array_equal(dist[b, :m], d[:m])
        assert np.array_equal(dist[b, m:].view(np.uint32), np.full(1000 - m, -123.0, np.float32).view(np.uint32))
    # counts as tensors of another dtype, and outside their range (clamped)
    rows2, _ = _run(pts[:, :, :], smp, torch.tensor([2000, 1, 517]), torch.tensor([99, 1, 33], dtype=torch.int64))
    assert np.array_equal(rows2, rows)
    rows3, dist3 = _run(pts, smp, [0, -4, 5], [64, 64, 0], dist_fill=5.0)
    assert (rows3 == -1).all() and (dist3[:2] == 5.0).all() and np.isinf(dist3[2, :5]).all()


@pytest.mark.gpu
def test_non_finite_points_and_samples():
    rng = np.random.default_rng(3)
    pts = rng.uniform(-50, 50, (2, 300, 3)).astype(np.float32)
    smp = rng.uniform(-50, 50, (2, 40, 3)).astype(np.float32)
    pts[0, 5, 1] = np.nan
    pts[0, 6, 0] = np.inf
    pts[0, 7, 2] = -np.inf
    smp[0, 0] = np.nan             # the first sample: never chosen
    smp[0, 11, 1] = np.nan
    smp[0, 12, 0] = np.inf
    smp[1] = np.nan                # a cloud whose samples are all NaN
    rows, dist = _check(pts, smp)
    assert (rows[0, 5:8] == -1).all() and np.isinf(dist[0, 5:8]).all()
    assert not np.isin(rows[0], [0, 11, 12]).any() and (np.delete(rows[0], [5, 6, 7]) >= 0).all()
    assert (rows[1] == -1).all() and np.isinf(dist[1]).all()


@pytest.mark.gpu
def test_duplicate_samples_give_the_smaller_index():
    rng = np.random.default_rng(4)
    pts = rng.uniform(-5, 5, (1, 200, 3)).astype(np.float32)
    smp = rng.uniform(-5, 5, (1, 16, 3)).astype(np.float32)
    smp[0, 8:] = smp[0, :8]        # every sample twice
    pts[0, :8] = smp[0, 8:]        # points that are samples themselves
    rows, dist = _check(pts, smp)
    assert rows.max() < 8 and np.array_equal(rows[0, :8], np.arange(8)) and (dist[0, :8] == 0).all()


@pytest.mark.gpu
def test_offset_cloud_keeps_the_low_bits():
    """Points at 10^4 + U(0, 1): |p|^2 + |s|^2 - 2 p.s would round the
    distances (~1e-2) away against 3e8; the differences are exact here."""
    rng = np.random.default_rng(5)
    pts = (1e4 + rng.uniform(0, 1, (1, 700, 3))).astype(np.float32)
    smp = pts[:, rng.choice(700, 50, replace=False)].copy()
    rows, dist = _check(pts, smp)
    p64, s64 = pts[0].astype(np.float64), smp[0].astype(np.float64)
    d64 = ((p64[:, None] - s64[None]) ** 2).sum(-1)
    assert np.array_equal(rows[0], d64.argmin(1))  # (coordinate differences are exact in float32 at this offset)
    assert len(np.unique(rows)) == 50


def test_abi_argument_checks_launch_nothing():
    """Every NDNET_ERR_ARG of include/ndnet_nearest.h; the arguments are host
    memory and nothing is launched."""
    from ndnet import _lib

    def ptr(a):
        return a.ctypes.data_as(ctypes.c_void_p)
    E = _lib.NDNET_ERR_ARG
    f = _lib.lib().ndnet_nearest_sample_run
    pts, smp = np.zeros((2, 8, 3), np.float32), np.zeros((2, 4, 3), np.float32)
    rows, dist = np.full((2, 8), 7, np.int32), np.full((2, 8), 7, np.float32)
    good = [ptr(pts), 2, 8, None, ptr(smp), 4, None, ptr(rows), ptr(dist), None]
    for i in (0, 4, 7):  # a NULL d_points, d_samples, d_rows
        a = list(good)
        a[i] = None
        assert f(*a) == E, i
    for i, bad in ((1, 0), (1, -1), (2, 0), (5, 0), (2, 1 << 31), (5, 1 << 31), (2, 1 << 40), (1, 65536)):
        a = list(good)
        a[i] = bad
        assert f(*a) == E, (i, bad)
    assert (rows == 7).all() and (dist == 7).all()
    g = _lib.lib().ndnet_pn_transform3_run
    t1, out = np.zeros((2, 9), np.float32), np.full((2, 8, 3), 7, np.float32)
    good = [ptr(pts), 3, ptr(t1), ptr(out), 3, 2, 8, None]
    for i in (0, 2, 3):
        a = list(good)
        a[i] = None
        assert g(*a) == E, i
    for i, bad in ((1, 2), (1, 0), (1, -3), (4, 2), (5, 0), (5, -1), (5, 65536), (6, 0), (6, 1 << 31)):
        a = list(good)
        a[i] = bad
        assert g(*a) == E, (i, bad)
    assert (out == 7).all()


@pytest.mark.gpu
@pytest.mark.parametrize("p_ld", [3, 4])
def test_transform3_equals_its_definition(p_ld):
    from ndnet import _lib
    B, n = 2, 67
    rng = np.random.default_rng(6 + p_ld)
    rows_in = rng.uniform(-30, 30, (B, n, p_ld)).astype(np.float32)
    if p_ld == 4:
        rows_in[..., 3] = np.nan                  # the fourth column is never read
    t1 = rng.uniform(-2, 2, (B, 3, 3)).astype(np.float32)
    # cloud 1: output 0 is inf - inf = NaN, output 1 overflows to +inf, output 2 to -inf (for x, y > 0)
    t1[1] = np.array([[3e38, -3e38, 0], [3e38, 3e38, 0], [-3e38, -3e38, 1]], np.float32)
    rows_in[1, :, :2] = np.abs(rows_in[1, :, :2]) + 2
    want = np.stack([transform3_ref(rows_in[b], t1[b]) for b in range(B)])
    fmax = np.finfo(np.float32).max
    assert (want[1, :, 0] == 0).all() and (want[1, :, 1] == fmax).all() and (want[1, :, 2] == -fmax).all()
    assert np.isfinite(want).all()
    for o_ld in (3, 4):
        x, t = torch.from_numpy(rows_in).cuda(), torch.from_numpy(t1).cuda()
        out = torch.full((B, n, o_ld), -9.0, device="cuda")
        rc = _lib.lib().ndnet_pn_transform3_run(x.data_ptr(), p_ld, t.data_ptr(), out.data_ptr(), o_ld, B, n,
                                                _lib.stream_ptr(x.device))
        assert rc == 0
        got = out.cpu().numpy()
        assert np.array_equal(got[..., :3], want)
        assert (got[..., 3:] == -9.0).all()       # only three floats of a row are written
