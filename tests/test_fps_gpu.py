"""Farthest point sampling on the GPU (ndnet_fps_run / ndnet_fps_run_f64 through
ndnet.preprocessing.farthest_point_sample) against the numpy oracle of
fps_ref.py.  The selection is defined operation by operation, so every
comparison is exact: the indices equal the oracle's, and min_dist equals the
oracle's bit for bit.

Sizes: the kernel has two storage boundaries per dtype besides its thread
count (include/ndnet_fps.h): the coordinates of the first
NDNET_FPS_LDS_POINTS_* points are LDS-resident, and the running distances of
the first NDNET_FPS_REG_POINTS_* points are register-resident; each is tested
at -1, 0 and +1.
"""
import os
import re

import numpy as np
import pytest

from conftest import REPO
from fps_ref import fps_ref, lattice

pytestmark = pytest.mark.gpu

DTYPES = ["float32", "float64"]
PAD, SENT = 131, -7


def _header_constants():
    hdr = open(os.path.join(REPO, "include", "ndnet_fps.h")).read()
    return {k: int(v) for k, v in re.findall(r"#define NDNET_FPS_(\w+) (\d+)\n", hdr)}


H = _header_constants()
THREADS = H["THREADS"]
LDS_POINTS = {"float32": H["LDS_POINTS_F32"], "float64": H["LDS_POINTS_F64"]}
REG_POINTS = {"float32": H["REG_POINTS_F32"], "float64": H["REG_POINTS_F64"]}

_refs = {}


def _ref(key, cloud, S, count, start):
    """The oracle's result, computed once per (key, ...) and shared read-only."""
    k = (key, cloud.dtype.str, S, count, start)
    if k not in _refs:
        _refs[k] = fps_ref(cloud, S, count, start)
    return _refs[k]


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _gpu(points, S, counts=None, start=None):
    """(indices [B, S], min_dist [B, n]) as numpy; both outputs sit inside sentinel-filled
    buffers whose margins must come back untouched."""
    import torch
    from ndnet.preprocessing import farthest_point_sample
    B, n, _ = points.shape
    d_pts = torch.from_numpy(points).cuda() if isinstance(points, np.ndarray) else points
    out_buf = torch.full((B * S + 2 * PAD,), SENT, dtype=torch.int32, device="cuda")
    md_buf = torch.full((B * n + 2 * PAD,), float(SENT), dtype=d_pts.dtype, device="cuda")
    out, md = out_buf[PAD:PAD + B * S].view(B, S), md_buf[PAD:PAD + B * n].view(B, n)
    got = farthest_point_sample(d_pts, S, counts=counts, start=start, out=out, min_dist=md)
    assert got is out
    out_h, md_h = out_buf.cpu().numpy(), md_buf.cpu().numpy()
    for buf in (out_h, md_h):
        assert (buf[:PAD] == SENT).all() and (buf[-PAD:] == SENT).all()
    return out_h[PAD:-PAD].reshape(B, S), md_h[PAD:-PAD].reshape(B, n)


def _check(key, points, S, counts=None, start=None):
    """Run the batch and require the oracle's indices and min_dist, cloud by cloud."""
    idx, md = _gpu(points, S, counts, start)
    B, n, _ = points.shape
    assert idx.dtype == np.int32 and md.dtype == points.dtype
    for b in range(B):
        m = n if counts is None else int(counts[b])
        r_idx, r_md = _ref((key, b), points[b], S, None if counts is None else m, 0 if start is None else int(start[b]))
        bad = np.nonzero(idx[b] != r_idx)[0]
        assert not len(bad), (key, b, "first differing sample", int(bad[0]), idx[b][bad[:4]], r_idx[bad[:4]])
        assert np.array_equal(_bits(md[b][:m]), _bits(r_md)), (key, b)
        assert (md[b][m:] == SENT).all()  # entries past counts[b] are not written
    return idx, md


def _gauss(seed, n, dtype, scale=20.0, B=1):
    return (np.random.default_rng(seed).standard_normal((B, n, 3)) * scale).astype(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 7])
def test_fewer_points_than_lanes(n, dtype):
    idx, md = _check(("tiny", n), _gauss(n, n, dtype), n)
    assert sorted(idx[0].tolist()) == list(range(n)) and (md == -1).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [THREADS - 1, THREADS, THREADS + 1])
def test_around_the_thread_count(n, dtype):
    _check(("threads", n), _gauss(n, n, dtype), 64)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("tier", ["lds", "reg"])
def test_around_the_storage_boundaries(tier, delta, dtype):
    n = (LDS_POINTS if tier == "lds" else REG_POINTS)[dtype] + delta
    assert n > THREADS
    _check((tier, n), _gauss(n, n, dtype), 64)


@pytest.mark.parametrize("dtype", DTYPES)
def test_lattice_ties(dtype):
    """The permuted 16^3 lattice: ties on every trip, squared distances exact in float32, so
    the float32 run also equals the float64 oracle."""
    g = np.stack([lattice(16, 0), lattice(16, 1)]).astype(dtype)
    idx, _ = _check("lattice", g, 512)
    for b in range(2):
        r64, _ = _ref(("lattice", b), g[b].astype(np.float64), 512, None, 0)
        assert np.array_equal(idx[b], r64)


@pytest.mark.parametrize("dtype", DTYPES)
def test_duplicates_give_a_permutation(dtype):
    base = _gauss(11, 100, dtype)[0]
    pts = np.repeat(base, 3, axis=0)[np.random.default_rng(12).permutation(300)][None]
    idx, md = _check("dups", pts, 300)
    assert sorted(idx[0].tolist()) == list(range(300)) and (md == -1).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_coordinates(dtype):
    pts = _gauss(13, 700, dtype)
    pts[0, 10, 1], pts[0, 20, 2] = np.nan, np.inf
    idx, md = _check("nonfinite", pts, 50, start=[3])
    assert idx[0, 0] == 3 and set(idx[0, 1:3].tolist()) == {10, 20} and len(set(idx[0].tolist())) == 50
    assert not np.isnan(md).any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_ragged_counts_and_starts(dtype):
    import torch
    n, S = 5000, 64
    counts, start = [n, n // 2 + 1, 37], [0, 5, 36]
    pts = _gauss(14, n, dtype, B=3)
    for b in range(3):
        pts[b, counts[b]:] = np.nan  # the padding is never read into the result
    idx, _ = _check("ragged", pts, S, counts, start)
    assert idx[1, 0] == 5 and idx[2, 0] == 36
    assert (idx[2, 37:] == -1).all() and sorted(idx[2, :37].tolist()) == list(range(37))
    assert (idx[:2] >= 0).all() and (idx[1] < counts[1]).all()
    # counts / start as device tensors of another integer type, start out of range (clamped)
    i2, _ = _gpu(pts, S, torch.tensor(counts, device="cuda", dtype=torch.int64), torch.tensor([0, 5, 99]))
    assert np.array_equal(i2, idx)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,S", [(20000, 256), (100000, 1024)])
def test_full_size(n, S, dtype):
    idx, _ = _check(("full", n), _gauss(n, n, dtype, B=2), S)
    assert len(set(idx[0].tolist())) == S


@pytest.mark.parametrize("dtype", DTYPES)
def test_non_contiguous_points(dtype):
    import torch
    base = torch.from_numpy(_gauss(15, 3000, dtype, B=2)).cuda()
    wide = torch.zeros((2, 3000, 5), dtype=base.dtype, device="cuda")
    wide[..., 1:4] = base
    view = wide[..., 1:4]
    assert not view.is_contiguous()
    a, ma = _gpu(view, 128)
    b, mb = _gpu(base, 128)
    assert np.array_equal(a, b) and np.array_equal(_bits(ma), _bits(mb))
    r, _ = _ref(("noncontig", 0), base[0].cpu().numpy(), 128, None, 0)
    assert np.array_equal(a[0], r)


def test_downsample_gathers_consistently():
    import torch
    from ndnet.preprocessing import farthest_point_sample, fps_downsample
    B, n, S, C = 3, 2500, 200, 28
    rng = np.random.default_rng(16)
    pts = torch.from_numpy(_gauss(16, n, "float32", B=B)).cuda()
    cls = torch.from_numpy(rng.integers(0, C + 1, (B, n))).cuda()
    onehot = torch.nn.functional.one_hot(cls, C + 1).float()
    counts = torch.tensor([n, 1999, 200], dtype=torch.int32)
    p, oh, ids = fps_downsample(pts, S, onehot, cls, counts=counts, start=[1, 2, 3])
    idx = farthest_point_sample(pts, S, counts=counts, start=[1, 2, 3]).long()
    assert p.shape == (B, S, 3) and oh.shape == (B, S, C + 1) and ids.shape == (B, S) and ids.dtype == torch.int64
    for b in range(B):
        assert (idx[b] < int(counts[b])).all() and len(set(idx[b].tolist())) == S
        assert torch.equal(p[b], pts[b][idx[b]]) and torch.equal(ids[b], cls[b][idx[b]])
        assert torch.equal(oh[b], onehot[b][idx[b]])
    assert torch.equal(oh.argmax(-1), ids)
    r, _ = _ref(("gather", 1), pts[1].cpu().numpy(), S, 1999, 2)
    assert np.array_equal(idx[1].cpu().numpy(), r)
    with pytest.raises(ValueError, match="at least n_samples"):
        fps_downsample(pts, S, counts=[n, 1999, 199])


def test_graph_capture_feeds_ndt_preprocessing():
    """farthest_point_sample into preallocated outputs, the gather and ndt_preprocessing in one
    captured graph (4096 -> 2048 points -> 256 NDs), replayed on a second input."""
    import torch
    from ndnet.preprocessing import farthest_point_sample, ndt_preprocessing
    from ndnet.synthetic import make_batch
    B, n, S, k = 2, 4096, 2048, 256
    inputs = [torch.from_numpy(make_batch(kind, B, n)).cuda() for kind in ("U", "L")]
    pts = torch.zeros((B, n, 3), dtype=torch.float32, device="cuda")
    idx = torch.empty((B, S), dtype=torch.int32, device="cuda")
    md = torch.empty((B, n), dtype=torch.float32, device="cuda")
    rows = torch.arange(B, device="cuda")[:, None]

    def step():
        farthest_point_sample(pts, S, out=idx, min_dist=md)
        sub = pts[rows, idx.long()]
        p, c, _ = ndt_preprocessing(k, sub)
        return sub, p, c

    def eager(x):
        i = farthest_point_sample(x, S)
        sub = x[rows, i.long()]
        p, c, _ = ndt_preprocessing(k, sub)
        return [t.clone() for t in (i, sub, p, c)]

    pts.copy_(inputs[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.no_grad(), torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        sub, p, c = step()
    for x in (inputs[1], inputs[0]):
        pts.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        e_idx, e_sub, e_p, e_c = eager(x)
        assert torch.equal(idx, e_idx) and torch.equal(sub, e_sub)
        assert torch.equal(p, e_p) and torch.equal(c, e_c)
    r, _ = _ref(("graph", 0), inputs[0][0].cpu().numpy(), S, None, 0)
    assert np.array_equal(idx[0].cpu().numpy(), r)
