"""Farthest point sampling, the parts that need no GPU: the numpy oracle
against plain loops, the C ABI's argument checks (nothing is launched), the
wrapper's own checks, whole-scan CARLA_Seg items and collate_padded."""
import numpy as np
import pytest
import torch

from fps_ref import fps_loops, fps_ref, lattice


def _write_scan(path, n, n_classes, seed):
    """A tiny scan in the CARLA PLY layout: 10 header lines; x y z, extra columns, class tag last."""
    rng = np.random.default_rng(seed)
    with open(path, "w") as f:
        f.write(f"ply\nformat ascii 1.0\nelement vertex {n}\nproperty float32 x\nproperty float32 y\n"
                "property float32 z\nproperty float32 CosAngle\nproperty uint32 ObjIdx\nproperty uint32 ObjTag\n"
                "end_header\n")
        for _ in range(n):
            x, y, z = rng.uniform(-80, 80, 3)
            f.write(f"{x:.6f} {y:.6f} {z:.6f} {rng.uniform(-1, 1):.6f} {rng.integers(0, 5000)} "
                    f"{rng.integers(0, n_classes + 1)}\n")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_oracle_agrees_with_plain_loops(dtype):
    rng = np.random.default_rng(3)
    pts = (rng.standard_normal((50, 3)) * 20).astype(dtype)
    pts[11] = pts[4]  # a duplicate: still distinct indices
    for start, count in ((0, None), (7, None), (49, 33), (-3, 50), (99, 20)):
        i1, m1 = fps_ref(pts, 50, count, start)
        i2, m2 = fps_loops(pts, 50, count, start)
        assert np.array_equal(i1, i2) and np.array_equal(m1.view(np.uint8), m2.view(np.uint8))
        m = 50 if count is None else count
        assert sorted(i1[:m].tolist()) == list(range(m)) and (i1[m:] == -1).all() and (m1 == -1).all()
    i1, m1 = fps_ref(pts, 9)
    i2, m2 = fps_loops(pts, 9)
    assert np.array_equal(i1, i2) and np.array_equal(m1.view(np.uint8), m2.view(np.uint8))
    assert (m1[i1] == -1).all() and (np.delete(m1, i1) >= 0).all()


def test_oracle_on_the_lattice_and_on_odd_points():
    g = lattice(8)
    i32, m32 = fps_ref(g.astype(np.float32), 100)
    i64, m64 = fps_ref(g, 100)
    assert np.array_equal(i32, i64) and np.array_equal(m32.astype(np.float64), m64)  # exact in float32
    rng = np.random.default_rng(5)
    pts = rng.standard_normal((60, 3)).astype(np.float32)
    pts[10, 1], pts[20, 2] = np.nan, np.inf
    idx, mind = fps_ref(pts, 30, start=3)
    assert len(set(idx.tolist())) == 30 and set(idx[1:3].tolist()) == {10, 20}  # picked early, and once
    assert not np.isnan(mind).any()


@pytest.mark.parametrize("entry", ["ndnet_fps_run", "ndnet_fps_run_f64"])
def test_argument_checks_launch_nothing(entry):
    from ndnet import _lib
    f = getattr(_lib.lib(), entry)
    E, P = _lib.NDNET_ERR_ARG, 0x1000  # (never dereferenced: every case is refused before any launch)
    assert E == -20
    assert f(None, 1, 8, 4, None, None, P, P, None) == E
    assert f(P, 1, 8, 4, None, None, None, P, None) == E
    assert f(P, 1, 8, 4, None, None, P, None, None) == E
    assert f(P, 0, 8, 4, None, None, P, P, None) == E
    assert f(P, -1, 8, 4, None, None, P, P, None) == E
    assert f(P, 1, 0, 0, None, None, P, P, None) == E
    assert f(P, 1, 8, 0, None, None, P, P, None) == E
    assert f(P, 1, 8, 9, None, None, P, P, None) == E
    assert f(P, 1, 1 << 31, 4, None, None, P, P, None) == E
    assert f(P, 1, 1 << 40, 4, None, None, P, P, None) == E


def test_wrapper_checks_come_before_the_gpu():
    from ndnet.preprocessing import farthest_point_sample, fps_downsample
    pts = torch.zeros((2, 16, 3))
    with pytest.raises(ValueError, match="float32 or float64"):
        farthest_point_sample(pts.half(), 4)
    with pytest.raises(ValueError, match="n_samples"):
        farthest_point_sample(pts, 17)
    with pytest.raises(ValueError, match="n_samples"):
        farthest_point_sample(pts, 0)
    with pytest.raises(ValueError):
        farthest_point_sample(pts[0], 4)
    with pytest.raises(ValueError):
        farthest_point_sample(torch.zeros((2, 16, 4)), 4)
    with pytest.raises(ValueError, match="at least n_samples"):
        fps_downsample(pts, 8, counts=torch.tensor([16, 7]))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):  # valid arguments, no GPU: no CPU fallback
            farthest_point_sample(pts, 4)


def test_whole_scans_and_collate_padded(tmp_path):
    from ndnet.datasets import CARLA_Seg, collate_padded
    from ndnet.datasets.carla_seg import loader, read_ply
    d = tmp_path / "scans"
    d.mkdir()
    sizes = [37, 53]
    for i, n in enumerate(sizes):
        _write_scan(d / f"{i:04d}.ply", n, 28, seed=20 + i)
    ds = CARLA_Seg(28, None, str(d))
    state = np.random.get_state()[1].copy()
    items = [ds[i] for i in range(2)]
    assert np.array_equal(np.random.get_state()[1], state)  # no random choice was made
    for (pts, cls), n, name in zip(items, sizes, ds.filenames):
        xyz, tags = read_ply(str(d / name), 28)
        assert pts.dtype == torch.float32 and pts.shape == (n, 3) and cls.dtype == torch.int64 and cls.shape == (n,)
        assert np.array_equal(pts.numpy(), xyz.astype(np.float32)) and np.array_equal(cls.numpy(), tags)
    points, classes, counts = collate_padded(items)
    assert points.dtype == torch.float32 and points.shape == (2, 53, 3)
    assert classes.dtype == torch.int64 and classes.shape == (2, 53)
    assert counts.dtype == torch.int32 and counts.tolist() == sizes
    for b, (pts, cls) in enumerate(items):
        assert torch.equal(points[b, :len(pts)], pts) and torch.equal(classes[b, :len(cls)], cls)
    assert not points[0, 37:].any() and not classes[0, 37:].any()
    # as the loader's collate_fn (in this process: no workers)
    batches = list(loader(ds, 2, shuffle=False, num_workers=0, collate_fn=collate_padded))
    assert len(batches) == 1
    for got, want in zip(batches[0], (points, classes, counts)):
        assert torch.equal(got, want)
    # an integer n_samples stays what it was
    np.random.seed(1)
    p, gt = CARLA_Seg(28, 16, str(d))[0]
    assert p.shape == (16, 3) and gt.shape == (16, 29)
