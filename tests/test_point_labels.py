"""Per-point segmentation labels: the row every input point was folded into
(ndnet_ndt_point_rows), the rows' classes gathered to the points
(ndnet_seg_point_labels), the point-level confusion matrix
(ndnet_seg_confusion) and the graphed step that launches them.

The expected membership comes from the fixtures' reference data, not from the
library: voxel = floor((float64(p) - ref_off) / ref_voxel_size), index =
z lx ly + y lx + x, masked to i < 8 (n / 8) -- which reproduces the
reference's own per-voxel counts (asserted below) -- and the expected row of a
voxel is its rank among the voxels the oracle kept, in ascending order.
Integer results throughout: every comparison is exact.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import REPO, golden

pytestmark = pytest.mark.gpu

FIXTURES = ["ndt_U4096_k256_s0.npz", "ndt_U4096_k256_s1.npz", "ndt_L4096_k256_s0.npz", "ndt_L4096_k256_s1.npz",
            "ndt_U2003_k128_s7.npz"]


def _voxel_index(points, off, vs, length):
    """Linear voxel index of every point (float64 restatement of voxel.c:83-103), -1 out of grid."""
    v = np.floor((points.astype(np.float64) - np.asarray(off, np.float64)) / float(vs)).astype(np.int64)
    ln = np.asarray(length, np.int64)
    ok = ((v >= 0) & (v < ln)).all(1)
    idx = (v[:, 2] * ln[1] + v[:, 1]) * ln[0] + v[:, 0]
    return np.where(ok, idx, -1)


def _rows_of_kept(idx, kept_voxels, n, num_voxels, limit):
    """Expected rows: the rank of a point's voxel among the kept voxels (ascending), -1 for a
    voxel not kept, a rank >= limit, an out-of-grid point and the n % 8 tail."""
    kept = np.zeros(num_voxels, bool)
    kept[np.asarray(kept_voxels, np.int64)] = True
    rank = np.cumsum(kept) - 1
    rows = np.full(n, -1, np.int64)
    ok = idx >= 0
    ok[8 * (n // 8):] = False
    hit = ok & kept[np.where(ok, idx, 0)]
    rows[hit] = rank[idx[hit]]
    rows[rows >= limit] = -1
    return rows


def _expected_rows(z):
    n = len(z["points"])
    idx = _voxel_index(z["points"], z["ref_off"], z["ref_voxel_size"], z["ref_len"])
    inb = idx[:8 * (n // 8)]
    # the restatement is the reference's membership: it reproduces its per-voxel counts
    assert np.array_equal(np.bincount(inb[inb >= 0], minlength=len(z["ref_count"])), z["ref_count"])
    return _rows_of_kept(idx, np.nonzero(z["orc_kept"])[0], n, len(z["ref_count"]), int(z["k"]))


_runs = {}


def _fixture_run(name):
    """One run per fixture, shared (read-only) by the tests: plan, device points, device rows
    block, rows under both fills (numpy)."""
    import torch
    from ndnet.preprocessing.ndtnet_preprocessing import NdtPlan
    if name not in _runs:
        z = golden(name)
        k, n = int(z["k"]), len(z["points"])
        plan = NdtPlan(1, n, k, -1)
        pts = torch.from_numpy(np.ascontiguousarray(z["points"][None], dtype=np.float32)).cuda()
        out = torch.empty((1, k, 12), dtype=torch.float32, device="cuda")
        plan.run(pts, None, out, None)
        none = plan.point_rows(pts, fill="none")
        near = plan.point_rows(pts, out, fill="nearest")
        torch.cuda.synchronize()
        assert plan.host_stats()[0].rc == 0
        _runs[name] = dict(z=z, plan=plan, pts=pts, block=out, none=none.cpu().numpy()[0],
                           nearest=near.cpu().numpy()[0], expect=_expected_rows(z))
    return _runs[name]


@pytest.mark.parametrize("name", FIXTURES)
def test_rows_match_reference_membership(name):
    r = _fixture_run(name)
    z, rows = r["z"], r["none"]
    n = len(z["points"])
    assert rows.dtype == np.int32 and rows.shape == (n,)
    assert np.array_equal(rows, r["expect"])
    kept = np.nonzero(z["orc_kept"])[0]
    assert np.array_equal(np.bincount(rows[rows >= 0], minlength=len(kept)), z["ref_count"][kept])
    if n % 8:
        assert (rows[-(n % 8):] == -1).all() and (r["nearest"][-(n % 8):] >= 0).all()
    # the fixtures leave points without a row (pruned NDs, the n % 8 tail): fill=none says so
    without = {"ndt_L4096_k256_s0.npz": 1046, "ndt_U4096_k256_s0.npz": 817, "ndt_U2003_k128_s7.npz": 79}
    assert (rows < 0).any() and (name not in without or (rows < 0).sum() == without[name])


def test_batch_of_mixed_clouds():
    """Four clouds in one plan: each equals its single-cloud result (no leak
    between clouds); a failed cloud (test_edge_clouds' flat cloud: z constant,
    rc -3) beside a good one has no rows under either fill and leaves the good
    cloud's rows as they are."""
    import torch
    from ndnet.preprocessing.ndtnet_preprocessing import NdtPlan
    names = FIXTURES[:4]
    pts = np.stack([golden(f)["points"] for f in names]).astype(np.float32)
    plan = NdtPlan(4, 4096, 256, -1)
    d_pts = torch.from_numpy(pts).cuda()
    out = torch.empty((4, 256, 12), dtype=torch.float32, device="cuda")
    plan.run(d_pts, None, out, None)
    none = plan.point_rows(d_pts).cpu().numpy()
    near = plan.point_rows(d_pts, out, fill="nearest").cpu().numpy()
    for b, f in enumerate(names):
        single = _fixture_run(f)
        assert np.array_equal(none[b], single["none"]), f
        assert np.array_equal(near[b], single["nearest"]), f
    # a failed cloud beside a good one
    rng = np.random.default_rng(5)
    n, k = 4101, 200
    flat = rng.uniform(-5, 5, (n, 3)).astype(np.float32)
    flat[:, 2] = 1.5
    good = np.concatenate([pts[0], pts[0][:n - 4096] + np.float32(0.25)])  # padded to the same n
    res = {}
    for key, batch in (("single", good[None]), ("pair", np.stack([flat, good]))):
        B = len(batch)
        plan = NdtPlan(B, n, k, -1)
        d = torch.from_numpy(np.ascontiguousarray(batch)).cuda()
        o = torch.empty((B, k, 12), dtype=torch.float32, device="cuda")
        plan.run(d, None, o, None)
        res[key] = (plan.point_rows(d).cpu().numpy(), plan.point_rows(d, o, fill="nearest").cpu().numpy(),
                    [s.rc for s in plan.host_stats()])
    assert res["single"][2] == [0] and res["pair"][2] == [-3, 0]
    for fill in (0, 1):
        assert (res["pair"][fill][0] == -1).all()
        assert np.array_equal(res["pair"][fill][1], res["single"][fill][0])
    assert (res["single"][0][0] >= 0).any() and (res["single"][1][0] >= 0).all()


def test_rows_follow_prune_levels():
    """256 -> 128 -> 64 (plan.prune): after each level the rows match an
    expectation built from the oracle chain's rows -- every row's float64 mean
    matched against the oracle's voxel means recovers the kept set -- on both
    launch paths; ndt_multiscale leaves its last level's block and plan for
    ndnet.segment.point_rows."""
    import torch
    import oracle as O
    from ndnet import segment
    from ndnet.preprocessing.ndtnet_preprocessing import NdtPlan, ndt_multiscale
    levels = (256, 128, 64)
    pts = np.stack([golden("ndt_U4096_k256_s0.npz")["points"], golden("ndt_L4096_k256_s0.npz")["points"]])
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    n = pts.shape[1]
    expect = []  # [cloud][level] -> rows
    for b in range(2):
        p64 = pts[b].astype(np.float64)
        r = O.run(p64, levels[0])
        assert r.rc == 0
        V = int(np.prod(r.search.len))
        means = {tuple(r.vox_mean[v]): v for v in np.nonzero(r.vox_n[:V])[0]}
        assert len(means) == r.search.num_nds  # the voxel means are distinct: a mean names its voxel
        idx = _voxel_index(pts[b], r.search.off, r.search.voxel_size, r.search.len)
        ch = O.LegacyChain(p64)
        per_level = []
        for lv, k in enumerate(levels):
            pc, _ = ch.downsample(k) if lv == 0 else ch.prune(k)
            assert ch.rc == 0
            kept = [means[tuple(m)] for m in pc]
            assert kept == sorted(kept) and len(set(kept)) == k
            per_level.append(_rows_of_kept(idx, kept, n, V, k))
        ch.cleanup()
        expect.append(per_level)
    d_pts = torch.from_numpy(pts).cuda()
    got = {}
    for path in (1, 2):
        plan = NdtPlan(2, n, levels[0], -1)
        plan.set_path(path)
        assert plan.path == path
        got[path] = []
        for lv, k in enumerate(levels):
            blk = torch.empty((2, k, 12), dtype=torch.float32, device="cuda")
            if lv == 0:
                plan.run(d_pts, None, blk, None)
            else:
                plan.prune(k, blk)
            rows = plan.point_rows(d_pts, blk, num_nds=k).cpu().numpy()
            near = plan.point_rows(d_pts, blk, num_nds=k, fill="nearest").cpu().numpy()
            for b in range(2):
                assert np.array_equal(rows[b], expect[b][lv]), (path, lv, b)
                has = rows[b] >= 0
                assert np.array_equal(near[b][has], rows[b][has]) and (near[b] >= 0).all() and (near[b] < k).all()
            got[path].append((rows, near))
    for (r1, n1), (r2, n2) in zip(got[1], got[2]):
        assert np.array_equal(r1, r2) and np.array_equal(n1, n2)
    # ndt_multiscale remembers its last level's block beside the plan
    out = ndt_multiscale(levels, d_pts)
    rows = segment.point_rows(d_pts).cpu().numpy()
    assert np.array_equal(rows, got[1][2][0])
    near = segment.point_rows(d_pts, fill="nearest").cpu().numpy()
    assert np.array_equal(near, got[1][2][1])
    assert out[2][0].shape == (2, levels[2], 3)


def test_worker_cut_is_honoured():
    """A float32 cloud whose x extent is exactly 25 voxels of the first guess
    (374.875 = 25 * 14.995): the point on the grid maximum is out of grid, its
    reference worker abandons the rest of its chunk (normal_distributions.c
    :47-52) and the oracle accepts that grid.  The abandoned points have no
    row, on both launch paths; the expectation is the numpy restatement with
    the cut, which reproduces the oracle's per-voxel counts."""
    import torch
    import oracle as O
    from ndnet.preprocessing.ndtnet_preprocessing import NdtPlan
    rng = np.random.default_rng(12)
    n, k, bad = 4096, 90, 1300
    a = np.stack([rng.uniform(0, 374.875, n), rng.uniform(0, 59.9, n), rng.uniform(0, 14.9, n)], 1).astype(np.float32)
    a[5] = [0, 0, 0]
    a[bad] = [374.875, 30.0, 7.0]
    r = O.run(a.astype(np.float64), k)
    assert r.rc == 0 and r.search.voxel_size == 14.995 and tuple(r.search.len) == (25, 4, 1)
    V = 100
    idx = _voxel_index(a, r.search.off, r.search.voxel_size, r.search.len)
    chunk = n // 8
    assert np.nonzero(idx < 0)[0].tolist() == [bad]
    cut = np.arange(n)
    idx[(cut >= bad) & (cut < (bad // chunk + 1) * chunk)] = -1  # the worker's abandoned points
    assert np.array_equal(np.bincount(idx[idx >= 0], minlength=V), r.vox_n[:V])
    assert r.vox_n[:V].sum() == n - ((bad // chunk + 1) * chunk - bad) < n
    expect = _rows_of_kept(idx, np.nonzero(r.vox_kept[:V])[0], n, V, k)
    d = torch.from_numpy(a[None]).cuda()
    for path in (1, 2):
        plan = NdtPlan(1, n, k, -1)
        plan.set_path(path)
        assert plan.path == path
        out = torch.empty((1, k, 12), dtype=torch.float32, device="cuda")
        plan.run(d, None, out, None)
        rows = plan.point_rows(d).cpu().numpy()[0]
        near = plan.point_rows(d, out, fill="nearest").cpu().numpy()[0]
        st = plan.host_stats()[0]
        assert st.rc == 0 and st.num_out == r.nout
        assert np.array_equal(rows, expect), path
        assert (rows[bad:(bad // chunk + 1) * chunk] == -1).all() and (near >= 0).all()
        _check_nearest(a, out.cpu().numpy()[0][:, :3], rows, near, k)


def _d64(points32, means32):
    """Squared distances in float64 from fp32 points to fp32 row means: [points, rows]."""
    d = points32.astype(np.float64)[:, None, :] - means32.astype(np.float64)[None, :, :]
    return (d * d).sum(2)


def _check_nearest(points32, means32, rows_none, rows_near, nrows):
    """A point with a row keeps it; one without gets a row within (1 + 1e-6) of the float64
    minimum over rows < nrows: the margin covers the four fp32 roundings (each <= 2^-24
    relative) of a sum of non-negative terms, on both sides of the comparison."""
    has = rows_none >= 0
    assert np.array_equal(rows_near[has], rows_none[has])
    fill = np.nonzero(~has)[0]
    assert len(fill)
    got = rows_near[fill]
    assert (got >= 0).all() and (got < nrows).all()
    d = _d64(points32[fill], means32[:nrows])
    assert (d[np.arange(len(fill)), got] <= d.min(1) * (1 + 1e-6)).all()
    return fill


@pytest.mark.parametrize("name", FIXTURES)
def test_nearest_fill(name):
    import torch
    r = _fixture_run(name)
    z, plan, pts, block = r["z"], r["plan"], r["pts"], r["block"]
    k = int(z["k"])
    p32 = np.ascontiguousarray(z["points"], dtype=np.float32)
    blk = block.cpu().numpy()[0]
    fill = _check_nearest(p32, blk[:, :3], r["none"], r["nearest"], k)
    # a planted exact tie: the lowest row wins.  Row 5 takes row 3's mean (as the issue asks), and
    # -- so that the tie is certainly met -- a higher row takes the mean of the row most points
    # were filled with
    popular = int(np.bincount(r["nearest"][fill], minlength=k).argmax())
    for lo, hi in ((3, 5), (popular, popular + 1 if popular + 1 < k else None)):
        if hi is None:
            continue
        tied = block.clone()
        tied[0, hi, :3] = tied[0, lo, :3]
        rows = plan.point_rows(pts, tied, fill="nearest").cpu().numpy()[0]
        assert not (rows[fill] == hi).any()
        assert np.array_equal(rows[r["none"] >= 0], r["none"][r["none"] >= 0])
        if lo == popular:
            assert (rows[fill] == lo).any()
    # a non-finite coordinate (planted in a copy given only to point_rows) stays -1 under both fills
    with_row, without = int(np.nonzero(r["none"] >= 0)[0][7]), int(fill[0])
    bad = pts.clone()
    bad[0, with_row, 1] = float("nan")
    bad[0, without, 2] = float("inf")
    for f in ("none", "nearest"):
        rows = plan.point_rows(bad, block, fill=f).cpu().numpy()[0]
        assert rows[with_row] == -1 and rows[without] == -1
        keep = np.ones(len(rows), bool)
        keep[[with_row, without]] = False
        assert np.array_equal(rows[keep], r[f][keep])
    assert torch.equal(plan.point_rows(pts, block, fill="nearest").cpu(), torch.from_numpy(r["nearest"])[None])


def test_nearest_fill_skips_rows_past_the_survivors():
    """A level with fewer survivors than rows: pruned to 64, then asked for 128
    (prune_nds' "desired > valid", rc -1: the 64 survivors stay, rows 64..127
    are zero).  No point gets a row >= num_out, although the zero rows lie at
    the origin, nearer to many points than any survivor."""
    import torch
    from ndnet.preprocessing.ndtnet_preprocessing import NdtPlan
    z = golden("ndt_U4096_k256_s0.npz")
    p32 = np.ascontiguousarray(z["points"], dtype=np.float32)
    pts = torch.from_numpy(p32[None]).cuda()
    plan = NdtPlan(1, 4096, 256, -1)
    out = torch.empty((1, 256, 12), dtype=torch.float32, device="cuda")
    plan.run(pts, None, out, None)
    b64 = torch.empty((1, 64, 12), dtype=torch.float32, device="cuda")
    plan.prune(64, b64)
    rows64 = plan.point_rows(pts, b64, num_nds=64).cpu().numpy()[0]
    b128 = torch.empty((1, 128, 12), dtype=torch.float32, device="cuda")
    plan.prune(128, b128)
    st = plan.host_stats()[0]
    assert st.prune_rc == -1 and st.num_out == 64
    blk = b128.cpu().numpy()[0]
    assert np.array_equal(blk[:64], b64.cpu().numpy()[0]) and not blk[64:].any()
    none = plan.point_rows(pts, b128, num_nds=128).cpu().numpy()[0]
    near = plan.point_rows(pts, b128, num_nds=128, fill="nearest").cpu().numpy()[0]
    assert np.array_equal(none, rows64)
    fill = _check_nearest(p32, blk[:, :3], none, near, 64)
    # the zero rows would have won for some of them
    d = _d64(p32[fill], blk[:, :3])
    assert (d[:, 64:].min(1) < d[:, :64].min(1)).any()
    assert near.max() < 64


def _scores(rng, B, k, cols):
    s = rng.standard_normal((B, k, cols)).astype(np.float32)
    flat = s.reshape(B * k, cols)
    if cols > 1:
        flat[0, cols // 2] = np.nan                      # a NaN counts as the maximum
        if len(flat) > 1:
            flat[1, :] = 0.25                            # an all-equal row: the first column
        if len(flat) > 2:
            flat[2, [cols - 1, cols // 3]] = 9.0         # an exact tie of the maximum: the first wins
        if len(flat) > 3:
            flat[3, [0, cols - 1]] = np.nan              # two NaNs: the first
        if len(flat) > 4:
            flat[4, 0], flat[4, cols - 1] = 0.0, -0.0    # +0 and -0 are equal
            flat[4, 1:cols - 1] = -1.0
    return s


def _np_argmax(s):
    """First maximum per row, NaN as a maximum (torch.argmax / ndnet_row_argmax)."""
    nan = np.isnan(s)
    a = np.where(nan, np.inf, s)
    a = np.where(nan.any(-1, keepdims=True) & ~nan, -np.inf, a)
    return a.argmax(-1).astype(np.int32)


@pytest.mark.parametrize("cols", [1, 2, 29, 65, 301])
def test_point_labels_and_argmax(cols):
    import torch
    from ndnet import _lib
    rng = np.random.default_rng(cols)
    B, PAD, SENT, UN = 3, 67, -77, -5
    for k in (1, 63, 256):
        s = _scores(rng, B, k, cols)
        nd_ref = _np_argmax(s)
        assert np.array_equal(nd_ref, torch.from_numpy(s).argmax(-1).numpy())
        d_s = torch.from_numpy(s).cuda()
        for n in (1, 65, 4099):
            rows = rng.integers(-1, k, (B, n)).astype(np.int32)
            rows[0, 0] = -1
            rows[-1, -1] = k - 1
            d_rows = torch.from_numpy(rows).cuda()
            nd_buf = torch.full((B * k + 2 * PAD,), SENT, dtype=torch.int32, device="cuda")
            pl_buf = torch.full((B * n + 2 * PAD,), SENT, dtype=torch.int32, device="cuda")
            nd, pl = nd_buf[PAD:PAD + B * k].view(B, k), pl_buf[PAD:PAD + B * n].view(B, n)
            rc = _lib.lib().ndnet_seg_point_labels(d_s.data_ptr(), d_rows.data_ptr(), B, n, k, cols, UN,
                                                   nd.data_ptr(), pl.data_ptr(), _lib.stream_ptr())
            assert rc == 0
            nd_h, pl_h = nd_buf.cpu().numpy(), pl_buf.cpu().numpy()
            for buf in (nd_h, pl_h):
                assert (buf[:PAD] == SENT).all() and (buf[-PAD:] == SENT).all()
            assert np.array_equal(nd_h[PAD:-PAD].reshape(B, k), nd_ref), (k, n)
            expect = np.where(rows >= 0, np.take_along_axis(nd_ref, np.maximum(rows, 0), 1), UN)
            assert np.array_equal(pl_h[PAD:-PAD].reshape(B, n), expect), (k, n)
    # the Python wrapper, default unassigned -1
    from ndnet import segment
    got = segment.point_labels(d_s, d_rows).cpu().numpy()
    assert got.dtype == np.int32
    assert np.array_equal(got, np.where(rows >= 0, np.take_along_axis(nd_ref, np.maximum(rows, 0), 1), -1))


def _conf_ref(pred, gt, cols):
    ok = (pred >= 0) & (pred < cols) & (gt >= 0) & (gt < cols)
    ref = np.bincount(gt[ok].astype(np.int64) * cols + pred[ok], minlength=cols * cols + 1).astype(np.uint64)
    ref[cols * cols] = (~ok).sum()
    return ref


def test_confusion_counts():
    import torch
    from ndnet import _lib, segment
    X = _lib.SEG_CONF_LDS_MAX_COLS  # the LDS histogram's last width (include/ndnet_segment.h)
    hdr = open(os.path.join(REPO, "include", "ndnet_segment.h")).read()
    assert f"#define NDNET_SEG_CONF_LDS_MAX_COLS {X}\n" in hdr
    rng = np.random.default_rng(8)
    for cols in (1, 2, 29, X, X + 1, 301):
        for count in (1, 63, 64, 65, 100003):
            pred = rng.integers(-2, cols + 2, count).astype(np.int32)  # out of range on both sides
            gt = rng.integers(-2, cols + 2, count).astype(np.int32)
            if count > 2:
                pred[:2], gt[:2] = (cols - 1, 0), (0, cols - 1)
            start = rng.integers(0, 1 << 40, cols * cols + 1).astype(np.uint64)  # accumulates: 64-bit counters
            conf = torch.from_numpy(start.view(np.int64).copy()).cuda()
            d_pred, d_gt = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
            rc = _lib.lib().ndnet_seg_confusion(d_pred.data_ptr(), d_gt.data_ptr(), count, cols, conf.data_ptr(),
                                                _lib.stream_ptr())
            assert rc == 0
            torch.cuda.synchronize()
            assert np.array_equal(conf.cpu().numpy().view(np.uint64), start + _conf_ref(pred, gt, cols)), (cols, count)
    # the wrapper: int64 [C + 1, C + 1], [gt, pred], out-of-range points left out
    got = segment.confusion(d_pred, d_gt, cols - 1)
    assert got.dtype == torch.int64 and got.shape == (cols, cols)
    assert np.array_equal(got.cpu().numpy().ravel().astype(np.uint64), _conf_ref(pred, gt, cols)[:-1])


def _dump_vox_alive(plan, cloud, nd):
    from ndnet import _lib
    nd_n, vox, alive = np.zeros(nd, np.uint32), np.zeros(nd, np.uint32), np.zeros(nd, np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    iters = ctypes.c_uint32(0)
    rc = _lib.lib().ndnet_ndt_debug_dump(plan.handle, cloud, p(nd_n), None, None, None, p(vox), None, None, None,
                                         None, None, ctypes.byref(iters), p(alive))
    assert rc == 0
    return nd_n, vox, alive


def test_full_size_rows_agree_with_the_run():
    """100k -> 1000 (one U and one L cloud), where the fp32 key screen's double
    fallback fires: the rows' counts are the run's own per-ND counts (the
    debug dump the parity tests pin) for the first min(num_out, k) survivors,
    and every assigned point's key, recomputed in numpy, is its ND's voxel."""
    import torch
    from ndnet.preprocessing.ndtnet_preprocessing import NdtPlan
    from ndnet.synthetic import make_batch
    n, k = 100_000, 1000
    pts = np.concatenate([make_batch("U", 1, n), make_batch("L", 1, n)])
    d_pts = torch.from_numpy(pts).cuda()
    plan = NdtPlan(2, n, k, -1)
    out = torch.empty((2, k, 12), dtype=torch.float32, device="cuda")
    plan.run(d_pts, None, out, None)
    rows = plan.point_rows(d_pts).cpu().numpy()
    near = plan.point_rows(d_pts, out, fill="nearest").cpu().numpy()
    stats = plan.host_stats()
    for b in range(2):
        st = stats[b]
        assert st.rc == 0
        nd_n, vox, alive = _dump_vox_alive(plan, b, int(st.num_nds))
        surv = np.nonzero(alive)[0][:min(int(st.num_out), k)]
        assert np.array_equal(np.bincount(rows[b][rows[b] >= 0], minlength=len(surv)), nd_n[surv])
        idx = _voxel_index(pts[b], st.offset[:], st.voxel_size, st.len[:])
        has = rows[b] >= 0
        assert np.array_equal(idx[has], vox[surv[rows[b][has]]].astype(np.int64))
        assert np.array_equal(near[b][has], rows[b][has]) and (near[b] >= 0).all() and (near[b] < len(surv)).all()
        # a sample of the filled points against float64 (the whole cloud would be 1e8 distances)
        fill = np.nonzero(~has)[0][:1024]
        if len(fill):
            d = _d64(pts[b][fill], out[b, :len(surv), :3].cpu().numpy())
            assert (d[np.arange(len(fill)), near[b][fill]] <= d.min(1) * (1 + 1e-6)).all()


def _small_model():
    import torch
    from ndnet.models.ndtnet import NDTNetSegmentation
    torch.manual_seed(3)
    return NDTNetSegmentation(3, 31, 128).cuda().eval()


def test_graphed_point_labels_equal_eager(monkeypatch):
    import torch
    from ndnet import pipeline, segment
    B, N, k = 2, 4096, 256
    model = _small_model()
    inputs = [np.stack([golden(FIXTURES[0])["points"], golden(FIXTURES[2])["points"]]),
              np.stack([golden(FIXTURES[3])["points"], golden(FIXTURES[1])["points"]])]
    inputs = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda() for a in inputs]
    calls = {"rows": 0, "labels": 0}
    real_rows, real_labels = segment.point_rows, segment.point_labels

    def spy_rows(*a, **kw):
        calls["rows"] += 1
        return real_rows(*a, **kw)

    def spy_labels(*a, **kw):
        calls["labels"] += 1
        return real_labels(*a, **kw)

    monkeypatch.setattr(segment, "point_rows", spy_rows)
    monkeypatch.setattr(segment, "point_labels", spy_labels)
    plain = pipeline.GraphedSegmentation(model, k, B, N)
    assert calls == {"rows": 0, "labels": 0}  # the default graph launches neither
    assert plain.point_labels is None and plain.point_rows is None
    graphed = pipeline.GraphedSegmentation(model, k, B, N, point_labels="nearest")
    assert calls["rows"] >= 2 and calls["rows"] == calls["labels"]  # warm-up and capture
    monkeypatch.undo()
    for pts in inputs + inputs[:1]:
        lp = graphed(pts).clone()
        labels, rows = graphed.point_labels.clone(), graphed.point_rows.clone()
        lp_plain = plain(pts).clone()
        e_labels, e_lp = segment.segment_points(model, k, pts)
        e_rows = segment.point_rows(pts, fill="nearest")
        assert labels.dtype == torch.int32 and labels.shape == (B, N)
        assert torch.equal(lp, lp_plain)  # bit for bit: the point labels change nothing upstream
        assert torch.equal(lp, e_lp)
        assert torch.equal(rows, e_rows) and torch.equal(labels, e_labels)
        assert (labels >= 0).all() and (labels <= 31).all()
        assert torch.equal(labels, torch.gather(e_lp.argmax(-1), 1, rows.long()).int())
    none = pipeline.GraphedSegmentation(model, k, B, N, point_labels="none")
    none(inputs[1])
    e_labels, _ = segment.segment_points(model, k, inputs[1], fill="none")
    assert torch.equal(none.point_labels, e_labels) and (e_labels == -1).any()
    assert torch.equal(none.point_rows, segment.point_rows(inputs[1]))


def test_point_rows_write_no_plan_state():
    """ndt_preprocessing's rows and stats before and after point_rows calls on
    its plan are bit-equal, and so is a further prune level."""
    import torch
    from ndnet import segment
    from ndnet.preprocessing.ndtnet_preprocessing import ndt_preprocessing
    pts = torch.from_numpy(np.stack([golden(FIXTURES[2])["points"], golden(FIXTURES[0])["points"]])).cuda()

    def level2(plan):
        blk = torch.empty((2, 100, 12), dtype=torch.float32, device="cuda")
        plan.prune(100, blk)
        return blk.cpu(), [bytes(s) for s in plan.host_stats()]

    p, c, _ = ndt_preprocessing(256, pts)
    plan = ndt_preprocessing.last_plan
    before = (p.cpu().clone(), c.cpu().clone(), [bytes(s) for s in plan.host_stats()], level2(plan))
    p, c, _ = ndt_preprocessing(256, pts)
    assert ndt_preprocessing.last_plan is plan and ndt_preprocessing.last_rows.shape == (2, 256, 12)
    r0 = segment.point_rows(pts)
    r1 = segment.point_rows(pts, fill="nearest")
    assert torch.equal(r0, segment.point_rows(pts)) and torch.equal(r1[r0 >= 0], r0[r0 >= 0])
    after_l2 = level2(plan)
    p2, c2, _ = ndt_preprocessing(256, pts)
    after = (p2.cpu(), c2.cpu(), [bytes(s) for s in plan.host_stats()])
    assert torch.equal(before[0], p.cpu()) and torch.equal(before[1], c.cpu())
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1]) and before[2] == after[2]
    assert torch.equal(before[3][0], after_l2[0]) and before[3][1] == after_l2[1]


def test_point_rows_rejects_misuse():
    import torch
    from ndnet import _lib
    from ndnet.preprocessing.ndtnet_preprocessing import NdtPlan
    z = golden(FIXTURES[4])
    n, k = len(z["points"]), int(z["k"])
    plan = NdtPlan(1, n, k, -1)
    pts = torch.from_numpy(z["points"][None]).cuda()
    out = torch.full((1, n), 9, dtype=torch.int32, device="cuda")
    blk = torch.zeros((1, k, 12), device="cuda")
    f = _lib.lib().ndnet_ndt_point_rows
    st = _lib.stream_ptr()
    E = _lib.NDNET_ERR_ARG
    assert f(plan.handle, st, None, blk.data_ptr(), k, 0, out.data_ptr()) == E
    assert f(plan.handle, st, pts.data_ptr(), blk.data_ptr(), k, 0, None) == E
    assert f(plan.handle, st, pts.data_ptr(), blk.data_ptr(), 0, 0, out.data_ptr()) == E
    assert f(plan.handle, st, pts.data_ptr(), blk.data_ptr(), k + 1, 0, out.data_ptr()) == E
    assert f(plan.handle, st, pts.data_ptr(), blk.data_ptr(), k, 2, out.data_ptr()) == E
    assert f(plan.handle, st, pts.data_ptr(), None, k, 1, out.data_ptr()) == E
    # a plan whose last run was the float64 entry point
    p64 = pts.double()
    rc = _lib.lib().ndnet_ndt_run_f64(plan.handle, st, p64.data_ptr(), None, None, None, None, blk.data_ptr(), None)
    assert rc == 0
    assert f(plan.handle, st, pts.data_ptr(), blk.data_ptr(), k, 0, out.data_ptr()) == E
    torch.cuda.synchronize()
    assert (out == 9).all()  # nothing was launched
    with pytest.raises(ValueError):
        plan.point_rows(pts, fill="nearest")
    with pytest.raises(ValueError):
        plan.point_rows(pts, fill="mean")
