"""Ragged batches: a padded [B, n_max, 3] batch plus per-cloud point counts
through the batched NDT path, the points' rows, segment_points and the graphed
step.  Cloud b is the first counts[b] points of a synthetic cloud; what it
yields must be, bit for bit, what the CPU oracle (and a plan of that cloud
alone) yields for the prefix, whatever the padding holds.  Every comparison is
exact (integers, or doubles computed by the same IEEE operations).
"""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 128
N4K, COUNTS8 = 4096, (4096, 2003, 3001, 1024, 640, 129, 1025, 2048)
N16K, COUNTS16K = 16384, (16384, 640, 9001)
ERR_ARG = -20


# ---------------------------------------------------------------- inputs and oracle (computed once, read-only)

@functools.lru_cache(maxsize=None)
def _cloud(kind, n_max, seed):
    from ndnet.synthetic import lidar_cloud, uniform_cloud
    a = {"U": uniform_cloud, "L": lidar_cloud}[kind](n_max, seed)
    a.setflags(write=False)
    return a


def _padded(kind, n_max, counts, seed0=0, pad=np.nan):
    """[B, n_max, 3] float32: cloud b = the first counts[b] points of cloud (n_max, seed0 + b), the rest `pad`."""
    pts = np.stack([_cloud(kind, n_max, seed0 + b) for b in range(len(counts))]).copy()
    for b, c in enumerate(counts):
        pts[b, max(0, min(int(c), n_max)):] = pad
    return pts


@functools.lru_cache(maxsize=None)
def _orc(kind, n_max, seed, count, k=K):
    import oracle as O
    return O.run(_cloud(kind, n_max, seed)[:count].astype(np.float64), k)


# ---------------------------------------------------------------- helpers (as tests/test_ndt_gpu.py has them)

def _dump(plan, cloud: int, nd: int, ne: int):
    from ndnet import _lib
    d = dict(nd_n=np.zeros(nd, np.uint32), nd_mean=np.zeros((nd, 3)), nd_cov_pre=np.zeros((nd, 9)),
             nd_cov_post=np.zeros((nd, 9)), vox=np.zeros(nd, np.uint32), ord_val=np.zeros(max(ne, 1)),
             ord_p=np.zeros(max(ne, 1), np.uint32), ord_q=np.zeros(max(ne, 1), np.uint32),
             guesses=np.zeros(16), counts=np.zeros(16, np.uint32), alive=np.zeros(nd, np.uint8))
    iters = ctypes.c_uint32(0)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rc = _lib.lib().ndnet_ndt_debug_dump(plan.handle, cloud, p(d["nd_n"]), p(d["nd_mean"]), p(d["nd_cov_pre"]),
                                         p(d["nd_cov_post"]), p(d["vox"]), p(d["ord_val"]), p(d["ord_p"]),
                                         p(d["ord_q"]), p(d["guesses"]), p(d["counts"]), ctypes.byref(iters),
                                         p(d["alive"]))
    assert rc == 0
    d["iters"] = iters.value
    return d


def _f32_rows(pc64, cov64, k):
    rows = np.zeros((k, 12), np.float32)
    rows[:, :3] = np.nan_to_num(pc64.astype(np.float32), nan=0.0, posinf=0.0, neginf=0.0)
    rows[:, 3:] = np.nan_to_num(cov64.astype(np.float32), nan=0.0, posinf=0.0, neginf=0.0)
    return rows


class _Run:
    pass


def _run(pts, counts, k=K, path=0, labels=None, ncls=-1, tune=None, dumps=True, vcap=0):
    """One run of a new plan.  counts: a sequence (sent as a device tensor, so no host check) or None;
    vcap: the plan's voxel capacity (0: the default)."""
    import torch
    from ndnet.preprocessing.ndtnet_preprocessing import NdtPlan
    B, n, _ = pts.shape
    r = _Run()
    r.plan = plan = NdtPlan(B, n, k, ncls, vcap)
    if path:
        plan.set_path(path)
        assert plan.path == path
    plan.set_exact_counts(True)
    if tune is not None:
        tune(plan)
    r.d_pts = torch.from_numpy(np.array(pts, dtype=np.float32)).cuda()
    r.d_counts = None if counts is None else torch.tensor([int(c) for c in counts], dtype=torch.int32, device="cuda")
    d_lbl = None if labels is None else torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).cuda()
    r.block = torch.full((B, k, 12), 7.0, dtype=torch.float32, device="cuda")  # zero rows are then the run's
    d_cls = None if labels is None else torch.full((B, k, ncls + 1), 7.0, dtype=torch.float32, device="cuda")
    plan.run(r.d_pts, d_lbl, r.block, d_cls, counts=r.d_counts)
    torch.cuda.synchronize()
    plan.raise_sync_failures()  # no NDNET_ERR_SYNC
    r.out = r.block.cpu().numpy()
    r.out_cls = None if d_cls is None else d_cls.cpu().numpy()
    r.stats = plan.host_stats()
    r.raw = [bytes(s) for s in r.stats]
    r.dumps = None
    if dumps:
        r.dumps = [_dump(plan, b, int(s.num_nds), int(s.num_events)) if s.rc == 0 else None
                   for b, s in enumerate(r.stats)]
    return r


def _path2_allowed(B, n, k=K):
    from ndnet.preprocessing.ndtnet_preprocessing import NdtPlan
    return NdtPlan(B, n, k, -1).path == 2


def _check_cloud(run, b, orc, k=K):
    """Cloud b of a run against the oracle's result for its prefix."""
    st, d, s = run.stats[b], run.dumps[b], orc.search
    assert st.rc == orc.rc == 0, (b, st.rc, orc.rc)
    assert st.iters == len(s.guesses) == d["iters"], b
    assert tuple(st.len) == tuple(s.len) and st.voxel_size == s.voxel_size, b
    assert st.num_nds == s.num_nds and st.num_out == orc.nout, b
    assert np.array_equal(d["guesses"][:st.iters], s.guesses), b
    V = int(np.prod(s.len))
    occ = np.nonzero(orc.vox_n[:V])[0]
    assert len(occ) == s.num_nds
    assert np.array_equal(d["vox"], occ), b
    assert np.array_equal(d["nd_n"], orc.vox_n[occ]), b
    assert np.array_equal(d["nd_mean"], orc.vox_mean[occ]), b
    assert np.array_equal(d["nd_cov_pre"], orc.vox_cov_pre[occ], equal_nan=True), b
    assert np.array_equal(d["alive"], orc.vox_kept[occ]), b
    assert np.array_equal(run.out[b], _f32_rows(orc.out_pc, orc.out_cov, k)), b


def _same_runs(a, b):
    assert np.array_equal(a.out, b.out)
    assert a.raw == b.raw
    for da, db in zip(a.dumps, b.dumps):
        assert (da is None) == (db is None)
        if da is not None:
            for key in da:
                assert np.array_equal(da[key], db[key], equal_nan=True), key


def _paths(B, n):
    return (1, 2) if _path2_allowed(B, n) else (1,)


# ---------------------------------------------------------------- 1, 2: parity with the oracle

@pytest.mark.parametrize("B", [8, 3])  # B % 8 == 0: the XCD-local deal of k_front; 3: the other one
@pytest.mark.parametrize("kind", ["U", "L"])
def test_ragged_batch_matches_oracle_cloud_by_cloud(kind, B):
    counts = COUNTS8[:B]
    pts = _padded(kind, N4K, counts)
    runs = [_run(pts, counts, path=p) for p in _paths(B, N4K)]
    for r in runs:
        for b in range(B):
            orc = _orc(kind, N4K, b, counts[b])
            assert orc.rc == 0 and orc.nout == K  # (as checked on the CPU when the cases were chosen)
            _check_cloud(r, b, orc)
    for r in runs[1:]:
        _same_runs(runs[0], r)


@pytest.mark.parametrize("kind", ["U", "L"])
def test_16384_batch_welford_forms_and_cu_share(kind):
    """12 bisection iterations on U; most workgroups of the 640-point cloud own no point."""
    from ndnet.preprocessing.ndtnet_preprocessing import NdtPlan
    B, counts = 3, COUNTS16K
    pts = _padded(kind, N16K, counts)
    variants = [(1, None)]
    if _path2_allowed(B, N16K):
        variants += [(2, lambda p: p.set_welford_form("quad")), (2, lambda p: p.set_welford_form("light64"))]
        try:  # a CU share of 2, where k_front fits it
            NdtPlan(B, N16K, K, -1).set_cu_share(2)
            variants.append((2, lambda p: p.set_cu_share(2)))
        except RuntimeError:
            pass
    runs = [_run(pts, counts, path=p, tune=t) for p, t in variants]
    for r in runs:
        for b in range(B):
            _check_cloud(r, b, _orc(kind, N16K, b, counts[b]))
    for r in runs[1:]:
        _same_runs(runs[0], r)


# ---------------------------------------------------------------- 3, 4: padding, full counts

@pytest.mark.parametrize("kind", ["U", "L"])
def test_padding_is_inert(kind):
    for path in _paths(8, N4K):
        runs = [_run(_padded(kind, N4K, COUNTS8, pad=pad), COUNTS8, path=path, dumps=False)
                for pad in (0.0, np.nan, np.inf, 1e30)]
        assert all(s.rc == 0 for s in runs[0].stats)
        for r in runs[1:]:
            assert np.array_equal(runs[0].out, r.out) and runs[0].raw == r.raw, path


def test_full_counts_equal_no_counts():
    for kind, B in (("U", 8), ("L", 3)):
        pts = _padded(kind, N4K, (N4K,) * B)
        for path in _paths(B, N4K):
            _same_runs(_run(pts, None, path=path), _run(pts, (N4K,) * B, path=path))


# ---------------------------------------------------------------- 5, 9: a cloud alone, the points' rows

@functools.lru_cache(maxsize=None)
def _ragged8(kind):
    """The B = 8 batch (NaN padding, default path) with its points' rows under both fills."""
    r = _run(_padded(kind, N4K, COUNTS8), COUNTS8)
    r.none = r.plan.point_rows(r.d_pts, fill="none", counts=r.d_counts).cpu().numpy()
    r.near = r.plan.point_rows(r.d_pts, r.block, fill="nearest", counts=r.d_counts).cpu().numpy()
    return r


@functools.lru_cache(maxsize=None)
def _alone(kind, b):
    """Cloud b of the B = 8 batch in a [1, counts[b], 3] plan of its own (no counts, no padding)."""
    c = COUNTS8[b]
    r = _run(_cloud(kind, N4K, b)[None, :c], None)
    r.none = r.plan.point_rows(r.d_pts, fill="none").cpu().numpy()[0]
    r.near = r.plan.point_rows(r.d_pts, r.block, fill="nearest").cpu().numpy()[0]
    return r


@pytest.mark.parametrize("kind", ["U", "L"])
def test_ragged_equals_alone(kind):
    rag = _ragged8(kind)
    for b in range(8):
        one = _alone(kind, b)
        assert np.array_equal(rag.out[b], one.out[0]), b
        assert rag.raw[b] == one.raw[0], b  # every stats field
        for key in one.dumps[0]:
            assert np.array_equal(rag.dumps[b][key], one.dumps[0][key], equal_nan=True), (b, key)


@pytest.mark.parametrize("kind", ["U", "L"])
def test_point_rows_of_a_ragged_batch(kind):
    import torch
    rag = _ragged8(kind)
    checked = 0
    for b, c in enumerate(COUNTS8):
        one = _alone(kind, b)
        for fill in ("none", "near"):
            rows = getattr(rag, fill)[b]
            assert np.array_equal(rows[:c], getattr(one, fill)), (b, fill)
            assert (rows[c:] == -1).all(), (b, fill)
        assert (rag.near[b, :c] >= 0).all() and (rag.none[b, :c] >= 0).any()
        # points per row = the oracle's per-voxel counts of the surviving NDs, for a cloud
        # whose every estimated point is in grid (asserted from the oracle: no worker cut)
        orc = _orc(kind, N4K, b, c)
        V = int(np.prod(orc.search.len))
        if int(orc.vox_n[:V].sum()) == 8 * (c // 8):
            kept = np.nonzero(orc.vox_kept[:V])[0]
            assert len(kept) == orc.nout
            got = rag.none[b]
            assert np.array_equal(np.bincount(got[got >= 0], minlength=len(kept)), orc.vox_n[kept]), b
            checked += 1
    assert checked >= 6
    # finite padding is padding too: the rows do not change when it holds zeros or 1e30
    for pad in (0.0, 1e30):
        p2 = torch.from_numpy(_padded(kind, N4K, COUNTS8, pad=pad)).cuda()
        assert np.array_equal(rag.plan.point_rows(p2, fill="none", counts=rag.d_counts).cpu().numpy(), rag.none)
        assert np.array_equal(rag.plan.point_rows(p2, rag.block, fill="nearest", counts=rag.d_counts).cpu().numpy(),
                              rag.near)


def test_ragged_equals_alone_with_many_bins_per_workgroup():
    """A CU share that gives k_front's workgroups more bins than they hold in
    registers (the bins past the first eight are re-read in every phase, with
    clamped loads): each cloud still equals its run alone."""
    n_max, k, counts = 30_000, 300, (30_000, 17_001, 1_999)
    if not _path2_allowed(3, n_max, k):
        return
    pts = _padded("U", n_max, counts, seed0=40, pad=1e30)
    rag = _run(pts, counts, k=k, path=2, tune=lambda p: p.set_cu_share(42, 1))  # 256 CUs: 2 workgroups of 15 bins
    for b, c in enumerate(counts):
        one = _run(_cloud("U", n_max, 40 + b)[None, :c], None, k=k)
        assert np.array_equal(rag.out[b], one.out[0]) and rag.raw[b] == one.raw[0], b
        for key in one.dumps[0] or ():
            assert np.array_equal(rag.dumps[b][key], one.dumps[0][key], equal_nan=True), (b, key)


# ---------------------------------------------------------------- 6, 7: labels, float64

def test_labelled_ragged_batch():
    import oracle as O
    ncls, B = 5, 8
    labels = np.stack([np.random.default_rng(100 + b).integers(0, 6, N4K) for b in range(B)])
    pts = _padded("U", N4K, COUNTS8)
    expect, seen = [], set()
    for b, c in enumerate(COUNTS8):
        r = O.run(_cloud("U", N4K, b)[:c].astype(np.float64), K, classes=labels[b, :c], num_classes=ncls)
        assert r.rc == 0
        onehot = np.zeros((K, ncls + 1), np.float32)
        onehot[np.arange(K), r.out_cls] = 1.0
        expect.append((onehot, _f32_rows(r.out_pc, r.out_cov, K)))
        seen |= set(r.out_cls[:r.nout].tolist())
    assert len(seen) >= 3  # the classes are not all one value: the check below says something
    for path in _paths(B, N4K):
        got = []
        for fill in (5, 0):  # the padding's labels
            lb = labels.copy()
            for b, c in enumerate(COUNTS8):
                lb[b, c:] = fill
            r = _run(pts, COUNTS8, path=path, labels=lb, ncls=ncls, dumps=False)
            for b in range(B):
                assert np.array_equal(r.out_cls[b], expect[b][0]), (path, fill, b)
                assert np.array_equal(r.out[b], expect[b][1]), (path, fill, b)
            got.append(r)
        assert np.array_equal(got[0].out_cls, got[1].out_cls) and got[0].raw == got[1].raw


def test_float64_entry_with_counts():
    import torch
    import oracle as O
    from ndnet import _lib
    from ndnet.preprocessing.ndtnet_preprocessing import NdtPlan
    B, counts = 3, COUNTS8[:3]
    for kind in ("U", "L"):
        p64 = torch.from_numpy(_padded(kind, N4K, counts).astype(np.float64)).cuda()
        d_counts = torch.tensor(counts, dtype=torch.int32, device="cuda")
        for path in _paths(B, N4K):
            plan = NdtPlan(B, N4K, K, -1)
            plan.set_path(path)
            pc = torch.full((B, K, 3), 7.0, dtype=torch.float64, device="cuda")
            cov = torch.full((B, K, 9), 7.0, dtype=torch.float64, device="cuda")
            cls = torch.full((B, K), 7, dtype=torch.int16, device="cuda")
            blk = torch.full((B, K, 12), 7.0, dtype=torch.float32, device="cuda")
            rc = _lib.lib().ndnet_ndt_run_f64_counts(plan.handle, _lib.stream_ptr(), p64.data_ptr(), None,
                                                     d_counts.data_ptr(), pc.data_ptr(), cov.data_ptr(),
                                                     cls.data_ptr(), blk.data_ptr(), plan.stats.data_ptr())
            assert rc == 0
            torch.cuda.synchronize()
            plan.raise_sync_failures()
            stats = plan.host_stats()
            for b in range(B):
                orc = _orc(kind, N4K, b, counts[b])
                assert stats[b].rc == 0 and stats[b].num_out == orc.nout == K
                assert np.array_equal(pc[b].cpu().numpy(), orc.out_pc), (kind, path, b)
                assert np.array_equal(cov[b].cpu().numpy(), orc.out_cov, equal_nan=True), (kind, path, b)
                assert np.array_equal(blk[b].cpu().numpy(), _f32_rows(orc.out_pc, orc.out_cov, K))


# ---------------------------------------------------------------- 8: invalid and tiny counts

@pytest.mark.parametrize("kind", ["U", "L"])
def test_invalid_and_tiny_counts(kind):
    counts = (4096, 0, 2003, 5000, 3001)
    pts = _padded(kind, N4K, counts)
    runs = []
    for path in _paths(5, N4K):
        r = _run(pts, counts, path=path)
        for b in (1, 3):
            assert r.stats[b].rc == ERR_ARG and r.stats[b].num_out == 0, (path, b)
            assert not r.out[b].any()
            for fill, blk in (("none", None), ("nearest", r.block)):
                rows = r.plan.point_rows(r.d_pts, blk, fill=fill, counts=r.d_counts).cpu().numpy()
                assert (rows[b] == -1).all()
        for b in (0, 2, 4):
            orc = _orc(kind, N4K, b, counts[b])
            assert orc.rc == 0
            _check_cloud(r, b, orc)
        runs.append(r)
    for r in runs[1:]:
        _same_runs(runs[0], r)
    # fewer points than workers
    tiny = (4096, 5, 2003)
    pts = _padded(kind, N4K, tiny)
    for path in _paths(3, N4K):
        r = _run(pts, tiny, path=path)
        assert r.stats[1].rc != 0 and not r.out[1].any()
        _check_cloud(r, 0, _orc(kind, N4K, 0, 4096))
        _check_cloud(r, 2, _orc(kind, N4K, 2, 2003))


# ---------------------------------------------------------------- 10, 11: segment_points, one graph for many lengths

def _small_model():
    import torch
    from ndnet.models.ndtnet import NDTNetSegmentation
    torch.manual_seed(3)
    return NDTNetSegmentation(3, 31, 128).cuda().eval()


def test_segment_points_with_counts():
    import torch
    from ndnet import segment
    model = _small_model()
    pts = torch.from_numpy(_padded("L", N4K, COUNTS8)).cuda()
    counts = torch.tensor(COUNTS8, dtype=torch.int32)  # a CPU tensor: checked on the host, then moved
    gt = torch.from_numpy(np.random.default_rng(9).integers(0, 32, (8, N4K))).int().cuda()
    for fill in ("nearest", "none"):
        labels, lp = segment.segment_points(model, K, pts, fill=fill, counts=counts)
        rows = segment.point_rows(pts, fill)  # the last call's plan, block and counts
        assert labels.shape == (8, N4K) and labels.dtype == torch.int32 and lp.shape == (8, K, 32)
        assert torch.equal(labels, segment.point_labels(lp, rows))
        total = torch.zeros((32, 32), dtype=torch.int64, device="cuda")
        for b, c in enumerate(COUNTS8):
            assert (labels[b, c:] == -1).all() and (rows[b, c:] == -1).all()
            one, _ = segment.segment_points(model, K, pts[b:b + 1, :c].contiguous(), fill=fill)
            total += segment.confusion(one, gt[b:b + 1, :c].contiguous(), 31)
        if fill == "nearest":
            assert all((labels[b, :c] >= 0).all() for b, c in enumerate(COUNTS8))
        conf = segment.confusion(labels, gt, 31)
        assert torch.equal(conf, total)
        assert int(conf.sum()) == int((labels >= 0).sum()) <= sum(COUNTS8)


def _new_batch(kind, counts, seed0):
    import torch
    return torch.from_numpy(_padded(kind, N4K, counts, seed0=seed0)).cuda()


def test_one_graph_serves_many_lengths():
    import torch
    from ndnet import pipeline, segment
    model = _small_model()
    g = pipeline.GraphedSegmentation(model, K, 8, N4K, ragged=True, point_labels="nearest")
    assert g.counts.dtype == torch.int32 and g.counts.tolist() == [N4K] * 8
    short = (2003, 3001, 1024, 640, 129, 1025, 2048, 2003)  # every count <= 3001
    cases = [(_new_batch("L", COUNTS8, 0), COUNTS8), (_new_batch("U", COUNTS8[::-1], 8), COUNTS8[::-1]),
             (_new_batch("L", (N4K,) * 8, 16), (N4K,) * 8), (_new_batch("U", short, 24)[:, :3001], short)]
    for pts, counts in cases:
        lp = g(pts, torch.tensor(counts, dtype=torch.int32)).clone()
        rows, labels = g.point_rows.clone(), g.point_labels.clone()
        # the eager call on what the graph read: a shorter input leaves the rest of the buffer
        # (here: the previous batch's finite points) as padding
        full = g.points.clone()
        assert torch.equal(full[:, :pts.shape[1]].isnan(), pts.isnan())
        cnt = torch.tensor(counts, dtype=torch.int32, device="cuda")
        e_labels, e_lp = segment.segment_points(model, K, full, counts=cnt)
        e_rows = segment.point_rows(full, "nearest")
        assert torch.equal(lp, e_lp) and torch.equal(rows, e_rows) and torch.equal(labels, e_labels)
        for b, c in enumerate(counts):
            assert (labels[b, c:] == -1).all() and (rows[b, c:] == -1).all()
        assert (labels >= 0).any()
    with pytest.raises(ValueError):
        g(counts=[N4K + 1] * 8)
    with pytest.raises(ValueError):
        pipeline.GraphedSegmentation(model, K, 8, N4K)(counts=[N4K] * 8)


def test_one_multilevel_graph_serves_many_lengths():
    import torch
    from ndnet import pipeline
    from ndnet.preprocessing.ndtnet_preprocessing import ndt_multiscale
    model = _small_model()
    levels = (256, 128, 64)
    g = pipeline.GraphedSegmentation(model, levels[0], 8, N4K, levels=levels, ragged=True)
    for seed0, counts in ((0, COUNTS8), (8, COUNTS8[::-1]), (16, (N4K,) * 8)):
        pts = _new_batch("L", counts, seed0)
        outs = [o.clone() for o in g(pts, list(counts))]
        cnt = torch.tensor(counts, dtype=torch.int32, device="cuda")
        with torch.no_grad():
            eager = [model(p, c) for p, c, _ in ndt_multiscale(levels, pts, counts=cnt)]
        assert len(outs) == 3
        for o, e, k in zip(outs, eager, levels):
            assert o.shape == (8, k, 32) and torch.equal(o, e)


# ---------------------------------------------------------------- 12: multiscale

@pytest.mark.parametrize("kind", ["U", "L"])
def test_multiscale_with_counts_equals_legacy_chain(kind):
    import torch
    import oracle as O
    from ndnet.preprocessing.ndtnet_preprocessing import last_stats, ndt_multiscale
    levels, counts = (256, 128), COUNTS8[:3]
    pts = torch.from_numpy(_padded(kind, N4K, counts)).cuda()
    out = ndt_multiscale(levels, pts, counts=list(counts))
    assert [s.rc for s in last_stats()] == [0, 0, 0]
    for b, c in enumerate(counts):
        ch = O.LegacyChain(_cloud(kind, N4K, b)[:c].astype(np.float64))
        for lv, k in enumerate(levels):
            pc, cov = ch.downsample(k) if lv == 0 else ch.prune(k)
            assert ch.rc == 0
            rows = _f32_rows(pc, cov, k)
            assert np.array_equal(out[lv][0][b].cpu().numpy(), rows[:, :3]), (b, k)
            assert np.array_equal(out[lv][1][b].cpu().numpy(), rows[:, 3:]), (b, k)
        ch.cleanup()
