"""The HIP NDT path against the CPU oracle on the adversarial corpus of
tests/ndt_cases.py: stage by stage, through every kernel form, in a ragged
batch and alone, through the float64 legacy entry and the prune levels, the
points' rows, and a small voxel capacity.

Every comparison is exact: integers and doubles bit-equal (the kernels perform
the oracle's IEEE operations), NaN by position (equal_nan), float32 rows after
the driver's cast and nan_to_num.  One ragged batch per k group (NaN padding,
counts on the device), run once and shared read-only by the tests.
"""
import functools

import numpy as np
import pytest

import ndt_cases as C
from test_point_labels import _rows_of_kept, _voxel_index
from test_ragged_gpu import _f32_rows, _path2_allowed, _run, _same_runs

pytestmark = pytest.mark.gpu

BATCHES = {f"k{k}": C.group(k) for k in C.K_GROUPS}
BATCHES.update({c.name: (c,) for c in C.group(64, labelled=True)})  # a labelled plan of its own each


def _inputs(name):
    """(points [B, n_max, 3] NaN-padded, counts, k, labels [B, n_max] or None, num_classes or -1) of a batch."""
    cases = BATCHES[name]
    pts, counts = C.padded(cases)
    ncls = cases[0].num_classes
    labels = None
    if ncls is not None:
        labels = np.zeros(pts.shape[:2], np.int32)
        for b, c in enumerate(cases):
            labels[b, :c.n] = C.case_labels(c)
    return pts, counts, cases[0].k, labels, -1 if ncls is None else ncls


def _go(name, **kw):
    pts, counts, k, labels, ncls = _inputs(name)
    return _run(pts, counts, k=k, labels=labels, ncls=ncls, **kw)


@functools.lru_cache(maxsize=None)
def _base(name):
    """The batch on the default path with every grid counted (read-only)."""
    return _go(name)


def _paths(name):
    pts, _, k, _, _ = _inputs(name)
    return (1, 2) if _path2_allowed(pts.shape[0], pts.shape[1], k) else (1,)


def _same(a, b):
    _same_runs(a, b)
    assert (a.out_cls is None) == (b.out_cls is None)
    assert a.out_cls is None or np.array_equal(a.out_cls, b.out_cls)


# ---------------------------------------------------------------- a: stage by stage against the oracle

def _check_stages(run, b, c):
    """Cloud b of a run against the oracle's run of case c, as
    test_ndt_gpu.test_stages_match_reference_and_oracle checks a fixture."""
    orc = C.oracle_run(c)
    st, d, s, k = run.stats[b], run.dumps[b], orc.search, c.k
    assert st.rc == orc.rc == 0, (c, st.rc)
    # bisection
    it = len(s.guesses)
    assert st.iters == it == d["iters"]
    assert np.array_equal(d["guesses"][:it], s.guesses)
    assert np.array_equal(d["counts"][:it], s.counts)
    assert tuple(st.len) == tuple(s.len) and st.voxel_size == s.voxel_size
    assert np.array_equal(np.array(st.offset[:]), s.off)
    # per-ND state at the accepted size, dense ids in ascending voxel order
    V = int(np.prod(s.len))
    occ = np.nonzero(orc.vox_n[:V])[0]
    nd = len(occ)
    assert st.num_nds == s.num_nds == nd
    assert np.array_equal(d["vox"], occ)
    assert np.array_equal(d["nd_n"], orc.vox_n[occ])
    assert np.array_equal(d["nd_mean"], orc.vox_mean[occ], equal_nan=True)
    assert np.array_equal(d["nd_cov_pre"], orc.vox_cov_pre[occ], equal_nan=True)
    # KL list in the reference's insertion order, after the level-1 prune's left shift
    dense = -np.ones(V + 1, np.int64)
    dense[occ] = np.arange(nd)
    dense[-1] = 0xFFFFFFFF  # index -1: an entry the reference never wrote (poison)
    E = len(orc.ord_div)
    assert st.num_events == E and st.num_kl == orc.post_nkl
    live = orc.post_p >= 0
    assert np.array_equal(d["ord_val"][:E][live], orc.post_div[live], equal_nan=True)
    assert np.array_equal(d["ord_p"][:E], dense[orc.post_p])
    assert np.array_equal(d["ord_q"][:E], dense[orc.post_q])
    # the prune
    assert np.array_equal(d["nd_cov_post"], orc.vox_cov_post[occ], equal_nan=True)
    assert np.array_equal(d["alive"], orc.vox_kept[occ])
    assert st.num_valid == orc.num_valid and st.num_out == orc.nout and st.prune_rc == orc.prune_rc
    # rows as ndt_preprocessing returns them: min(num_out, k) of them, zeros after
    assert np.array_equal(run.out[b], _f32_rows(orc.out_pc, orc.out_cov, k))
    if c.num_classes is not None:
        onehot = np.zeros((k, c.num_classes + 1), np.float32)
        onehot[np.arange(k), orc.out_cls] = 1.0
        assert np.array_equal(run.out_cls[b], onehot)


@pytest.mark.parametrize("name", list(BATCHES))
def test_stages_match_oracle(name):
    run = _base(name)
    for b, c in enumerate(BATCHES[name]):
        _check_stages(run, b, c)


def test_default_path_is_the_front_kernel():
    """Every corpus plan fits k_front (path 2), clouds smaller than a wave included: the
    default runs above are its runs, and the path-1 variant below is the other implementation."""
    for name in BATCHES:
        assert _base(name).plan.path == 2, name
    assert _path2_allowed(1, 8, 1)


def test_two_layers_prune_runs_out_of_list():
    """prune_nds walks off the end of its list (rc -2) with more survivors than
    k: num_out says so, and the k rows written are the oracle's first k."""
    cases = BATCHES["k64"]
    b = [c.name for c in cases].index("two_layers")
    orc, run = C.oracle_run(cases[b]), _base("k64")
    st = run.stats[b]
    assert orc.prune_rc == -2 and orc.nout > 64
    assert st.rc == 0 and st.prune_rc == -2 and st.num_out == orc.nout == st.num_valid
    expect = _f32_rows(orc.out_pc, orc.out_cov, 64)
    assert expect.any(1).sum() == 64  # (every one of the k rows is a survivor's)
    assert np.array_equal(run.out[b], expect)
    assert run.dumps[b]["alive"].sum() == orc.nout


# ---------------------------------------------------------------- b: every kernel form gives the same answer

def _debug(fn, value):
    def tune(plan):
        from ndnet import _lib
        _lib.check(getattr(_lib.lib(), fn)(plan.handle, value), fn)
    return tune


VARIANTS = {
    "path1": dict(path=1),
    "path2": dict(path=2),
    "lazy_on": dict(tune=lambda p: p.set_lazy_list(True)),
    "lazy_off": dict(tune=lambda p: p.set_lazy_list(False)),
    "list_sort0": dict(tune=_debug("ndnet_ndt_debug_set_list_sort", 0)),
    "list_sort1": dict(tune=_debug("ndnet_ndt_debug_set_list_sort", 1)),
    "list_sort3": dict(tune=_debug("ndnet_ndt_debug_set_list_sort", 3)),
    "kl_fuse0": dict(tune=_debug("ndnet_ndt_debug_set_kl_fuse", 0)),
    "kl_fuse1": dict(tune=_debug("ndnet_ndt_debug_set_kl_fuse", 1)),
    "light64": dict(tune=lambda p: p.set_welford_form("light64")),
    "quad": dict(tune=lambda p: p.set_welford_form("quad")),
    "heavy1": dict(tune=lambda p: p.set_heavy_threshold(1)),
    "heavy256": dict(tune=lambda p: p.set_heavy_threshold(256)),
    "heavy_none": dict(tune=lambda p: p.set_heavy_threshold(1 << 31)),
    "cu_share2": dict(tune=lambda p: p.set_cu_share(2)),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", list(BATCHES))
def test_kernel_forms_agree(name, variant):
    """One switch at a time against the default run: rows, classes, every stats field, every dumped intermediate."""
    from ndnet.preprocessing.ndtnet_preprocessing import NdtPlan
    pts, _, k, _, ncls = _inputs(name)
    B, n, _ = pts.shape
    if variant == "path2" and not _path2_allowed(B, n, k):
        return
    if variant == "cu_share2":  # where k_front fits it
        try:
            NdtPlan(B, n, k, ncls).set_cu_share(2)
        except RuntimeError:
            return
    _same(_base(name), _go(name, **VARIANTS[variant]))


@pytest.mark.parametrize("name", list(BATCHES))
def test_skipped_grids_change_nothing(name):
    """Default mode (grids of fewer voxels than k are not counted): the same
    guesses, counted counts, rows, stats and intermediates on every path.
    k_front skips exactly the grids of fewer than k voxels, the extent taken
    from the oracle's limits (an all-negative axis reaches up to DBL_MIN)."""
    base = _base(name)
    any_skipped = False
    for path in _paths(name):
        r = _go(name, path=path, tune=lambda p: p.set_exact_counts(False))
        assert np.array_equal(base.out, r.out) and base.raw == r.raw
        assert base.out_cls is None or np.array_equal(base.out_cls, r.out_cls)
        for c, d1, d0 in zip(BATCHES[name], base.dumps, r.dumps):
            it = d1["iters"]
            skipped = d0["counts"][:it] == 0xFFFFFFFF
            assert np.array_equal(d0["counts"][:it][~skipped], d1["counts"][:it][~skipped])
            for key in d1:
                if key != "counts":
                    assert np.array_equal(d1[key], d0[key], equal_nan=True), (path, key)
            if path == 2:
                lim = C.oracle_run(c).search.lim
                V = [int(np.prod(np.ceil((lim[:3] - lim[3:]) / g))) for g in d1["guesses"][:it]]
                assert skipped.tolist() == [v < c.k for v in V], c.name  # (8 (n / 8) >= k in every case)
                any_skipped |= bool(skipped.any())
    if name in ("k64", "k256") and 2 in _paths(name):
        assert any_skipped


# ---------------------------------------------------------------- c: in a batch equals alone

@pytest.mark.parametrize("b", range(len(BATCHES["k64"])), ids=[c.name for c in BATCHES["k64"]])
def test_in_a_batch_equals_alone(b):
    """A tiny cloud beside a 3096-point neighbour, `far` beside bitmap-grid clouds: each as in a plan of its own."""
    c, rag = BATCHES["k64"][b], _base("k64")
    one = _run(C.cloud(c.cloud)[None], None, k=64)
    assert np.array_equal(rag.out[b], one.out[0])
    assert rag.raw[b] == one.raw[0]
    for key in one.dumps[0]:
        assert np.array_equal(rag.dumps[b][key], one.dumps[0][key], equal_nan=True), key


# ---------------------------------------------------------------- d: the float64 legacy entry and prune levels

@pytest.mark.parametrize("name,k", [("far", 64), ("two_layers", 64), ("lattice_L_x1024", 256), ("blob_singles", 64),
                                    ("tiny_n64", 16)])
def test_legacy_sampler_levels(name, k):
    """NDT_Sampler.downsample(k) -> prune(k / 2) -> prune(k / 4) on float64 points against the oracle's chain."""
    import oracle as O
    from ndnet.preprocessing.ndt_legacy import NDT_Sampler
    pts = C.cloud(C.case(name, k).cloud).astype(np.float64)
    s, ref = NDT_Sampler(pts), O.LegacyChain(pts)
    for lv, kk in enumerate((k, k // 2, k // 4)):
        pc, cov, _ = s.downsample(kk) if lv == 0 else s.prune(kk)
        pc2, cov2 = ref.downsample(kk) if lv == 0 else ref.prune(kk)
        assert s.last_rc == ref.rc, lv
        assert s.num_valid_nds.contents.value == ref.nvalid.value, lv
        assert s.num_kl_divergences.contents.value == ref.nkl.value, lv
        assert np.array_equal(pc, pc2, equal_nan=True), lv
        assert np.array_equal(cov, cov2, equal_nan=True), lv
    assert (s.len_x.contents.value, s.len_y.contents.value, s.len_z.contents.value) == \
        (ref.lx.value, ref.ly.value, ref.lz.value)
    s.cleanup()
    ref.cleanup()


def test_multiscale_batch_matches_oracle_chain():
    """The k = 64 group through ndt_multiscale (64 -> 32 -> 16) with counts: every level of every cloud."""
    import torch
    import oracle as O
    from ndnet.preprocessing.ndtnet_preprocessing import last_stats, ndt_multiscale
    cases, levels = BATCHES["k64"], (64, 32, 16)
    pts, counts = C.padded(cases)
    out = ndt_multiscale(levels, torch.from_numpy(pts).cuda(), counts=list(counts))
    got = [(p.cpu().numpy(), cv.cpu().numpy()) for p, cv, _ in out]
    assert [s.rc for s in last_stats()] == [0] * len(cases)
    for b, c in enumerate(cases):
        ch = O.LegacyChain(C.cloud(c.cloud).astype(np.float64))
        for lv, k in enumerate(levels):
            pc, cov = ch.downsample(k) if lv == 0 else ch.prune(k)
            rows = _f32_rows(pc, cov, k)
            assert np.array_equal(got[lv][0][b], rows[:, :3]), (c.name, k)
            assert np.array_equal(got[lv][1][b], rows[:, 3:]), (c.name, k)
        assert last_stats()[b].prune_rc == ch.rc, c.name
        ch.cleanup()


# ---------------------------------------------------------------- e: the points' rows

def _membership(c, orc):
    """The float64 restatement of the reference's voxel membership of case c on
    the oracle's grid, and whether it reproduces the oracle's per-voxel counts
    (it does unless a reference worker abandoned part of its chunk).  A NaN
    coordinate converts to voxel 0 of its axis, as the reference's does."""
    s, pts = orc.search, C.cloud(c.cloud)
    nan = np.isnan(pts)
    idx = _voxel_index(np.where(nan, s.off.astype(np.float32), pts) if nan.any() else pts, s.off, s.voxel_size, s.len)
    V = int(np.prod(s.len))
    inb = idx[:8 * (c.n // 8)]
    return idx, V, np.array_equal(np.bincount(inb[inb >= 0], minlength=V), orc.vox_n[:V])


@pytest.mark.parametrize("name", ["k64", "k256"])
def test_point_rows(name):
    cases, run = BATCHES[name], _base(name)
    k = cases[0].k
    none = run.plan.point_rows(run.d_pts, fill="none", counts=run.d_counts).cpu().numpy()
    near = run.plan.point_rows(run.d_pts, run.block, fill="nearest", counts=run.d_counts).cpu().numpy()
    fallbacks = []
    for b, c in enumerate(cases):
        orc = C.oracle_run(c)
        idx, V, exact = _membership(c, orc)
        kept = np.nonzero(orc.vox_kept[:V])[0]
        assert len(kept) == orc.nout
        live = np.isfinite(C.cloud(c.cloud)).all(1)  # a point with a non-finite coordinate has no row (ndnet_amd.h)
        got = none[b, :c.n]
        assert (none[b, c.n:] == -1).all() and (near[b, c.n:] == -1).all(), c.name
        if exact:
            expect = _rows_of_kept(idx, kept, c.n, V, k)
            expect[~live] = -1
            assert np.array_equal(got, expect), c.name
        else:  # a cut chunk: points per row = the oracle's per-voxel counts of the surviving NDs
            assert live.all() and int(orc.vox_n[:V].sum()) == 8 * (c.n // 8)
            assert np.array_equal(np.bincount(got[got >= 0], minlength=len(kept))[:k], orc.vox_n[kept][:k]), c.name
            fallbacks.append(c.name)
        assert (near[b, :c.n][live] >= 0).all() and (near[b, :c.n] < min(orc.nout, k)).all(), c.name
        assert (near[b, :c.n][~live] == -1).all(), c.name
        has = got >= 0
        assert has.any() and np.array_equal(near[b, :c.n][has], got[has]), c.name
    assert len(fallbacks) <= 2 and not any(f == "far" or f.startswith("lattice") for f in fallbacks), fallbacks


# ---------------------------------------------------------------- f: capacity

@pytest.mark.parametrize("name", ["k16", "k64"])
def test_voxel_capacity_fails_far_alone(name):
    """A plan of 2^16 voxels per cloud: `far` visits a larger grid and fails
    (rc -1, zero rows) with the same stats on both paths; the batch's other
    clouds still equal the oracle."""
    cases = BATCHES[name]
    far = [c.name for c in cases].index("far")
    runs = [_go(name, path=p, vcap=2 ** 16) for p in _paths(name)]
    for r in runs:
        assert r.stats[far].rc == -1 and r.stats[far].num_out == 0 and not r.out[far].any()
        for b, c in enumerate(cases):
            if b != far:
                _check_stages(r, b, c)
    for r in runs[1:]:
        _same_runs(runs[0], r)
