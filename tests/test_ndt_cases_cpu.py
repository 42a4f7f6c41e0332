"""The NDT corpus (tests/ndt_cases.py) is what it claims to be: every case is
accepted by the CPU oracle quickly and within 2^20 voxels per visited grid, and
has the property it exists for.  Where the reference's compiled estimate stage
(oracle/_ref) is present, the oracle is pinned to it on every case, bit for
bit.  The truth here is the oracle alone; no GPU.
"""
import os

import numpy as np
import pytest

import ndt_cases as C
import oracle as O

ALL = pytest.mark.parametrize("c", C.CASES, ids=C.IDS)


def _occ(r):
    V = int(np.prod(r.search.len))
    return np.nonzero(r.vox_n[:V])[0]


def _grid_sizes(s):
    """Voxels of every visited grid, from the limits {max_xyz, min_xyz} and the guesses."""
    ext = s.lim[:3] - s.lim[3:]
    return [int(np.prod(np.ceil(ext / g))) for g in s.guesses]


def test_table():
    assert len(set(C.IDS)) == len(C.IDS)
    for c in C.CASES:
        assert c.k in C.K_GROUPS and 8 <= c.n <= C.N_MAX and c.k <= c.n
        a = C.cloud(c.cloud)
        assert a.shape == (c.n, 3) and a.dtype == np.float32 and not a.flags.writeable
        assert not np.isinf(a).any() and len(np.unique(a, axis=0)) > 1
        assert np.isnan(a).any() == c.name.startswith("one_nan")
    # every k group has clouds of several sizes (a ragged batch), the labelled plans stand alone
    assert all(len({c.n for c in C.group(k)}) > 1 for k in C.K_GROUPS)
    assert [c.name for c in C.group(64, labelled=True)] == ["lab_alt", "lab_40"]


@ALL
def test_oracle_accepts(c):
    r = C.oracle_run(c)
    s = r.search
    assert r.rc == 0 and s.rc == 0
    assert 1 <= len(s.guesses) < 15
    assert max(_grid_sizes(s)) <= 2 ** 20
    assert r.seconds < 1.0
    assert int(np.prod(s.len)) == _grid_sizes(s)[-1] and s.num_nds == len(_occ(r)) >= c.k


@pytest.mark.parametrize("name,axes", [("neg_octant", (0, 1, 2)), ("neg_y", (1,)), ("neg_y_300", (1,)), ("far", (1,)),
                                       ("flat_neg", (2,)), ("pos_octant", ())])
def test_all_negative_axes_keep_dbl_min(name, axes):
    for c in (c for c in C.CASES if c.name == name):
        pts, lim = C.cloud(c.cloud), C.oracle_run(c).search.lim
        for a in range(3):
            if a in axes:
                assert pts[:, a].max() < 0 and lim[a] == C.DBL_MIN
            else:
                assert lim[a] == pts[:, a].max() > 0
        assert np.array_equal(lim[3:], pts.min(0).astype(np.float64))


def test_flat_zero_has_a_one_layer_grid():
    """z = 0 for every point: the maximum stays DBL_MIN > 0 = the minimum, one layer of voxels."""
    s = C.oracle_run(C.case("flat_zero", 64)).search
    assert s.lim[2] == C.DBL_MIN and s.lim[5] == 0.0 and s.len[2] == 1
    assert C.oracle_run(C.case("flat_neg", 64)).search.len[2] == 2


@pytest.mark.parametrize("k", [16, 64])
def test_far_is_anisotropic_and_past_the_bitmap(k):
    s = C.oracle_run(C.case("far", k)).search
    assert max(_grid_sizes(s)) > 32768 and s.len[1] > 1000 and max(s.len[0], s.len[2]) < 8


def test_two_layers_runs_out_of_list():
    r = C.oracle_run(C.case("two_layers", 64))
    assert r.prune_rc == -2 and r.nout > 64 and r.nout == r.num_valid < r.search.num_nds


@pytest.mark.parametrize("kind", ["U", "L"])
def test_coarse_lattices_have_duplicates_and_zero_covariances(kind):
    c = C.case(f"lattice_{kind}_x1024", 256)
    pts, r = C.cloud(c.cloud), C.oracle_run(c)
    assert len(np.unique(pts, axis=0)) < c.n
    occ = _occ(r)
    zero = ~r.vox_cov_pre[occ].any(1)
    assert zero.any()
    if kind == "L":  # ... also of an ND with several (identical) samples
        assert (zero & (r.vox_n[occ] > 1)).any()
    # the finer lattices are the same scan: the points differ, the point count does not
    fine = C.cloud((f"lattice_{kind}", 1))
    assert fine.shape == pts.shape and not np.array_equal(fine, pts)


def test_lattice_half_has_duplicates_and_face_points():
    pts = C.cloud("lattice_half")
    assert len(np.unique(pts, axis=0)) < len(pts) and np.array_equal(pts * 2, np.rint(pts * 2))


def test_blob_singles():
    r = C.oracle_run(C.case("blob_singles", 64))
    n = r.vox_n[_occ(r)]
    assert n.max() >= 256 and (n == 1).sum() >= 10


def test_tiny_n_reaches_the_degenerate_grids():
    runs = [(c, C.oracle_run(c)) for c in C.CASES if c.name.startswith("tiny_n")]
    assert len(runs) == 2 * len(C.TINY_N) + sum(n >= 64 for n in C.TINY_N)
    assert any(tuple(r.search.len) == (1, 1, 1) for _, r in runs)
    assert any(len(r.ord_div) == 0 for _, r in runs)
    assert any(len(r.ord_div) > 0 and c.k <= 2 for c, r in runs)
    assert all(r.nout == c.k for c, r in runs)
    # a cloud of 8 points: one point per reference worker
    assert any(c.n == 8 and r.vox_n.sum() == 8 for c, r in runs)


def test_lab_alt_has_both_classes_and_ties():
    c = C.case("lab_alt", 64)
    r = C.oracle_run(c)
    assert set(r.out_cls[:r.nout].tolist()) == {1, 2}
    # an ND with as many points of class 1 as of class 2 exists: the first maximum decided it
    pts, lb = C.cloud(c.cloud).astype(np.float64), C.labels("lab_alt")
    s = r.search
    v = np.floor((pts - s.off) / s.voxel_size).astype(np.int64)
    idx = (v[:, 2] * s.len[1] + v[:, 1]) * s.len[0] + v[:, 0]
    V = int(np.prod(s.len))
    assert np.array_equal(np.bincount(idx, minlength=V), r.vox_n[:V])
    tied = np.bincount(idx[lb == 1], minlength=V) == np.bincount(idx[lb == 2], minlength=V)
    assert (tied & (r.vox_n[:V] > 0)).any()
    r40 = C.oracle_run(C.case("lab_40", 64))
    assert len(set(r40.out_cls[:r40.nout].tolist())) >= 10


def test_one_nan():
    r = C.oracle_run(C.case("one_nan", 64))
    occ = _occ(r)
    assert np.isnan(r.vox_mean[occ]).any(1).sum() == 1
    assert np.isfinite(r.search.lim).all() and r.vox_n[occ].sum() == 1000  # the NaN point is in the grid
    # in the n % 8 tail no worker reads it
    t = C.oracle_run(C.case("one_nan_tail", 64))
    assert not np.isnan(t.vox_mean[_occ(t)]).any() and t.vox_n[_occ(t)].sum() == 1000
    assert np.isnan(C.cloud(("one_nan", 1001))[1000]).any()


@pytest.mark.skipif(not os.path.exists(O.REF_LIB), reason="oracle/_ref is built only where the reference sources exist")
@ALL
def test_oracle_matches_compiled_reference(c):
    """ref_search on guesses, counts, grid and voxel size; ref_estimate on counts, means and covariances."""
    r = C.oracle_run(c)
    s = r.search
    pts = C.cloud(c.cloud).astype(np.float64)
    rc, g, cnt, ln, off, vs = O.ref_search(pts, c.k)
    assert rc == 0
    assert np.array_equal(g, s.guesses) and np.array_equal(cnt, s.counts)
    assert tuple(ln) == tuple(s.len) and vs == s.voxel_size and np.array_equal(off, s.off)
    V = int(np.prod(s.len))
    n, mean, cov, cls, nn = O.ref_estimate(pts, vs, ln, off, classes=C.case_labels(c), num_classes=c.num_classes or 0)
    assert nn == s.num_nds
    assert np.array_equal(n, r.vox_n[:V])
    assert np.array_equal(mean, r.vox_mean[:V], equal_nan=True)
    assert np.array_equal(cov, r.vox_cov_pre[:V], equal_nan=True)
    if c.num_classes is not None:
        assert np.array_equal(cls[n > 0], r.vox_cls[:V][n > 0])
