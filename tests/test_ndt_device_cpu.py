"""The corpora of tests/ndt_device_cases.py are what they claim, shown with the
CPU oracle alone: every branch the per-function GPU tests
(tests/test_ndt_device_gpu.py) are meant to reach is reached by some case, so
none of them passes vacuously."""
import numpy as np

import ndt_device_cases as C


def test_kl_corpus_reaches_every_branch():
    """Counted from orc_kl_pairs' outputs and the oracle's LU of the inputs:
    both flags; among the scored pairs each of the six pivot permutations of
    Q, an inverse entry exactly 0 (dgemm's skip-zero rule), a U diagonal whose
    reciprocal is exactly 1, 0 or neither (the three beta rules of tri_UL's
    dgemv), an a12 of exactly 0 (dgemv's skip of a zero x), NaN, -inf and
    +inf scores, and a subnormal determinant ratio."""
    P, Q = C.kl_pair_cases()
    score, flag, inv = C.ref_kl_pairs()
    on = flag == 1
    counts = {"pairs": len(P), "flag0": int((~on).sum()), "flag1": int(on.sum())}
    LUp, _, sp = C.ref_lu(P)
    LUq, perm, sq = C.ref_lu(Q)
    for p in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        counts[f"perm{p}"] = int(((perm == np.array(p)).all(axis=1) & on).sum())
    counts["inv_zero"] = int(((inv == 0).any(axis=1) & on).sum())
    with np.errstate(all="ignore"):
        a11 = 1.0 / LUq[:, 4]
        a22 = 1.0 / LUq[:, 8]
        a12 = (0.0 + LUq[:, 5] * a11) * -a22  # lu3_invert step 1, i = 2
        det = lambda LU, s: ((s.astype(np.float64) * LU[:, 0]) * LU[:, 4]) * LU[:, 8]  # noqa: E731
        ratio = det(LUq, sq) / det(LUp, sp)
    counts["u11_one"] = int(((a11 == 1.0) & on).sum())
    counts["u11_zero"] = int(((a11 == 0.0) & on).sum())
    counts["u11_other"] = int(((a11 != 1.0) & (a11 != 0.0) & on).sum())
    counts["a12_zero"] = int(((a12 == 0.0) & on).sum())
    counts["a12_nonzero"] = int(((a12 != 0.0) & on).sum())
    counts["score_nan"] = int((np.isnan(score) & on).sum())
    counts["score_neg_inf"] = int((np.isneginf(score) & on).sum())
    counts["score_pos_inf"] = int((np.isposinf(score) & on).sum())
    counts["score_finite"] = int((np.isfinite(score) & on).sum())
    tiny = np.finfo(np.float64).tiny
    counts["ratio_subnormal"] = int(((np.abs(ratio) < tiny) & (ratio != 0) & on).sum())
    counts["ratio_zero"] = int(((ratio == 0) & on).sum())
    counts["ratio_inf"] = int((np.isinf(ratio) & on).sum())
    counts["ratio_negative"] = int(((ratio < 0) & on).sum())
    counts["inv_neg_zero"] = int(((inv == 0) & np.signbit(inv) & on[:, None]).sum())
    print("kl corpus:", counts)
    assert len(P) >= 3000
    assert all(v > 0 for v in counts.values()), counts
    # where there is no event the outputs are 0
    assert (score[~on] == 0).all() and (inv[~on] == 0).all()


def test_voxel_corpus_reaches_the_boundaries():
    """In every grid: quotients (p - off) / vs that are exactly an integer,
    and ones within 4 ulp of an integer on either side, in the double run and
    in the float run (there 4 ulp of float32, the screen's precision); in-grid
    and out-of-grid results among the boundary families; all-random waves,
    all-boundary waves and waves with one boundary lane."""
    cases, refs = C.voxel_cases(), C.ref_voxel_cases()
    assert len({c["vs"] for c in cases}) >= 9
    assert any((c["off"] < 0).any() for c in cases) and any((np.abs(c["off"]) > 9e5).any() for c in cases)
    for g, (c, key) in enumerate(zip(cases, refs)):
        assert max(c["len"]) <= 64
        assert (c["off"] == c["off"].astype(np.float32)).all()
        pts, fam, f32 = c["points"], c["family"], c["f32"]
        assert len(pts) % C.WAVE == 37 and (np.flatnonzero(f32)[0] % C.WAVE) == 0
        assert (pts[f32] == pts[f32].astype(np.float32))[~np.isnan(pts[f32])].all()
        assert not (pts[f32] < c["off"]).any()  # the float screen's precondition
        with np.errstate(all="ignore"):
            q = (pts - c["off"]) / c["vs"]  # the oracle's quotient: two IEEE operations
            r = np.rint(q)
            mag = np.maximum(np.abs(q), 1.0)
            ulp = np.where(f32[:, None], np.spacing(np.minimum(mag, 1e30).astype(np.float32)).astype(np.float64),
                           np.spacing(mag))
            ulps = (q - r) / ulp
        fin = np.isfinite(q) & (np.abs(q) < 2.0 ** 40)
        counts = {}
        for name, part in (("f64", ~f32), ("f32", f32)):
            m = part[:, None] & fin
            counts[f"{name}_exact"] = int((m & (ulps == 0)).sum())
            counts[f"{name}_just_below"] = int((m & (ulps < 0) & (ulps >= -4)).sum())
            counts[f"{name}_just_above"] = int((m & (ulps > 0) & (ulps <= 4)).sum())
            b = part & (fam >= 0)
            counts[f"{name}_boundary_in"] = int((b & (key != C.KEY_INVALID)).sum())
            counts[f"{name}_boundary_out"] = int((b & (key == C.KEY_INVALID)).sum())
            counts[f"{name}_random_in"] = int((part & (fam < 0) & (key != C.KEY_INVALID)).sum())
        w = fam[:len(fam) // C.WAVE * C.WAVE].reshape(-1, C.WAVE) >= 0
        nb = w.sum(axis=1)
        counts["waves_all_random"] = int((nb == 0).sum())
        counts["waves_all_boundary"] = int((nb == C.WAVE).sum())
        for lane in (0, 31, 63):
            counts[f"waves_lane{lane}_only"] = int(((nb == 1) & w[:, lane]).sum())
        counts["below_off_special"] = int((fam == 2).sum())
        print(f"voxel grid {g}: n={len(pts)}", counts)
        assert all(v > 0 for v in counts.values()), (g, counts)
    # exact grids (vs = 0.25, integer offsets): d / vs = -1, -2^31 - 1 and -2^32 exactly, and what the reference makes of them
    for c, key in zip(cases[:2], refs[:2]):
        q = (c["points"] - c["off"]) / c["vs"]
        for v in (-1.0, -(2.0 ** 31) - 1.0, -(2.0 ** 32)):
            assert (q == v).any(), v
        wrap = (q == -(2.0 ** 32)).any(axis=1)
        assert (key[wrap] != C.KEY_INVALID).any()  # the low 32 bits are 0: in grid
        assert (key[(q == -1.0).any(axis=1)] == C.KEY_INVALID).all()


def test_float_screen_decides_random_points():
    """voxel_key_f32 leaves a point to the double path where some axis has
    |frac(q) - 1/2| >= half_tol = 1/2 - max(len) 2^-19 >= 1/2 - 2^-13 for
    len <= 64: a uniformly random point is undecided with probability at most
    3 * 2 * 2^-13 < 0.1 %.  The screen's definition evaluated in numpy float32
    on the random float points of every grid decides at least 99 % of them
    (measured: 99.81 % in the grid with an offset near 1e6, where the float
    lattice is coarse, 99.89 % or more in every other grid); 99 % is the cap
    the GPU test asserts for the device's screen on the same points."""
    shares = []
    for c in C.voxel_cases():
        half_tol = np.float32(0.5) - np.float32(max(c["len"])) * np.float32(2.0 ** -19)
        assert half_tol >= np.float32(0.5 - 2.0 ** -13)
        sel = c["f32"] & (c["family"] < 0)
        dec = C.f32_screen_decided(c["points"][sel], c["off"], c["len"], c["vs"])
        shares.append(dec.mean())
        assert sel.sum() >= 1000
        assert dec.mean() >= 0.99, (c["off"], c["vs"], dec.mean())
    print("float screen decided share per grid:", [f"{s:.4f}" for s in shares])


def test_division_corpus_covers_the_admitted_range():
    t, n = C.div_cases()
    assert len(t) >= 1_000_000 and n.min() == 1 and n.max() == (1 << 31) + 1
    e = np.frexp(t[t != 0])[1] - 1
    assert e.min() == -968 and e.max() == 899
    assert (t == 0).sum() >= 2000 and np.signbit(t[t == 0]).sum() >= 1000
    nd = n.astype(np.float64)
    q = t / nd
    short = (q.view(np.uint64) & np.uint64((1 << 31) - 1)) == 0  # at most 21 significant bits: q * n is exact
    exact = short & (q * nd == t) & (t != 0)                     # so t is q times n exactly
    assert exact.sum() > 100_000
    for k in range(32):
        for d in (-1, 0, 1):
            assert (n == max(1, (1 << k) + d)).any()
    assert (t > 0).sum() > 400_000 and (t < 0).sum() > 400_000
    # the midpoint cases: the quotient's mantissa is k + 1/2 -+ 1 / (2 n), checked in integers
    th, nh = t[C.DIV_HARD], n[C.DIV_HARD]
    fr, _ = np.frexp(np.abs(th))
    for m, d in zip((fr * 2.0 ** 53).astype(np.uint64)[::97].tolist(), nh[::97].tolist()):
        a = next(a for a in (d.bit_length() - 1, d.bit_length()) if (1 << 52) <= (m << a) // d < (1 << 53))
        assert abs(2 * ((m << a) % d) - d) == 1, (m, d)
    assert len(np.unique(nh)) > 20_000 and nh.max() == (1 << 31) + 1


def test_key_corpus_has_the_specials():
    x = C.key_cases()
    assert not np.isnan(x).any()
    b = x.view(np.uint64)
    for bits in (0x0, 0x1, 0x000FFFFFFFFFFFFF, 0x0010000000000000, 0x7FEFFFFFFFFFFFFF, 0x7FF0000000000000):
        assert (b == bits).any() and (b == (bits | (1 << 63))).any(), hex(bits)
    assert len(x) > 20_000


def test_log_corpus_has_the_edges():
    """Both sides of every table-index boundary and of the sqrt(2) split are
    in the corpus, as the oracle's own index computation sees them."""
    x = C.log_cases()
    assert 19_000 <= len(x) <= 30_000
    v = x[C.log_positive_finite(x) & (x >= 2.0 ** -1000)]
    m, _ = np.frexp(v)  # [0.5, 1)
    mant = (m * 2).view(np.uint64) & np.uint64((1 << 52) - 1)
    t = np.where(mant > C.LOG_SPLIT_MANT, m, m * 2)  # ndnet_log's t in [sqrt(1/2), sqrt(2)]
    idx = (t * 128.0 + 0.5).astype(int)
    assert idx.min() == C.LOG_TAB_LO and idx.max() == C.LOG_TAB_HI
    for i in range(C.LOG_TAB_LO, C.LOG_TAB_HI):  # an input within 2 ulp on each side of every edge
        edge = (i + 0.5) / 128.0
        for side, sel in ((i, t < edge), (i + 1, t >= edge)):
            near = sel & (np.abs(t - edge) <= 2 * np.spacing(edge))
            assert near.any() and (idx[near] == side).all(), (i, side)
    for dm in (-1, 0, 1):
        assert (mant == C.LOG_SPLIT_MANT + dm).sum() >= 7  # at seven exponents above 2^-1000
    assert (x == 5e-324).any() and np.isnan(x).any() and np.isposinf(x).any() and (x < 0).any()
    assert np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
