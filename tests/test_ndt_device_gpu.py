"""The device functions of the NDT arithmetic (csrc/ndt_device.h,
csrc/ndt_log.h), one by one through the ndnet_debug_* entries, against the
CPU oracle (or numpy's IEEE arithmetic) bit for bit on the corpora of
tests/ndt_device_cases.py.  tests/test_ndt_device_cpu.py shows those corpora
reach every branch.

Every comparison is on the uint64 / uint32 bit patterns; NaN payloads are
excepted (NaN by position, the bits of everything else).  One launch per
entry (per grid for the voxel keys).
"""
import ctypes

import numpy as np
import pytest

import ndt_device_cases as C

pytestmark = pytest.mark.gpu


def _same_bits(got, ref):
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan)
    g, r = got.view(np.uint64)[~nan], ref.view(np.uint64)[~nan]
    bad = np.flatnonzero(g != r)
    assert bad.size == 0, (bad.size, bad[:5], got[~nan][bad[:5]], ref[~nan][bad[:5]])


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def test_log_matches_host_bits():
    """ndnet_log compiled for gfx950 gives the host build's bits (the host
    build is checked for correct rounding by test_portable_log_correctly_rounded)
    on ~25k inputs; -0.0 -> -inf, negative -> NaN."""
    import torch
    from ndnet import _lib
    x = C.log_cases()
    ref = C.ref_log_cases()
    dx = torch.from_numpy(x.copy()).cuda()
    dy = torch.full((len(x),), 7.0, dtype=torch.float64, device="cuda")
    _lib.check(_lib.lib().ndnet_debug_log(dx.data_ptr(), len(x), dy.data_ptr(), _stream()), "debug_log")
    y = dy.cpu().numpy()
    print(f"log: {len(x)} cases")
    _same_bits(y, ref)
    zero = x == 0
    assert zero.sum() >= 2 and np.signbit(x[zero]).any() and np.isneginf(y[zero]).all()
    assert (x < 0).sum() >= 4 and np.isnan(y[x < 0]).all()
    assert np.isposinf(y[np.isposinf(x)]).all() and np.isnan(y[np.isnan(x)]).all()


def test_kl_pairs_match_oracle():
    """lu3 on both matrices, then kl_event's determinants, flag, lu3_invert
    and kl_score, against orc_kl_pairs: flags equal; where the flag is 1 the
    inverse and the score bit-equal, signed zeros included; 0 elsewhere."""
    import torch
    from ndnet import _lib
    P, Q = C.kl_pair_cases()
    score_h, flag_h, inv_h = C.ref_kl_pairs()
    n = len(P)
    dP, dQ = torch.from_numpy(P.copy()).cuda(), torch.from_numpy(Q.copy()).cuda()
    score = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    flag = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    inv = torch.full((n, 9), 7.0, dtype=torch.float64, device="cuda")
    _lib.check(_lib.lib().ndnet_debug_kl_pairs(dP.data_ptr(), dQ.data_ptr(), n, score.data_ptr(), flag.data_ptr(),
                                               inv.data_ptr(), _stream()), "debug_kl_pairs")
    fl = flag.cpu().numpy().astype(np.uint32)
    print(f"kl pairs: {n} cases, {int(flag_h.sum())} scored")
    assert np.array_equal(fl, flag_h)
    _same_bits(inv.cpu().numpy(), inv_h)
    _same_bits(score.cpu().numpy(), score_h)


def test_voxel_keys_match_oracle():
    """voxel_key equals orc_voxel_keys at every point of every grid, specials
    included (fast exit, wave-uniform fallback and the exact division).
    voxel_key_f32, on the float points not below the offset: equal to the
    oracle wherever it is not kKeyRedo; kKeyRedo for NaN and for a point
    exactly at the offset; decided for at least 99 % of the random points
    (the definition's share on the same points, computed on the CPU, is
    99.81 % or more per grid: test_float_screen_decides_random_points; the
    bound on a continuous uniform point is 99.93 %)."""
    import torch
    from ndnet import _lib
    shares = []
    for g, (c, ref) in enumerate(zip(C.voxel_cases(), C.ref_voxel_cases())):
        pts, fam, f32 = c["points"], c["family"], c["f32"]
        n = len(pts)
        d = torch.from_numpy(pts.copy()).cuda()
        k64 = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        k32 = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        off = (ctypes.c_double * 3)(*c["off"])
        ln = (ctypes.c_uint32 * 3)(*c["len"])
        _lib.check(_lib.lib().ndnet_debug_voxel_keys(d.data_ptr(), n, off, ln, c["vs"], k64.data_ptr(), k32.data_ptr(),
                                                     _stream()), "debug_voxel_keys")
        k64 = k64.cpu().numpy().view(np.uint32)
        k32 = k32.cpu().numpy().view(np.uint32)
        bad = np.flatnonzero(k64 != ref)
        assert bad.size == 0, (g, bad.size, bad[:5], pts[bad[:5]], k64[bad[:5]], ref[bad[:5]])
        decided = f32 & (k32 != C.KEY_REDO)
        bad = np.flatnonzero(decided & (k32 != ref))
        assert bad.size == 0, (g, bad.size, bad[:5], pts[bad[:5]], k32[bad[:5]], ref[bad[:5]])
        nan = f32 & np.isnan(pts).any(axis=1)
        at_off = f32 & (pts == c["off"]).any(axis=1)
        assert nan.sum() >= 3 and (k32[nan] == C.KEY_REDO).all()
        assert at_off.sum() >= 12 and (k32[at_off] == C.KEY_REDO).all()
        rnd = f32 & (fam < 0)
        share = (k32[rnd] != C.KEY_REDO).mean()
        shares.append(share)
        assert (k32[f32 & (fam >= 0)] != C.KEY_REDO).any()  # boundary points the screen does decide are compared too
        assert share >= 0.99, (g, share)
    print("voxel keys:", sum(len(c["points"]) for c in C.voxel_cases()), "points; float screen decided share per grid:",
          [f"{s:.4f}" for s in shares])


def test_fold_division_is_ieee():
    """div_fast on recip_refined(n) -- the light Welford fold's three-step
    division, from the hardware reciprocal -- equals numpy's float64 t / n in
    every bit on ~10^6 pairs over the whole admitted range; for t = +-0 the
    quotient is a zero whose sign is not compared (div_fast's comment).
    The pairs include quotients 1 / (2 n) from a rounding midpoint, the
    hardest a count allows.  (What this cannot tell apart: recip_refined with
    one Newton step instead of two.  The last step q0 + rem * r multiplies the
    errors of q0 and r, 2^-48 or less each after one step from the hardware
    reciprocal (2^-24 or better), and 2^-96 is below the 2^-85 by which a 53-bit by 32-bit
    quotient stays clear of a midpoint; with no Newton step it fails.)"""
    import torch
    from ndnet import _lib
    t, n = C.div_cases()
    ref = t / n.astype(np.float64)
    dt = torch.from_numpy(t.copy()).cuda()
    dn = torch.from_numpy(n.view(np.int32).copy()).cuda()
    dq = torch.full((len(t),), 7.0, dtype=torch.float64, device="cuda")
    _lib.check(_lib.lib().ndnet_debug_div_recip(dt.data_ptr(), dn.data_ptr(), len(t), dq.data_ptr(), _stream()),
               "debug_div_recip")
    q = dq.cpu().numpy()
    print(f"division: {len(t)} pairs")
    zero = t == 0
    assert (q[zero] == 0).all()
    bad = np.flatnonzero((q.view(np.uint64) != ref.view(np.uint64)) & ~zero)
    assert bad.size == 0, (bad.size, bad[:5], t[bad[:5]], n[bad[:5]], q[bad[:5]], ref[bad[:5]])


def test_order_keys():
    """ord_key orders like the values with -0.0 below +0.0 (a stable argsort
    of the keys is the stable sort of the values), ord_unkey inverts it bit
    for bit, and score_key ascending is the score descending with the two
    zeros equal."""
    import torch
    from ndnet import _lib
    x = C.key_cases()
    n = len(x)
    dx = torch.from_numpy(x.copy()).cuda()
    key = torch.zeros((n,), dtype=torch.int64, device="cuda")
    back = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    skey = torch.zeros((n,), dtype=torch.int64, device="cuda")
    _lib.check(_lib.lib().ndnet_debug_ord_keys(dx.data_ptr(), n, key.data_ptr(), back.data_ptr(), skey.data_ptr(),
                                               _stream()), "debug_ord_keys")
    key = key.cpu().numpy().view(np.uint64)
    skey = skey.cpu().numpy().view(np.uint64)
    print(f"keys: {n} cases")
    assert np.array_equal(back.cpu().numpy().view(np.uint64), x.view(np.uint64))
    idx = np.arange(n)
    # value first, then the sign of a zero (negative first), then the position
    want = np.lexsort((idx, ~np.signbit(x), x))
    assert np.array_equal(np.argsort(key, kind="stable"), want)
    assert len(np.unique(key)) == len(np.unique(x.view(np.uint64)))  # distinct bits, distinct keys
    zeros = skey[x == 0]
    assert np.signbit(x[x == 0]).any() and (~np.signbit(x[x == 0])).any() and (zeros == zeros[0]).all()
    with np.errstate(all="ignore"):
        want = np.lexsort((idx, -(x + 0.0)))  # descending score, ties (the zeros too) by position
    assert np.array_equal(np.argsort(skey, kind="stable"), want)
