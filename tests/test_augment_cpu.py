"""The augmentation without a GPU: the oracle of aug_ref.py against Philox's
known answers and its own invariants, ndnet_aug_run's argument checks (host
memory: nothing reaches a GPU before NDNET_ERR_ARG), and Augment's."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import aug_ref as R
from conftest import REPO


def _tile():
    hdr = open(os.path.join(REPO, "include", "ndnet_augment.h")).read()
    return int(re.search(r"#define NDNET_AUG_TILE (\d+)\n", hdr).group(1))


# ---------------------------------------------------------------- the oracle

VECTORS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,out", VECTORS)
def test_philox_known_answers(ctr, key, out):
    got = R.philox(*ctr, *key)
    assert tuple(int(w) for w in got) == out
    # ... and as one element of an array of counters
    got = R.philox(np.array([5, ctr[0]]), np.array([6, ctr[1]]), np.array([7, ctr[2]]), np.array([8, ctr[3]]), *key)
    assert tuple(int(w[1]) for w in got) == out


def test_counter_layout_around_the_high_word():
    assert R.counter(9, 2, 2 ** 32 - 1, 1) == (9, 2, 0xffffffff, 1)
    assert R.counter(9, 2, 2 ** 32, 1) == (9, 2, 0, (1 << 2) | 1)
    assert R.counter(0, 0, 2 ** 32, 0) == (0, 0, 0, 4)
    assert R.counter(3, 1, 2 ** 62 - 1, 2) == (3, 1, 0xffffffff, 0xfffffffe)
    # the two steps draw different words, and the purposes of one step do too
    cfg = R.Config(seed=3)
    a, b = R.point_words(cfg, 0, 8, 2 ** 32 - 1), R.point_words(cfg, 0, 8, 2 ** 32)
    assert not (a == b).any(axis=0).all() and not np.array_equal(a[:4], a[4:])


def _cloud(seed, B, n):
    rng = np.random.default_rng(seed)
    return rng.uniform(-50, 50, (B, n, 3)).astype(np.float32)


def test_identity_config_returns_its_input():
    pts = _cloud(1, 2, 777)
    pts[0, 3] = (0.0, 1.5, -2.0)  # +0.0 is fine; the input holds no -0.0
    assert not np.signbit(pts[pts == 0]).any()
    labels = np.random.default_rng(2).integers(0, 9, (2, 777)).astype(np.int32)
    counts = np.array([777, 300])
    for step in (0, 5, 2 ** 40):
        X, T, idx, out, lab = R.augment(R.Config(seed=11), pts, labels, counts, step)
        assert (T == 0).all()
        assert np.array_equal(X.reshape(2, 3, 4)[:, :, :3], np.broadcast_to(np.eye(3, dtype=np.float32), (2, 3, 3)))
        for b in range(2):
            m = counts[b]
            assert np.array_equal(idx[b], np.arange(m))
            assert np.array_equal(out[b].view(np.uint32), pts[b, :m].view(np.uint32))
            assert np.array_equal(lab[b], labels[b, :m])


def test_kept_set_shrinks_as_the_threshold_grows():
    W = R.point_words(R.Config(seed=4, stream=1), 2, 5000, 17)
    prev = None
    for T in (0, 1, 2 ** 20, 2 ** 31, 2 ** 32 - 2 ** 20, 2 ** 32 - 1):
        k = R.keep_mask(W, T)
        assert k[0]
        if prev is not None:
            assert not (k & ~prev).any() and k.sum() <= prev.sum()
        prev = k
    assert R.keep_mask(W, 0).all() and 1 <= R.keep_mask(W, 2 ** 32 - 1).sum() < 5
    # the count of a real threshold is binomial: 5000 draws at p = 1/2, within 5 sigma
    assert abs(int(R.keep_mask(W, 2 ** 31).sum()) - 2500) < 5 * math.sqrt(1250)


def test_jitter_has_zero_mean_and_unit_variance():
    N = 300_000
    W = R.point_words(R.Config(seed=2024), 0, N // 3, 0)
    z = np.concatenate([R.jitter_z(W, a) for a in range(3)]).astype(np.float64)
    assert z.size == N
    mean, var = z.mean(), z.var()
    print(f"JITTER mean {mean:.3e} var {var:.6f} range {z.min():.3f} .. {z.max():.3f}")
    assert abs(mean) <= 4 / math.sqrt(N)
    assert abs(var - 1) <= 4 * math.sqrt(2 / N)
    assert np.abs(z).max() <= 131070 * float(R.K) + 1e-6 < 3.47


def test_cloud_params_ranges_and_structure():
    cfg = R.Config(seed=7, yaw_max=math.pi, scale_lo=0.9, scale_hi=1.1, shift_max=(1.0, 2.0, 0.5), drop_max=0.25,
                   flip_x_16=16384, flip_y_16=65536)
    X, T, flips = R.cloud_params(cfg, 4096, 3)
    X = X.reshape(-1, 3, 4)
    assert (X[:, 0, 2] == 0).all() and (X[:, 1, 2] == 0).all() and (X[:, 2, :2] == 0).all()
    s = X[:, 2, 2].astype(np.float64)
    assert (s >= np.float32(0.9)).all() and (s <= np.float32(1.1)).all()
    assert np.allclose(np.abs(np.linalg.det(X[:, :, :3].astype(np.float64))), s ** 3, rtol=1e-5)
    assert (np.abs(X[:, :, 3]) <= np.array([1.0, 2.0, 0.5], np.float32)).all()
    assert (flips[:, 1] == -1).all() and abs((flips[:, 0] == -1).mean() - 0.25) < 5 * math.sqrt(0.1875 / 4096)
    assert (T < 2 ** 30).all() and T.max() > 2 ** 29


# ---------------------------------------------------------------- the C ABI

def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _good_cfg():
    from ndnet import _lib
    c = _lib.AugConfig()
    c.seed, c.stream, c.yaw_max, c.scale_lo, c.scale_hi = 1, 0, 3.0, 0.9, 1.1
    c.shift_max[0], c.shift_max[1], c.shift_max[2] = 0.5, 0.5, 0.1
    c.drop_max, c.jitter_sigma, c.flip_x_16, c.flip_y_16 = 0.2, 0.01, 0, 32768
    return c


def test_aug_run_rejects_bad_arguments():
    """Every documented NDNET_ERR_ARG, on host memory: nothing is launched and nothing written."""
    import torch
    from ndnet import _lib
    f = _lib.lib().ndnet_aug_run
    E = _lib.NDNET_ERR_ARG
    B, n = 2, 9
    pts, lab, cnt = np.zeros((B, n, 3), np.float32), np.zeros((B, n), np.int32), np.full(B, n, np.int32)
    step = np.full(1, 5, np.uint64)
    work = np.full(_lib.lib().ndnet_aug_work_bytes(B, n) // 4 + 4, 7, np.uint32)
    opts, olab, ocnt = np.full((B, n, 3), 7, np.float32), np.full((B, n), 7, np.int32), np.full(B, 7, np.int32)
    xf = np.full((B, 12), 7, np.float32)

    def call(cfg=None, edit=None):
        c = cfg if cfg is not None else _good_cfg()
        a = [ctypes.byref(c), _p(pts), _p(lab), _p(cnt), B, n, _p(step), _p(work), _p(opts), _p(olab), _p(ocnt),
             _p(xf), None]
        for i, v in (edit or {}).items():
            a[i] = v
        return f(*a)

    for i in (0, 1, 6, 7, 8, 10):  # a NULL cfg, points, step, work, out points or out counts
        assert call(edit={i: None}) == E, i
    assert call(edit={2: None}) == E and call(edit={9: None}) == E  # labels out without in, in without out
    for i, bad in ((4, 0), (4, -1), (4, 65536), (5, 0), (5, 2 ** 31), (5, 2 ** 40)):
        assert call(edit={i: bad}) == E, (i, bad)
    assert call(edit={8: _p(pts)}) == E and call(edit={9: _p(lab)}) == E  # in place while drop_max > 0

    def cfg_with(**kw):
        c = _good_cfg()
        for k, v in kw.items():
            if k.startswith("shift"):
                c.shift_max[int(k[-1])] = v
            else:
                setattr(c, k, v)
        return c

    nan = float("nan")
    bad_cfgs = [dict(scale_lo=0.0), dict(scale_lo=-1.0), dict(scale_lo=nan), dict(scale_lo=1.2), dict(scale_hi=nan),
                dict(drop_max=-0.1), dict(drop_max=1.0001), dict(drop_max=nan),
                dict(yaw_max=-1.0), dict(yaw_max=nan), dict(jitter_sigma=-1e-9), dict(jitter_sigma=nan),
                dict(shift0=-1.0), dict(shift1=nan), dict(shift2=-0.5),
                dict(flip_x_16=65537), dict(flip_y_16=2 ** 32 - 1)]
    for kw in bad_cfgs:
        assert call(cfg=cfg_with(**kw)) == E, kw
    assert step[0] == 5 and (work == 7).all() and (xf == 7).all()
    assert (opts == 7).all() and (olab == 7).all() and (ocnt == 7).all()

    # the unedited block is accepted up to the launch: without a GPU the launch itself fails
    # (NDNET_ERR_HIP); with one, the same block on device memory runs
    if not torch.cuda.is_available():
        assert call() == _lib.NDNET_ERR_HIP
        for kw in (dict(drop_max=0.0), dict(drop_max=1.0), dict(flip_x_16=65536), dict(scale_lo=1.1),
                   dict(yaw_max=0.0, jitter_sigma=0.0, shift0=0.0)):  # the ranges' ends are inside
            assert call(cfg=cfg_with(**kw)) == _lib.NDNET_ERR_HIP, kw
        assert call(cfg=cfg_with(drop_max=0.0), edit={8: _p(pts), 9: _p(lab)}) == _lib.NDNET_ERR_HIP  # in place
    else:
        d = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype != np.float32 else a).cuda()  # noqa: E731
        t = [d(x) for x in (pts, lab, cnt, step, work, opts, olab, ocnt, xf)]
        c = _good_cfg()
        rc = f(ctypes.byref(c), t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), B, n, t[3].data_ptr(),
               t[4].data_ptr(), t[5].data_ptr(), t[6].data_ptr(), t[7].data_ptr(), t[8].data_ptr(),
               torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == _lib.NDNET_OK and t[3].cpu().numpy().view(np.uint64)[0] == 6


def test_work_bytes_grow_with_the_tile_count():
    from ndnet import _lib
    wb = _lib.lib().ndnet_aug_work_bytes
    tile = _tile()
    assert _lib.AUG_TILE == tile
    assert wb(0, 5) == 0 and wb(3, 0) == 0 and wb(3, 2 ** 31) == 0
    B = 3
    assert wb(B, 1) == wb(B, tile) > 0
    for tiles in (1, 2, 5, 1000):
        assert wb(B, tiles * tile + 1) - wb(B, tiles * tile) == 4 * B  # one count more per cloud
        assert wb(B, tiles * tile) == wb(B, (tiles - 1) * tile + 1)
    assert wb(2 * B, 7 * tile) - wb(B, 7 * tile) == B * (48 + 4 + 4 * 7)  # matrix, threshold, counts per cloud


# ---------------------------------------------------------------- the Python class

def test_augment_checks_its_arguments_before_any_gpu_work(monkeypatch):
    from ndnet import _lib
    from ndnet.augment import Augment

    def no_gpu_work():
        raise AssertionError("GPU work before the argument check")

    monkeypatch.setattr(_lib, "require_gpu", no_gpu_work)
    nan = float("nan")
    bad = [dict(yaw=-0.1), dict(yaw=nan), dict(scale=(0.0, 1.0)), dict(scale=(1.1, 1.0)), dict(scale=(nan, 1.0)),
           dict(scale=1.0), dict(scale=(1.0, 1.0, 1.0)), dict(flip=(-0.1, 0.0)), dict(flip=(0.0, 1.5)), dict(flip=0.5),
           dict(shift=(0.0, 0.0)), dict(shift=(0.0, -1.0, 0.0)), dict(shift=(nan, 0.0, 0.0)), dict(jitter=-1.0),
           dict(jitter=nan), dict(drop=-0.01), dict(drop=1.01), dict(drop=nan), dict(seed=-1), dict(seed=2 ** 32),
           dict(seed=1.5), dict(stream=-1), dict(stream=2 ** 32)]
    for kw in bad:
        with pytest.raises(ValueError):
            Augment(**kw)
    a = Augment(yaw=0.5, scale=(0.9, 1.1), flip=(0.25, 1.0), shift=(1, 2, 3), jitter=0.02, drop=1.0, seed=2 ** 32 - 1,
                stream=4)
    c = a.config()
    assert (c.seed, c.stream, c.flip_x_16, c.flip_y_16) == (2 ** 32 - 1, 4, 16384, 65536)
    assert (c.yaw_max, c.scale_lo, c.scale_hi, tuple(c.shift_max), c.drop_max, c.jitter_sigma) == \
        (0.5, 0.9, 1.1, (1.0, 2.0, 3.0), 1.0, 0.02)
    assert Augment().resolve_stream() == 0  # no process group: stream 0
    k = Augment(seed=np.uint32(7), stream=np.int64(2))  # any integer type is a key word; bool and float are not
    assert (k.seed, k.stream) == (7, 2) and type(k.seed) is int
    for kw in (dict(seed=True), dict(stream=np.float32(1.0))):
        with pytest.raises(ValueError):
            Augment(**kw)
    # the state round-trips, the counter with it, without a device
    a.step = 2 ** 32 + 3
    b = Augment()
    b.load_state_dict(a.state_dict())
    assert b.state_dict() == a.state_dict() and b.step == 2 ** 32 + 3
    with pytest.raises(ValueError):
        a.step = 2 ** 62
    with pytest.raises(ValueError):
        b.load_state_dict({**a.state_dict(), "drop": 2.0})
    # the call's own checks come before the GPU too
    import torch
    for pts, lab in ((torch.zeros(4, 3), None), (torch.zeros(2, 4, 2), None),
                     (torch.zeros(2, 4, 3), torch.zeros(2, 4)), (torch.zeros(2, 4, 3), torch.zeros(2, 5, dtype=int))):
        with pytest.raises(ValueError):
            a(pts, lab)
    with pytest.raises(AssertionError):  # valid arguments go on to the GPU work
        a(torch.zeros(2, 4, 3), torch.zeros(2, 4, dtype=torch.int64))


def test_stream_defaults_to_the_rank(monkeypatch):
    import torch
    import torch.distributed as dist
    from ndnet.augment import Augment
    from ndnet.models.ndtnet import NDTNetSegmentation
    from ndnet.training import Trainer
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_rank", lambda *a: 3)
    a, given = Augment(seed=5), Augment(seed=5, stream=7)
    assert a.stream is None
    for aug in (a, given):  # the trainer settles it at construction (ddp=False: no wrapping on the CPU here)
        Trainer(NDTNetSegmentation(3, 5, 64), 1e-3, 8, 5, torch.device("cpu"), ddp=False, augment=aug)
    assert a.stream == 3 and a.config().stream == 3 and given.stream == 7


def test_trainer_checks_augment_before_any_gpu_work():
    import torch
    from ndnet.models.ndtnet import NDTNetSegmentation
    from ndnet.training import Trainer
    with pytest.raises(ValueError, match="augment"):
        Trainer(NDTNetSegmentation(3, 5, 64), 1e-3, 8, 5, torch.device("cpu"), ddp=False, augment="yes")
