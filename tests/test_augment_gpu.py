"""The augmentation kernels (ndnet_aug_run, include/ndnet_augment.h) against the
numpy oracle of aug_ref.py.  The call is defined operation by operation, so
the comparisons are exact: the counts, the kept index set (the labels carry the
points' indices), the labels, the thresholds, the translation, m22, the flips'
signs and the structural zeros equal the oracle's, and the output points equal,
bit for bit, the oracle's float32 chain applied with the kernel's own matrices.

The one allowance: the four trig entries of a matrix are within one float32 ulp
of the float32-rounded float64 oracle value, |got - ref| <= np.spacing(|ref|),
because the device's and the host's double cos / sin may differ in their last
bits, which can move the float32 rounding by one step and no more.

Every output sits between sentinel pads that must come back untouched, and the
rows from counts'[b] on must still hold the sentinel."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import aug_ref as R
from conftest import REPO

pytestmark = pytest.mark.gpu

PAD = 131
SENT_F, SENT_I = -777.25, -7
TRIG, EXACT = (0, 1, 4, 5), (2, 3, 6, 7, 8, 9, 10, 11)


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _tile():
    hdr = open(os.path.join(REPO, "include", "ndnet_augment.h")).read()
    return int(re.search(r"#define NDNET_AUG_TILE (\d+)\n", hdr).group(1))


TILE = _tile()
B3 = 3
SIZES = [1, 7, TILE - 1, TILE, TILE + 1, 3 * TILE + 5]


def _c_config(cfg):
    from ndnet import _lib
    c = _lib.AugConfig()
    c.seed, c.stream, c.yaw_max, c.scale_lo, c.scale_hi = cfg.seed, cfg.stream, cfg.yaw_max, cfg.scale_lo, cfg.scale_hi
    c.shift_max[0], c.shift_max[1], c.shift_max[2] = cfg.shift_max
    c.drop_max, c.jitter_sigma, c.flip_x_16, c.flip_y_16 = cfg.drop_max, cfg.jitter_sigma, cfg.flip_x_16, cfg.flip_y_16
    return c


def _padded(n_words, fill, dtype):
    buf = torch.full((n_words + 2 * PAD,), fill, dtype=dtype, device="cuda")
    return buf, buf[PAD:PAD + n_words]


def _run(cfg, pts, labels, counts, step, in_place=False):
    """ndnet_aug_run at the C ABI: (points' [B, n, 3], labels' [B, n] or None, counts' [B], xform
    [B, 12], T [B], step after) as numpy, every output between sentinel pads that are checked here."""
    from ndnet import _lib
    B, n, _ = pts.shape
    d_pts = torch.from_numpy(pts).cuda()
    d_lab = torch.from_numpy(labels).cuda() if labels is not None else None
    d_cnt = torch.from_numpy(np.asarray(counts, np.int32)).cuda() if counts is not None else None
    d_step = torch.tensor([step], dtype=torch.int64, device="cuda")
    wbytes = _lib.lib().ndnet_aug_work_bytes(B, n)
    assert wbytes % 4 == 0
    bufs = {"points": _padded(B * n * 3, SENT_F, torch.float32), "labels": _padded(B * n, SENT_I, torch.int32),
            "counts": _padded(B, SENT_I, torch.int32), "xform": _padded(B * 12, SENT_F, torch.float32),
            "work": _padded(wbytes // 4 + (-(PAD * 4) % 16) // 4, SENT_I, torch.int32)}
    work = bufs["work"][1]
    work = work[(-work.data_ptr() % 16) // 4:]  # 16-byte aligned
    o_pts, o_lab = bufs["points"][1], bufs["labels"][1]
    if in_place:
        o_pts.copy_(d_pts.reshape(-1))
        d_pts = o_pts
        if d_lab is not None:
            o_lab.copy_(d_lab.reshape(-1))
            d_lab = o_lab
    c = _c_config(cfg)
    rc = _lib.lib().ndnet_aug_run(
        ctypes.byref(c), d_pts.data_ptr(), d_lab.data_ptr() if d_lab is not None else None,
        d_cnt.data_ptr() if d_cnt is not None else None, B, n, d_step.data_ptr(), work.data_ptr(), o_pts.data_ptr(),
        o_lab.data_ptr() if d_lab is not None else None, bufs["counts"][1].data_ptr(), bufs["xform"][1].data_ptr(),
        torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    host = {}
    for name, (buf, _) in bufs.items():
        h = buf.cpu().numpy()
        fill = SENT_F if h.dtype == np.float32 else SENT_I
        assert (h[:PAD] == fill).all() and (h[-PAD:] == fill).all(), f"words outside {name} were written"
        host[name] = h[PAD:-PAD]
    if labels is None:
        assert (host["labels"] == SENT_I).all()
    w = work.cpu().numpy()
    assert int(w[:2].view(np.uint64)[0]) == step  # the snapshot
    T = w[4 + 12 * B:4 + 13 * B].view(np.uint32)
    assert np.array_equal(w[4:4 + 12 * B].view(np.float32).view(np.uint32), host["xform"].view(np.uint32))
    return (host["points"].reshape(B, n, 3), host["labels"].reshape(B, n) if labels is not None else None,
            host["counts"], host["xform"].reshape(B, 12), T, int(d_step.item()))


def _compare(cfg, pts, labels, counts, step, got, tag):
    """The outputs `got` = (points', labels', counts', xform, T or None) against the oracle; returns the
    number of trig entries that differ from the float32-rounded float64 value at all."""
    g_pts, g_lab, g_cnt, g_xf, g_T = got
    B, n, _ = pts.shape
    X, T, flips = R.cloud_params(cfg, B, step)
    if g_T is not None:
        assert np.array_equal(g_T, T), (tag, g_T, T)
    # exact entries bit for bit (the zeros are +0.0f), the trig entries within one ulp, same sign
    assert np.array_equal(g_xf[:, EXACT].view(np.uint32), X[:, EXACT].view(np.uint32)), tag
    assert (g_xf[:, (2, 6, 8, 9)].view(np.uint32) == 0).all(), tag
    gt, rt = g_xf[:, TRIG], X[:, TRIG]
    assert (np.abs(gt.astype(np.float64) - rt.astype(np.float64)) <= np.spacing(np.abs(rt)).astype(np.float64)).all(), \
        (tag, gt, rt)
    nz = rt != 0
    assert np.array_equal(np.signbit(gt[nz]), np.signbit(rt[nz])), tag
    assert np.array_equal(np.sign(gt[:, 0] * gt[:, 3])[nz[:, 0] & nz[:, 3]],
                          (flips[:, 0] * flips[:, 1])[nz[:, 0] & nz[:, 3]]), tag  # m00 m11 = s^2 c^2 fx fy
    # the points through the kernel's own matrices, the kept set, the labels, the counts
    _, _, idx, o_pts, o_lab = R.augment(cfg, pts, labels, counts, step, xform=g_xf)
    for b in range(B):
        mk = len(idx[b])
        assert g_cnt[b] == mk, (tag, b, g_cnt.tolist(), [len(i) for i in idx])
        assert np.array_equal(g_pts[b, :mk].view(np.uint32), o_pts[b].view(np.uint32)), (tag, b)
        assert (g_pts[b, mk:] == np.float32(SENT_F)).all(), (tag, b, "rows past the new count were written")
        if labels is not None:
            assert np.array_equal(g_lab[b, :mk], o_lab[b]), (tag, b)
            assert (g_lab[b, mk:] == SENT_I).all(), (tag, b)
    return int((gt.view(np.uint32) != rt.view(np.uint32)).sum())


def _cfg(drop, seed, **kw):
    d = dict(seed=seed, stream=0, yaw_max=math.pi, scale_lo=0.8, scale_hi=1.25, shift_max=(1.0, 2.0, 0.5),
             drop_max=drop, jitter_sigma=0.05, flip_x_16=32768, flip_y_16=32768)
    d.update(kw)
    return R.Config(**d)


def _batch(n, seed, counts=None, B=B3):
    """Points [B, n, 3] with 1e30 in the padding and labels [B, n] that are the points' own indices."""
    pts = np.random.default_rng(seed).uniform(-40, 40, (B, n, 3)).astype(np.float32)
    labels = np.broadcast_to(np.arange(n, dtype=np.int32), (B, n)).copy()
    if counts is not None:
        for b, c in enumerate(counts):
            pts[b, c:] = 1e30
            labels[b, c:] = -99
    return pts, labels


def _count_mixes(n):
    """None, and rotations of the values of {1, TILE, TILE + 1, n} that fit in n."""
    vals = sorted({1, min(TILE, n), min(TILE + 1, n), n})
    return [None] + [[vals[(k + b) % len(vals)] for b in range(B3)] for k in range(len(vals))]


@pytest.mark.parametrize("drop", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("n", SIZES)
def test_against_the_oracle(n, drop):
    differ = total = 0
    for k, counts in enumerate(_count_mixes(n)):
        for with_labels in (True, False):
            step = 3 + k
            cfg = _cfg(drop, seed=100 * n + k)
            pts, labels = _batch(n, n + k, counts)
            labels = labels if with_labels else None
            *got, after = _run(cfg, pts, labels, counts, step)
            assert after == step + 1
            differ += _compare(cfg, pts, labels, counts, step, got, (n, drop, counts, with_labels))
            total += 4 * B3
            kept, m = got[2], np.array(counts if counts is not None else [n] * B3)
            assert (kept >= 1).all() and (kept <= m).all()
            if drop == 0.0:
                assert np.array_equal(kept, m)
    print(f"TRIG n {n} drop {drop}: {differ} of {total} trig entries differ from the rounded float64 value")


def test_dropout_thins_and_point_zero_survives():
    """drop_max = 1 over many clouds: thresholds spread over the whole range, the kept share follows them,
    and a cloud whose threshold keeps nothing else still keeps point 0."""
    B, n = 64, 2 * TILE + 3
    cfg = _cfg(1.0, seed=9, jitter_sigma=0.0)
    pts, labels = _batch(n, 5, B=B)
    *got, _ = _run(cfg, pts, labels, None, 0)
    _compare(cfg, pts, labels, None, 0, got, "thin")
    kept, T = got[2].astype(np.float64), got[4].astype(np.float64)
    assert (got[1][:, 0] == 0).all()  # point 0 first in every cloud
    assert T.min() < 2 ** 32 * 0.1 and T.max() > 2 ** 32 * 0.9
    expect = 1 + (n - 1) * (1 - T / 2 ** 32)
    assert (np.abs(kept - expect) <= 6 * np.sqrt(n / 4) + 1).all()


def test_in_place_without_dropout_and_identity():
    n = 2 * TILE + 9
    counts = [n, TILE + 1, 1]
    pts, labels = _batch(n, 21, counts)
    cfg = _cfg(0.0, seed=4)
    *got, _ = _run(cfg, pts, labels, counts, 8, in_place=True)
    # in place the rows past a count keep the input, not the sentinel: compare the existing rows only
    _, _, idx, o_pts, o_lab = R.augment(cfg, pts, labels, counts, 8, xform=got[3])
    for b, c in enumerate(counts):
        assert got[2][b] == c
        assert np.array_equal(got[0][b, :c].view(np.uint32), o_pts[b].view(np.uint32))
        assert np.array_equal(got[0][b, c:], pts[b, c:]) and np.array_equal(got[1][b], labels[b])
    # the identity configuration returns the existing rows bit for bit (the input holds no -0.0)
    ident = R.Config(seed=77)
    *got, _ = _run(ident, pts, labels, counts, 2 ** 33)
    for b, c in enumerate(counts):
        assert np.array_equal(got[0][b, :c].view(np.uint32), pts[b, :c].view(np.uint32))
        assert np.array_equal(got[1][b, :c], labels[b, :c]) and got[2][b] == c


# ---------------------------------------------------------------- the step counter, graphs, streams

def _aug(stream=0, seed=5, drop=0.4):
    from ndnet.augment import Augment
    return Augment(yaw=math.pi, scale=(0.9, 1.1), flip=(0.5, 0.5), shift=(0.5, 0.5, 0.1), jitter=0.02, drop=drop,
                   seed=seed, stream=stream)


def _call(A, d_pts, d_lab, d_cnt):
    p, l_, c = A(d_pts, d_lab, d_cnt)
    torch.cuda.synchronize()
    return p.cpu().numpy(), l_.cpu().numpy(), c.cpu().numpy(), A.xform.cpu().numpy()


def _compare_class(A, pts, labels, counts, step, out, tag):
    """Augment's outputs (fresh tensors: no sentinel past the counts) against the oracle."""
    cfg = R.Config.of(A)
    g_pts, g_lab, g_cnt, g_xf = out
    _, T, idx, o_pts, o_lab = R.augment(cfg, pts, labels, counts, step, xform=g_xf)
    X, _, _ = R.cloud_params(cfg, pts.shape[0], step)
    assert np.array_equal(g_xf[:, EXACT].view(np.uint32), X[:, EXACT].view(np.uint32)), tag
    assert (np.abs(g_xf[:, TRIG].astype(np.float64) - X[:, TRIG]) <= np.spacing(np.abs(X[:, TRIG]))).all(), tag
    for b in range(pts.shape[0]):
        mk = len(idx[b])
        assert g_cnt[b] == mk, (tag, b)
        assert np.array_equal(g_pts[b, :mk].view(np.uint32), o_pts[b].view(np.uint32)), (tag, b)
        assert np.array_equal(g_lab[b, :mk], o_lab[b]), (tag, b)


def test_two_eager_calls_use_consecutive_steps():
    n, counts = TILE + 77, [TILE + 77, 500, TILE + 1]
    pts, labels = _batch(n, 3, counts)
    d = (torch.from_numpy(pts).cuda(), torch.from_numpy(labels).cuda(), torch.tensor(counts, device="cuda"))
    A = _aug()
    A.step = 41
    first, second = _call(A, *d), _call(A, *d)
    assert A.step == 43
    _compare_class(A, pts, labels, counts, 41, first, "first")
    _compare_class(A, pts, labels, counts, 42, second, "second")
    assert not np.array_equal(first[3], second[3]) and first[2].tolist() != second[2].tolist()
    assert first[2].dtype == np.int32
    # int64 ids and list counts are converted; without labels the middle result is None
    p, l_, c = A(d[0], None, counts)
    assert l_ is None and c.dtype == torch.int32 and c.is_cuda and A.step == 44
    # a resumed augmentation repeats the draws
    from ndnet.augment import Augment
    A2 = Augment()
    state = A.state_dict()
    state["step"] = 42
    A2.load_state_dict(state)
    again = _call(A2, d[0], d[1].long(), d[2])
    for a, b in zip(again, second):
        m = [slice(0, int(k)) for k in second[2]]
        if a.ndim >= 2 and a.shape[:2] == pts.shape[:2]:
            assert all(np.array_equal(a[i, s], b[i, s]) for i, s in enumerate(m))
        else:
            assert np.array_equal(a, b)


def test_a_captured_call_draws_anew_on_every_replay_across_the_high_word():
    n, counts = 2 * TILE + 5, [2 * TILE + 5, TILE, 9]
    pts, labels = _batch(n, 13, counts)
    d = (torch.from_numpy(pts).cuda(), torch.from_numpy(labels).cuda(), torch.tensor(counts, device="cuda",
                                                                                     dtype=torch.int32))
    A = _aug(seed=8)
    _call(A, *d)  # (the kernels are loaded and the work buffer exists before the capture)
    s = 2 ** 32 - 1
    A.step = s
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        o_p, o_l, o_c = A(*d)
    xf = A.xform
    assert A.step == s  # capturing runs nothing
    seen = []
    for r in range(3):
        g.replay()
        torch.cuda.synchronize()
        out = (o_p.cpu().numpy(), o_l.cpu().numpy(), o_c.cpu().numpy(), xf.cpu().numpy())
        _compare_class(A, pts, labels, counts, s + r, out, ("replay", r))
        seen.append(out[3])
    assert A.step == s + 3 == 2 ** 32 + 2
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])


def test_streams_are_independent_and_reproducible():
    n = TILE + 3
    pts, labels = _batch(n, 17)
    d = (torch.from_numpy(pts).cuda(), torch.from_numpy(labels).cuda(), None)
    outs = {}
    for name, stream in (("a", 0), ("b", 1), ("a2", 0)):
        A = _aug(stream=stream)
        outs[name] = _call(A, *d)
        _compare_class(A, pts, labels, None, 0, outs[name], name)
    for x, y in zip(outs["a"], outs["a2"]):
        k = outs["a"][2]
        if x.ndim >= 2 and x.shape[:2] == pts.shape[:2]:
            assert all(np.array_equal(x[b, :k[b]], y[b, :k[b]]) for b in range(B3))
        else:
            assert np.array_equal(x, y)
    assert not np.array_equal(outs["a"][3], outs["b"][3])
    assert not np.array_equal(outs["a"][1][:, :64], outs["b"][1][:, :64])  # another kept set
