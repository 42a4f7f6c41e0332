"""Packed int16 point input, the host side (no GPU): ``pack_points`` against
the oracle's transcription of the rules, the round-trip error bound, every
``ValueError``, the C entry point's argument checks on host memory,
``collate_packed``, and the pipeline's checks that run before any GPU work."""
import ctypes
import math

import numpy as np
import pytest

import packed_ref as R


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _clouds(seed, B=3, n=257, dtype=np.float64):
    """Random clouds at scales 1e-2 .. 1e3 and offsets up to 1e3."""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.uniform(-2, 3, (B, 1, 1))
    aspect = rng.uniform(0.05, 1.0, (B, 1, 3))
    offset = rng.uniform(-1e3, 1e3, (B, 1, 3))
    return (rng.uniform(-1, 1, (B, n, 3)) * scale * aspect + offset).astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_pack_points_equals_the_transcription(dtype):
    import torch
    from ndnet.packed import pack_points
    for seed in range(8):
        x = _clouds(seed, dtype=dtype)
        q, qp = pack_points(x)
        assert q.dtype == torch.int16 and qp.dtype == torch.float32 and not q.is_cuda
        rq, rqp = R.pack(x)
        assert np.array_equal(q.numpy(), rq) and np.array_equal(qp.numpy(), rqp), seed
        assert int(q.min()) >= -32767 and int(q.max()) <= 32767  # the default step reaches the box, no further
        assert int(q.abs().max()) >= 32766                       # ... and is the smallest that does
        # a tensor in: the same
        q2, qp2 = pack_points(torch.from_numpy(x))
        assert torch.equal(q, q2) and torch.equal(qp, qp2)
    # a given step, scalar and per cloud
    x = _clouds(3, dtype=dtype)
    big = R.pack(x)[1][:, 3] * np.float32(1.7)
    for step in (float(big.max()), big):
        q, qp = pack_points(x, step=step)
        rq, rqp = R.pack(x, step=step)
        assert np.array_equal(q.numpy(), rq) and np.array_equal(qp.numpy(), rqp)
        assert np.array_equal(qp.numpy()[:, 3], np.broadcast_to(np.asarray(step, np.float32), (3,)))


def test_default_step_is_the_smallest_float32():
    from ndnet.packed import _default_step
    rng = np.random.default_rng(5)
    for half in list(10.0 ** rng.uniform(-6, 6, 200)) + [32767.0, 1.0, 0.5 * 32767, 3.0e-3 * 32767]:
        s = _default_step(float(half))
        assert s.dtype == np.float32 and s == R.default_step(float(half))
        assert float(s) * 32767 >= half > float(np.nextafter(s, np.float32(0))) * 32767
    assert _default_step(0.0) == np.float32(1.0)


def test_zero_extent_padding_and_counts():
    from ndnet.packed import pack_points
    x = _clouds(11, B=3, n=40)
    x[1] = x[1, 0]                   # a cloud of zero extent: step 1, every q 0
    counts = [40, 17, 1]             # ... and one of a single point
    x[2, 1:] = np.nan                # the padding is never read
    q, qp = pack_points(x, counts)
    rq, rqp = R.pack(x, counts)
    assert np.array_equal(q.numpy(), rq) and np.array_equal(qp.numpy(), rqp)
    assert qp[1, 3] == 1 and qp[2, 3] == 1 and not q[1].any() and not q[2].any()
    assert np.array_equal(qp.numpy()[1, :3], x[1, 0].astype(np.float32))
    x[0, 30:] = 1e30                 # padding again: it must not widen the box
    q2, qp2 = pack_points(x, [30, 17, 1])
    assert not q2[0, 30:].any() and q2[0, :30].any()
    assert np.array_equal(q2.numpy()[0], R.pack(x[:1], [30])[0][0])


def test_pack_points_value_errors():
    import torch
    from ndnet.packed import pack_points
    x = _clouds(2, B=3, n=20)
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[1, 7, 2] = bad
        with pytest.raises(ValueError, match="cloud 1"):
            pack_points(y)
        pack_points(y, [20, 7, 20])  # ... unless that point is padding
    for step in (0.0, -0.01, np.nan, np.inf, [0.01, 0.0, 0.01], [0.01, np.nan, 0.01], 1e-50):
        with pytest.raises(ValueError, match="step"):
            pack_points(x, step=step)
    with pytest.raises(ValueError, match="step"):
        pack_points(x, step=[0.01, 0.01])  # one per cloud
    # a step too small for one cloud only: never clamped, the cloud is named
    steps = R.pack(x)[1][:, 3].astype(np.float64)
    steps[2] *= 0.9
    with pytest.raises(ValueError, match="cloud 2.*too small"):
        pack_points(x, step=steps)
    with pytest.raises(OverflowError):
        R.pack(x, step=steps)
    for shape in ((20, 3), (3, 20, 2), (3, 20, 4), (0, 20, 3), (3, 0, 3), (1, 3, 20, 3)):
        with pytest.raises(ValueError, match="shape"):
            pack_points(np.zeros(shape))
    with pytest.raises(ValueError, match="float32 or float64"):
        pack_points(np.zeros((1, 4, 3), np.int32))
    for counts in ([20, 21, 20], [20, 0, 20], [-1, 20, 20]):
        with pytest.raises(ValueError, match="count"):
            pack_points(x, counts)
    with pytest.raises(ValueError, match="shape"):
        pack_points(x, [20, 20])
    with pytest.raises(ValueError, match="shape"):
        pack_points(x, torch.tensor([[20, 20, 20]]))


def test_round_trip_error_bound():
    """|decode - x| <= step / 2 + 2^-24 (|x - o| + |x| + |decode|): half a step
    of quantisation, and the roundings of q * step (at most |x - o| + step / 2
    in size), of the sum and of x's own distance to the float32 origin."""
    from ndnet.packed import pack_points
    worst = 0.0
    for seed in range(200):
        x = _clouds(100 + seed, B=1, n=64)
        q, qp = pack_points(x)
        q, qp = q.numpy(), qp.numpy()
        assert int(np.abs(q.astype(np.int32)).max()) <= 32767  # nothing clamped
        d = R.decode(q, qp).astype(np.float64)
        o, step = qp[:, None, :3].astype(np.float64), float(qp[0, 3])
        bound = step / 2 + 2.0 ** -24 * (np.abs(x - o) + np.abs(x) + np.abs(d))
        ratio = float((np.abs(d - x) / bound).max())
        assert ratio <= 1.0, (seed, ratio)
        worst = max(worst, ratio)
    assert worst > 0.9  # the bound is not slack: half a step is reached


def test_fused_form_differs_on_the_tests_inputs():
    """The precondition of the kernel tests: on their inputs an fma-form decode
    differs from the oracle on >= 1% of the elements (so an fma in the kernel
    cannot pass), while a power-of-two step or a zero origin hides it."""
    for B, n in ((1, 33), (3, 33), (3, 1025), (3, 20_003)):
        for seed in (0, 1):
            q, qp = R.kernel_case(B, n, seed)
            assert not any(math.log2(float(s)).is_integer() for s in qp[:, 3]) and (qp[:, :3] != 0).all()
            assert (qp[:, :3] < 0).all(axis=1).any()  # one cloud's origin is negative on every axis
            flat = q.reshape(B, -1)
            if 3 * n >= 3:
                assert all((flat[b] == v).any() for b in range(B) for v in (-32768, 32767, 0))
            prod = np.abs(q.astype(np.float64) * qp[:, None, 3:4])
            assert ((prod == 0) | (prod >= 1e-30)).all()
            a, f = R.decode(q, qp), R.decode_fused(q, qp)
            for b in range(B):
                assert (a[b] != f[b]).mean() >= 0.01, (B, n, seed, b)
    q, qp = R.kernel_case(3, 1025)
    pow2, zero = qp.copy(), qp.copy()
    pow2[:, 3] = 2.0 ** -8
    zero[:, :3] = 0
    assert np.array_equal(R.decode(q, pow2), R.decode_fused(q, pow2))
    assert np.array_equal(R.decode(q, zero), R.decode_fused(q, zero))


def test_entry_point_rejects_bad_arguments():
    from ndnet import _lib
    f = _lib.lib().ndnet_pts_unpack_i16
    E = _lib.NDNET_ERR_ARG
    q, qp = R.kernel_case(2, 5)
    out, counts = np.full((2, 5, 3), 7.5, np.float32), np.array([5, 5], np.int32)
    good = [_p(q), _p(qp), 2, 5, _p(counts), _p(out), None]
    for i in (0, 1, 5):  # a NULL pointer (NULL counts are valid)
        a = list(good)
        a[i] = None
        assert f(*a) == E, i
    for i, bad in ((2, 0), (2, -1), (2, 65536), (3, 0), (3, 1 << 31), (3, (1 << 31) + 5), (3, 1 << 40), (3, (1 << 64) - 1)):
        for c in (_p(counts), None):
            a = list(good)
            a[i], a[4] = bad, c
            assert f(*a) == E, (i, bad)
    assert (out == 7.5).all()


def test_collate_packed_is_collate_padded_then_pack_points():
    import functools
    import torch
    from ndnet.datasets import collate_packed, collate_padded
    from ndnet.packed import pack_points
    rng = np.random.default_rng(9)
    scans = []
    for m in (50, 31, 64, 1):
        pts = torch.from_numpy((rng.normal(size=(m, 3)) * 20 + (5, -80, 1)).astype(np.float32))
        scans.append((pts, torch.from_numpy(rng.integers(0, 6, m))))
    points, classes, counts = collate_padded(scans)
    for step in (None, 0.01):
        fn = collate_packed if step is None else functools.partial(collate_packed, step=step)
        q, cl, cn, qp = fn(scans)
        eq, eqp = pack_points(points, counts, step)
        assert torch.equal(q, eq) and torch.equal(qp, eqp) and torch.equal(cl, classes) and torch.equal(cn, counts)
        assert q.dtype == torch.int16 and q.shape == points.shape and qp.shape == (4, 4) and cn.dtype == torch.int32
        assert q.element_size() * q.numel() * 2 == points.element_size() * points.numel()
    # the decoded batch is the scans to within half a step
    d = R.decode(q.numpy(), qp.numpy())
    for b, (pts, _) in enumerate(scans):
        assert np.abs(d[b, :len(pts)] - pts.numpy()).max() <= 0.01 / 2 + 1e-4


@pytest.fixture
def no_gpu(monkeypatch):
    from ndnet import _lib

    def no_gpu_work():
        raise AssertionError("GPU work before the argument check")

    monkeypatch.setattr(_lib, "require_gpu", no_gpu_work)


def test_unpack_arguments_are_checked_first(no_gpu):
    import torch
    from ndnet.packed import unpack
    q, qp = (torch.from_numpy(t) for t in R.kernel_case(2, 9))
    for bad_q in (q.to(torch.int32), q.float(), q[0], q[..., :2], q.numpy()):
        with pytest.raises(ValueError, match="int16"):
            unpack(bad_q, qp)
    for bad_qp in (qp.double(), qp[:1], qp[:, :3], qp.reshape(-1), None):
        with pytest.raises(ValueError, match="qparams"):
            unpack(q, bad_qp)
    for counts in ([9, 10], [0, 9], [9, -1]):
        with pytest.raises(ValueError, match="count"):
            unpack(q, qp, counts)
    with pytest.raises(ValueError, match="shape"):
        unpack(q, qp, [9, 9, 9])
    for bad_out in (torch.zeros((2, 9, 3), dtype=torch.float64), torch.zeros((2, 8, 3)), torch.zeros((2, 3, 9)).mT):
        with pytest.raises(ValueError, match="out"):
            unpack(q, qp, out=bad_out)
    for kw in (dict(), dict(counts=[9, 1]), dict(out=torch.zeros((2, 9, 3))), dict(counts=torch.tensor([3, 4]))):
        with pytest.raises(AssertionError, match="GPU work"):  # valid arguments go on to the GPU work
            unpack(q, qp, **kw)


def test_pipeline_packed_arguments_are_checked_first(no_gpu):
    import torch
    from ndnet import pipeline
    from ndnet.models.ndtnet import NDTNetSegmentation
    seg = NDTNetSegmentation(3, 5, 64).eval()
    for cls in (pipeline.PipelinedSegmentation, pipeline.GraphedSegmentation):
        for bad in (1, 0, None, "yes"):
            with pytest.raises(ValueError, match="packed"):
                cls(seg, 8, 1, 64, packed=bad)
        for kw in (dict(packed=True), dict(packed=True, ragged=True, point_labels="nearest"),
                   dict(packed=True, levels=(8, 4)), dict(packed=False)):
            with pytest.raises(AssertionError, match="GPU work"):  # valid arguments go on to the GPU work
                cls(seg, 8, 1, 64, **kw)
    with pytest.raises(AssertionError, match="GPU work"):
        pipeline.PipelinedSegmentation(seg, 8, 1, 64, packed=True, point_labels="none", label_dtype=torch.uint8)


def test_packed_input_checks_touch_nothing_else():
    """``replay_streamed``, ``load_resident`` and the graph's ``__call__`` check
    the packed input first: on an object that holds nothing but the input
    buffers, so any other work -- a replay, a copy, a stream -- would raise
    ``AttributeError`` instead."""
    import torch
    from ndnet import pipeline
    B, n = 2, 8
    q, qp = (torch.from_numpy(t) for t in R.kernel_case(B, n))
    pipe = object.__new__(pipeline.PipelinedSegmentation)
    pipe.packed, pipe.inputs = True, [torch.zeros((B, n, 3), dtype=torch.int16)]
    graph = object.__new__(pipeline.GraphedSegmentation)
    graph.packed, graph.points = True, pipe.inputs[0]
    calls = (lambda p, qparams: pipe.replay_streamed(p, qparams_next=qparams),
             lambda p, qparams: pipe.replay_streamed(p, None, None, qparams),
             lambda p, qparams: pipe.load_resident(p, qparams=qparams),
             lambda p, qparams: graph(p, qparams=qparams))
    for call in calls:
        with pytest.raises(ValueError, match="int16"):
            call(torch.zeros((B, n, 3)), qp)
        with pytest.raises(ValueError, match="int16"):
            call(torch.zeros((B, n, 3)), None)
        with pytest.raises(ValueError, match="qparams"):
            call(q, None)
        for bad in (qp.double(), qp[:1], qp[:, :3]):
            with pytest.raises(ValueError, match="qparams"):
                call(q, bad)
        with pytest.raises(AttributeError):  # valid: on to the work
            call(q, qp)
    pipe.packed = graph.packed = False
    pipe.inputs = [torch.zeros((B, n, 3))]
    for call in calls:
        with pytest.raises(ValueError, match="packed=True"):
            call(torch.zeros((B, n, 3)), qp)


def test_ring_order_keeps_packed_inputs_and_decoded_buffers_apart():
    """The vector-clock replay of the pipeline's event order
    (test_pipeline_labels_cpu._Sim) with the packed buffers added: qparams j is
    read inside slot j's NDT stage and replaced by the streamed copy, decoded
    buffer j % N is written and read inside that stage alone."""
    import itertools
    from test_pipeline_labels_cpu import _Sim

    class Sim(_Sim):
        def op(self, s, reads=(), writes=()):
            j = self.i % self.R
            if s.startswith("ndt"):
                reads = list(reads) + [("qparams", j)]
                writes = list(writes) + [("decoded", j % self.N)]
            elif s == "copy":
                writes = list(writes) + [("qparams", (self.i) % self.R)]  # streamed(): i is already the next step
            super().op(s, reads, writes)
            if s.startswith("ndt"):
                super().op(s, reads=[("decoded", j % self.N)])  # the run, the prune levels, k_point_rows

    for F, N in ((1, 1), (3, 1), (3, 2), (2, 2), (4, 3)):
        sim = Sim(F, N)
        for _ in range(4 * sim.R):
            sim.enqueue()
        for labels in itertools.islice(itertools.cycle((True, False)), 4 * sim.R):
            sim.streamed(labels)
        assert ("decoded", 0) in sim.last_write and ("qparams", 0) in sim.last_write
