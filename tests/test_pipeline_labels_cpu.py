"""The pipeline's label and ragged arguments, ``segment.point_labels``' uint8
form and the C entry point behind it reject misuse before any GPU work (CPU:
the arguments are host memory, ``require_gpu`` is never reached), and the
pipeline's event order keeps every ring buffer of the labelled path apart."""
import ctypes
import itertools
import math

import numpy as np
import pytest


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_seg_point_labels_u8_rejects_bad_arguments():
    from ndnet import _lib
    f = _lib.lib().ndnet_seg_point_labels_u8
    E = _lib.NDNET_ERR_ARG
    scores, rows = np.zeros((2, 4, 3), np.float32), np.zeros((2, 5), np.int32)
    nd, pl = np.full((2, 4), 7, np.int32), np.full((2, 5), 7, np.uint8)
    good = [_p(scores), _p(rows), 2, 5, 4, 3, 255, _p(nd), _p(pl), None]
    for i in (0, 1, 7, 8):  # a NULL pointer
        a = list(good)
        a[i] = None
        assert f(*a) == E, i
    for i, bad in ((2, 0), (2, -1), (3, 0), (4, 0), (5, 0), (5, -3)):  # B, n, k, cols < 1
        a = list(good)
        a[i] = bad
        assert f(*a) == E, (i, bad)
    for cols, un in ((256, 255), (300, 255), (3, 2), (3, 0), (255, 254)):  # no byte / the marker is a class
        a = list(good)
        a[5], a[6] = cols, un
        assert f(*a) == E, (cols, un)
    a = list(good)
    a[2] = 65536  # the grid's y limit, as the int32 entry
    assert f(*a) == E
    assert (nd == 7).all() and (pl == 7).all()


@pytest.fixture
def no_gpu(monkeypatch):
    from ndnet import _lib

    def no_gpu_work():
        raise AssertionError("GPU work before the argument check")

    monkeypatch.setattr(_lib, "require_gpu", no_gpu_work)


def test_point_labels_uint8_arguments_are_checked_first(no_gpu):
    import torch
    from ndnet import segment
    rows = torch.zeros((1, 8), dtype=torch.int32)
    wide, six = torch.zeros((1, 4, 256)), torch.zeros((1, 4, 6))
    with pytest.raises(ValueError, match="255 columns"):
        segment.point_labels(wide, rows, dtype=torch.uint8)
    with pytest.raises(ValueError, match="255 columns"):  # the dtype comes from out
        segment.point_labels(wide, rows, out=torch.zeros((1, 8), dtype=torch.uint8))
    for bad in (5, 0, -1, 256):
        with pytest.raises(ValueError, match="unassigned"):
            segment.point_labels(six, rows, unassigned=bad, dtype=torch.uint8)
    with pytest.raises(ValueError, match="int32 or uint8"):
        segment.point_labels(six, rows, dtype=torch.int64)
    for kw in (dict(dtype=torch.uint8), dict(unassigned=6, dtype=torch.uint8), dict(), dict(unassigned=-7),
               dict(out=torch.zeros((1, 8), dtype=torch.uint8))):
        with pytest.raises(AssertionError, match="GPU work"):  # valid arguments go on to the GPU work
            segment.point_labels(six, rows, **kw)
    with pytest.raises(AssertionError, match="GPU work"):  # 256 columns are fine as int32
        segment.point_labels(wide, rows)


def test_pipelined_arguments_are_checked_first(no_gpu):
    import torch
    from ndnet import pipeline
    from ndnet.models.ndtnet import NDTNetClassification, NDTNetSegmentation
    P = pipeline.PipelinedSegmentation
    seg = NDTNetSegmentation(3, 5, 64).eval()
    cls = NDTNetClassification(3, 5, 64).eval()
    with pytest.raises(ValueError, match="NDTNetSegmentation"):
        P(cls, 8, 1, 64, point_labels="nearest")
    with pytest.raises(ValueError, match="levels"):
        P(seg, 8, 1, 64, levels=(8, 4), point_labels="none")
    with pytest.raises(ValueError, match="point_labels"):
        P(seg, 8, 1, 64, point_labels="mean")
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="ragged"):
            P(seg, 8, 1, 64, ragged=bad)
    for bad in (torch.int64, torch.int8, torch.float32, None):
        with pytest.raises(ValueError, match="label_dtype"):
            P(seg, 8, 1, 64, point_labels="none", label_dtype=bad)
    with pytest.raises(ValueError, match="255"):  # 255 columns and the marker do not fit a byte
        P(NDTNetSegmentation(3, 255, 64).eval(), 8, 1, 64, point_labels="none", label_dtype=torch.uint8)
    for kw in (dict(point_labels="nearest"), dict(point_labels="none", ragged=True, label_dtype=torch.uint8),
               dict(ragged=True, levels=(8, 4)), dict()):
        with pytest.raises(AssertionError, match="GPU work"):  # valid arguments go on to the GPU work
            P(seg, 8, 1, 64, **kw)
    with pytest.raises(AssertionError, match="GPU work"):  # 254 classes: 255 columns, marker 255
        P(NDTNetSegmentation(3, 254, 64).eval(), 8, 1, 64, point_labels="none", label_dtype=torch.uint8)


class _Sim:
    """The pipeline's ``_enqueue`` and ``replay_streamed`` event order replayed
    on vector clocks: every stream is a sequence of operations, an event holds
    the clock of its stream at the record, a wait merges it in.  Operation a
    happens before b iff a's own tick is in b's clock."""

    def __init__(self, F, N, ndt_waits_fwd=True):
        self.ndt_waits_fwd = ndt_waits_fwd
        lcm = F * N // math.gcd(F, N)
        self.F, self.N, self.R = F, N, -(-(F + N + 1) // lcm) * lcm
        self.streams = [f"fwd{t}" for t in range(F)] + [f"ndt{t}" for t in range(N)] + ["copy", "out"]
        self.clock = {s: {} for s in self.streams}
        self.tick = {s: 0 for s in self.streams}
        self.events = {}
        self.last_write, self.reads = {}, {}
        self.i = 0

    def wait(self, s, ev):
        for k, v in self.events.get(ev, {}).items():
            self.clock[s][k] = max(self.clock[s].get(k, 0), v)

    def record(self, s, ev):
        self.events[ev] = dict(self.clock[s])

    def op(self, s, reads=(), writes=()):
        self.tick[s] += 1
        self.clock[s][s] = self.tick[s]
        me = (s, self.tick[s])
        seen = lambda other: self.clock[s].get(other[0], 0) >= other[1]
        for buf in reads:
            w = self.last_write.get(buf)
            assert w is None or seen(w), f"step {self.i}: {s} reads {buf} unordered after its write by {w}"
            self.reads.setdefault(buf, []).append(me)
        for buf in writes:
            w = self.last_write.get(buf)
            assert w is None or seen(w), f"step {self.i}: {s} writes {buf} unordered after its write by {w}"
            for r in self.reads.pop(buf, []):
                assert seen(r), f"step {self.i}: {s} overwrites {buf} before its read by {r}"
            self.last_write[buf] = me

    def enqueue(self):
        R, j = self.R, self.i % self.R
        p = (j - 1) % R
        sf, sn = f"fwd{j % self.F}", f"ndt{j % self.N}"
        self.wait(sf, ("ndt_done", p))
        self.wait(sf, ("labels_out", j))
        self.op(sf, reads=[("rows", p), ("point_rows", p)], writes=[("out", j), ("labels", j), ("ws", j % self.F)])
        self.record(sf, ("fwd_done", j))
        if self.ndt_waits_fwd:
            self.wait(sn, ("fwd_done", (j + 1) % R))
        self.wait(sn, ("copied", j))
        self.op(sn, reads=[("input", j), ("counts", j)],
                writes=[("rows", j), ("point_rows", j), ("plan", j % self.N)])
        self.record(sn, ("ndt_done", j))
        self.i += 1
        return j

    def streamed(self, labels: bool):
        nxt = (self.i + 1) % self.R
        j = self.enqueue()
        self.wait("copy", ("ndt_done", nxt))
        self.op("copy", writes=[("input", nxt), ("counts", nxt)])
        self.record("copy", ("copied", nxt))
        if labels:
            self.wait("out", ("fwd_done", j))
            self.op("out", reads=[("labels", j)])
            self.record("out", ("labels_out", j))


@pytest.mark.parametrize("F,N", [(1, 1), (2, 1), (3, 1), (3, 2), (2, 2), (1, 2), (4, 3)])
def test_ring_order_keeps_rows_labels_and_counts_apart(F, N):
    """Free-running (no joins: the weakest order the pipeline runs under): the
    points' rows of slot j are read by the next step's forward alone before
    the NDT stage of step i + R overwrites them, the counts and inputs are
    read inside the NDT stage before a streamed copy replaces them, and the
    labels are copied out before the forward of step i + R overwrites them --
    for the default (3, 1), the tests' (1, 1) and (3, 2), and more."""
    sim = _Sim(F, N)
    for _ in range(4 * sim.R):
        sim.enqueue()
    for labels in itertools.islice(itertools.cycle((True, True, False)), 4 * sim.R):
        sim.streamed(labels)
    # the simulation does catch a missing wait: without the NDT stage's wait on
    # fwd_done[(j + 1) % R] the rows are overwritten under their reader
    broken = _Sim(F, N, ndt_waits_fwd=False)
    with pytest.raises(AssertionError, match="overwrites"):
        for _ in range(4 * broken.R):
            broken.enqueue()
