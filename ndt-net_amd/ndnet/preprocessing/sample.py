"""An exact-size random subsample of every cloud on the GPU, and the gather of
points and labels by given indices.

The reference trains its PointNet baseline on ``n_samples`` points of every
scan chosen by ``np.random.choice(..., replace=False)`` on the host.
``RandomSample`` is that cut on the GPU (``ndnet_sample_random_run``,
include/ndnet_sample.h, which defines it): every existing point of a cloud
draws a 32-bit Philox key, the ``n_samples`` smallest keys are chosen (ties go
to the smaller index) and the chosen points leave in input order with their
labels.  It takes a ragged batch (``counts``), runs after the augmentation,
needs no host round trip and so lives inside a captured step.  The random
state is a step counter in device memory that every call (and every replay of
a captured call) advances; the draw is a pure function of ``(seed, stream,
step, cloud, point)`` and independent of an ``Augment`` with the same seed.

    sampler = RandomSample(4160, seed=1)
    pts, ids, sample_counts, idx = sampler(points.cuda(), ids.cuda(), counts)

A cloud shorter than ``n_samples`` is taken whole; its remaining rows repeat
point 0 with ``fill_label`` and index -1, and ``sample_counts`` says how many
rows are real.  ``gather_samples`` is the last pass alone, for indices from
``farthest_point_sample``.
"""
from __future__ import annotations

import ctypes
import operator
from typing import Optional, Tuple

import torch

from .. import _lib


def _key_word(v, what: str) -> int:
    """A 32-bit word of the Philox key: any integer type, but no bool and no float."""
    try:
        i = None if isinstance(v, bool) else operator.index(v)
    except TypeError:
        i = None
    if i is None or not 0 <= i < 1 << 32:
        raise ValueError(f"{what} must be an integer in 0 .. 2^32 - 1, got {v!r}")
    return i


def _check_points(points, what: str = "points") -> Tuple[int, int]:
    if not isinstance(points, torch.Tensor) or points.dim() != 3 or points.shape[-1] != 3:
        raise ValueError(f"{what} must be a [B, n, 3] tensor, got {tuple(getattr(points, 'shape', ()))}")
    if points.dtype != torch.float32:
        raise ValueError(f"{what} must be float32, got {points.dtype}")
    B, n, _ = points.shape
    if B < 1 or n < 1:
        raise ValueError(f"{what} must hold at least one cloud and one point, got {tuple(points.shape)}")
    return B, n


def _check_labels(labels, B: int, n: int) -> None:
    if labels is None:
        return
    if (not isinstance(labels, torch.Tensor) or labels.is_floating_point() or labels.dtype == torch.bool
            or tuple(labels.shape) != (B, n)):
        raise ValueError(f"labels must be integer class ids of shape {(B, n)}, got "
                         f"{getattr(labels, 'dtype', type(labels).__name__)} {tuple(getattr(labels, 'shape', ()))}")


def _check_counts(counts, B: int, n: int) -> None:
    """Shape ``[B]``; the values of a sequence or a CPU tensor in ``1 .. n``
    (a device tensor is not read: that would synchronise)."""
    if counts is None:
        return
    on_device = isinstance(counts, torch.Tensor) and counts.is_cuda
    t = counts if on_device else torch.as_tensor(counts)
    if tuple(t.shape) != (B,):
        raise ValueError(f"counts must have shape ({B},), got {tuple(t.shape)}")
    if t.is_floating_point() or t.dtype == torch.bool:
        raise ValueError(f"counts must be integers, got {t.dtype}")
    if not on_device and (int(t.min()) < 1 or int(t.max()) > n):
        raise ValueError(f"every count must lie in 1 .. n = {n}, got {int(t.min())} .. {int(t.max())}")


def _check_outputs(outs, dev) -> None:
    for name, t, shape, dtype in outs:
        if t is not None and not (isinstance(t, torch.Tensor) and t.is_contiguous() and t.dtype == dtype
                                  and tuple(t.shape) == shape and (dev is None or t.device == dev)):
            raise ValueError(f"{name} must be contiguous {dtype} {shape}" + (f" on {dev}" if dev is not None else ""))


def _ptr(t: Optional[torch.Tensor]):
    return t.data_ptr() if t is not None else None


class RandomSample:
    """``n_samples`` random points of every cloud (see the module docstring).

    ``seed`` and ``stream`` are the two 32-bit words of the Philox key;
    ``stream=None`` becomes the rank of the process under
    ``torch.distributed``, else 0, when the sampler first runs (or a
    ``BaselineTrainer`` takes it), so every DDP rank draws its own cut from
    one seed.  ``key_bits`` (32 in every product path) narrows the sort key:
    tests use it to force ties.

    One ``RandomSample`` belongs to one stream at a time: all its calls on a
    device share one work buffer (every call writes it anew, so it only grows
    to the largest batch seen: ragged batches padded to another length on
    every step cost no memory beyond the largest), and those that advance
    share one counter.  A call captured in a graph keeps the buffer it was
    captured with alive, and a later, larger batch gets a new one."""

    def __init__(self, n_samples: int, seed: int = 0, stream: Optional[int] = None, key_bits: int = 32) -> None:
        if isinstance(n_samples, bool) or int(n_samples) != n_samples or int(n_samples) < 1:
            raise ValueError(f"n_samples must be a positive integer, got {n_samples!r}")
        self.n_samples = int(n_samples)
        self.seed = _key_word(seed, "seed")
        self.stream = None if stream is None else _key_word(stream, "stream")
        if isinstance(key_bits, bool) or int(key_bits) != key_bits or not 1 <= int(key_bits) <= 32:
            raise ValueError(f"key_bits must lie in 1 .. 32, got {key_bits!r}")
        self.key_bits = int(key_bits)
        self._step0 = 0                            # the counter until it lives on a device
        self._step: Optional[torch.Tensor] = None  # one int64 on the device (the kernels' uint64)
        self._work: dict = {}         # device -> the scratch
        self._captured: list = []     # scratches a captured call reads: kept for good

    # ---- the key and the counter (as ndnet.augment.Augment)

    def resolve_stream(self) -> int:
        """``stream`` as given, or -- decided on the first call of this -- the
        process's rank under ``torch.distributed``, else 0."""
        if self.stream is None:
            import torch.distributed as dist
            self.stream = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        return self.stream

    def step_tensor(self, device) -> torch.Tensor:
        """The counter on ``device``: one int64 that every advancing call leaves one higher."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self._step is None:
            self._step = torch.tensor([self._step0], dtype=torch.int64, device=device)
        elif self._step.device != device:
            raise ValueError(f"this RandomSample's counter lives on {self._step.device}, not {device}")
        return self._step

    @property
    def step(self) -> int:
        """The number of the next draw (reading it synchronises with the device)."""
        return self._step0 if self._step is None else int(self._step.item())

    @step.setter
    def step(self, value: int) -> None:
        value = int(value)
        if not 0 <= value < 1 << 62:
            raise ValueError(f"step must lie in 0 .. 2^62 - 1, got {value}")
        self._step0 = value
        if self._step is not None:
            self._step.fill_(value)

    def config(self) -> "_lib.SampleConfig":
        c = _lib.SampleConfig()
        c.seed, c.stream, c.key_bits = self.seed, self.resolve_stream(), self.key_bits
        return c

    def state_dict(self) -> dict:
        """The configuration and the counter: a run resumed from it repeats the
        draws the original would have made."""
        return {"n_samples": self.n_samples, "seed": self.seed, "stream": self.stream, "key_bits": self.key_bits,
                "step": self.step}

    def load_state_dict(self, state: dict) -> None:
        fresh = RandomSample(**{k: v for k, v in state.items() if k != "step"})  # (validates)
        for k in ("n_samples", "seed", "stream", "key_bits"):
            setattr(self, k, getattr(fresh, k))
        self.step = state["step"]

    # ---- the call

    def _work_for(self, B: int, n: int, device) -> torch.Tensor:
        """The device's one scratch, grown to the largest batch seen."""
        words = (_lib.lib().ndnet_sample_work_bytes(B, n) + 7) // 8
        w = self._work.get(device)
        if w is None or w.numel() < words:
            w = self._work[device] = torch.empty(words, dtype=torch.int64, device=device)
        if torch.cuda.is_current_stream_capturing() and not any(w is k for k in self._captured):
            self._captured.append(w)  # the graph holds its address: it outlives a later, larger buffer
        return w

    def __call__(self, points: torch.Tensor, labels: Optional[torch.Tensor] = None, counts=None, *,
                 fill_label: int = -1, advance: bool = True, step: Optional[torch.Tensor] = None,
                 out_points: Optional[torch.Tensor] = None, out_labels: Optional[torch.Tensor] = None,
                 out_counts: Optional[torch.Tensor] = None, out_indices: Optional[torch.Tensor] = None
                 ) -> Tuple[torch.Tensor, Optional[torch.Tensor], torch.Tensor, torch.Tensor]:
        """``(points [B, S, 3], labels [B, S] int32 | None, sample_counts [B]
        int32, indices [B, S] int32)`` with ``S = n_samples``.

        ``points`` ``[B, n, 3]`` float32 on the GPU (a non-contiguous tensor
        is copied), ``labels`` None or integer class ids ``[B, n]`` (converted
        to int32), ``counts`` None or the ``[B]`` lengths of a ragged batch
        (converted to int32 on the device; range-checked when they come as a
        sequence or a CPU tensor; the padding is never read).  A cloud with
        fewer than ``S`` points fills its last rows with point 0,
        ``fill_label`` and index -1; ``sample_counts`` holds ``min(count,
        S)``.  ``advance=False`` leaves the counter where it is, so the next
        call repeats the draw.  ``step``: a one-element int64 device tensor to
        use as the counter instead of the sampler's own.  ``out_*``: buffers
        to write into (contiguous, of the outputs' shapes and dtypes), so a
        graph capture allocates nothing.  All arguments are checked before
        any GPU work (``ValueError``).  Stream ordered, no host
        synchronisation."""
        B, n = _check_points(points)
        S = self.n_samples
        if S > n:
            raise ValueError(f"n_samples must lie in 1 .. n = {n}, got {S}")
        _check_labels(labels, B, n)
        if labels is None and out_labels is not None:
            raise ValueError("out_labels goes with labels")
        _check_counts(counts, B, n)
        dev = points.device if points.is_cuda else None
        _check_outputs((("out_points", out_points, (B, S, 3), torch.float32),
                        ("out_labels", out_labels, (B, S), torch.int32),
                        ("out_counts", out_counts, (B,), torch.int32),
                        ("out_indices", out_indices, (B, S), torch.int32)), dev)
        if step is not None and not (isinstance(step, torch.Tensor) and step.dtype == torch.int64
                                     and step.numel() == 1 and (dev is None or step.device == dev)):
            raise ValueError("step must be a one-element int64 tensor on the points' device")
        fill_label = int(fill_label)
        if not -2 ** 31 <= fill_label < 2 ** 31:
            raise ValueError(f"fill_label must fit int32, got {fill_label}")
        _lib.require_gpu()
        if not points.is_cuda:
            raise RuntimeError("RandomSample needs its points on the GPU (there is no CPU fallback)")
        pts = points.contiguous()
        lab = labels.to(device=dev, dtype=torch.int32).contiguous() if labels is not None else None
        if counts is not None:
            counts = torch.as_tensor(counts).to(device=dev, dtype=torch.int32).contiguous()
        if out_points is None:
            out_points = torch.empty((B, S, 3), dtype=torch.float32, device=dev)
        if out_labels is None and lab is not None:
            out_labels = torch.empty((B, S), dtype=torch.int32, device=dev)
        if out_counts is None:
            out_counts = torch.empty((B,), dtype=torch.int32, device=dev)
        if out_indices is None:
            out_indices = torch.empty((B, S), dtype=torch.int32, device=dev)
        cfg = self.config()
        counter = step if step is not None else self.step_tensor(dev)
        rc = _lib.lib().ndnet_sample_random_run(
            ctypes.byref(cfg), pts.data_ptr(), _ptr(lab), _ptr(counts), B, n, S, fill_label, 1 if advance else 0,
            counter.data_ptr(), self._work_for(B, n, dev).data_ptr(), out_points.data_ptr(), _ptr(out_labels),
            out_counts.data_ptr(), out_indices.data_ptr(), _lib.stream_ptr(dev))
        _lib.check(rc, "ndnet_sample_random_run")
        return out_points, out_labels, out_counts, out_indices


def random_sample(points: torch.Tensor, n_samples: int, labels: Optional[torch.Tensor] = None, counts=None, *,
                  seed: int = 0, stream: int = 0, step: int = 0, fill_label: int = -1
                  ) -> Tuple[torch.Tensor, Optional[torch.Tensor], torch.Tensor, torch.Tensor]:
    """One draw without an object to keep: ``RandomSample(n_samples, seed,
    stream)`` at counter ``step``, called once."""
    sampler = RandomSample(n_samples, seed, stream)
    sampler.step = step
    return sampler(points, labels, counts, fill_label=fill_label)


def gather_samples(points: torch.Tensor, indices: torch.Tensor, labels: Optional[torch.Tensor] = None, *,
                   fill_label: int = -1, out_points: Optional[torch.Tensor] = None,
                   out_labels: Optional[torch.Tensor] = None, out_counts: Optional[torch.Tensor] = None
                   ) -> Tuple[torch.Tensor, Optional[torch.Tensor], torch.Tensor]:
    """``(points [B, S, 3], labels [B, S] int32 | None, sample_counts [B]
    int32)``: the points and labels at ``indices`` ``[B, S]`` int32 (those of
    ``farthest_point_sample``) in one HIP launch (``ndnet_sample_gather_run``).
    A row whose index lies in ``0 .. n - 1`` takes that point and label; any
    other (the -1 past a short cloud's count) takes point 0 and
    ``fill_label``, and ``sample_counts`` counts the valid rows.  ``points``
    ``[B, n, 3]`` float32 on the GPU, ``labels`` None or integer ids ``[B,
    n]``.  Checked before any GPU work (``ValueError``); stream ordered, no
    host synchronisation, no allocation when the ``out_*`` buffers are given."""
    B, n = _check_points(points)
    if (not isinstance(indices, torch.Tensor) or indices.dtype != torch.int32 or indices.dim() != 2
            or indices.shape[0] != B or indices.shape[1] < 1):
        raise ValueError(f"indices must be int32 [B, S] = [{B}, S >= 1], got "
                         f"{getattr(indices, 'dtype', type(indices).__name__)} {tuple(getattr(indices, 'shape', ()))}")
    S = indices.shape[1]
    _check_labels(labels, B, n)
    if labels is None and out_labels is not None:
        raise ValueError("out_labels goes with labels")
    if indices.device != points.device:
        raise ValueError(f"indices must be on the points' device {points.device}, got {indices.device}")
    dev = points.device if points.is_cuda else None
    _check_outputs((("out_points", out_points, (B, S, 3), torch.float32),
                    ("out_labels", out_labels, (B, S), torch.int32),
                    ("out_counts", out_counts, (B,), torch.int32)), dev)
    fill_label = int(fill_label)
    if not -2 ** 31 <= fill_label < 2 ** 31:
        raise ValueError(f"fill_label must fit int32, got {fill_label}")
    _lib.require_gpu()
    if not points.is_cuda:
        raise RuntimeError("gather_samples needs its points on the GPU (there is no CPU fallback)")
    pts, idx = points.contiguous(), indices.contiguous()
    lab = labels.to(device=dev, dtype=torch.int32).contiguous() if labels is not None else None
    if out_points is None:
        out_points = torch.empty((B, S, 3), dtype=torch.float32, device=dev)
    if out_labels is None and lab is not None:
        out_labels = torch.empty((B, S), dtype=torch.int32, device=dev)
    if out_counts is None:
        out_counts = torch.empty((B,), dtype=torch.int32, device=dev)
    rc = _lib.lib().ndnet_sample_gather_run(pts.data_ptr(), _ptr(lab), idx.data_ptr(), B, n, S, fill_label,
                                            out_points.data_ptr(), _ptr(out_labels), out_counts.data_ptr(),
                                            _lib.stream_ptr(dev))
    _lib.check(rc, "ndnet_sample_gather_run")
    return out_points, out_labels, out_counts
