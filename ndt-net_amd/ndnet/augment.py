"""Train-time augmentation of a batch of scans on the GPU.

``Augment`` draws, per cloud, a yaw about z, a scale, flips of x and y and a
shift, adds jitter to every point and drops a random share of the points, all
in three stream-ordered HIP launches (``ndnet_aug_run``,
include/ndnet_augment.h, which defines every operation).  Dropout is a stable
compaction: the kept points of cloud ``b`` move to its first rows, their
labels with them, and the new lengths leave as device ``counts`` for the ragged
NDT path -- no host round trip, so the call can be captured in a HIP graph.
The random state is a step counter in device memory that every call (and every
replay of a captured call) advances; the draws are a pure function of
``(seed, stream, step, cloud, point)``.

    aug = Augment(yaw=math.pi, scale=(0.95, 1.05), jitter=0.01, drop=0.2, seed=1)
    pts, ids, counts = aug(points.cuda(), ids.cuda(), counts)   # counts: int32 [B] on the device
    trainer = Trainer(model, ..., augment=aug)                  # or inside the (graphed) train step
"""
from __future__ import annotations

import ctypes
import math
import operator
from typing import Optional, Tuple

import torch

from . import _lib

_U32 = 1 << 32


def _amplitude(v, what: str) -> float:
    v = float(v)
    if not v >= 0.0:  # (NaN included)
        raise ValueError(f"{what} must be >= 0, got {v}")
    return v


def _probability(v, what: str) -> float:
    v = float(v)
    if not 0.0 <= v <= 1.0:
        raise ValueError(f"{what} must lie in [0, 1], got {v}")
    return v


def _key_word(v, what: str) -> int:
    try:  # any integer type (numpy and torch scalars too), but no bool and no float
        i = None if isinstance(v, bool) else operator.index(v)
    except TypeError:
        i = None
    if i is None or not 0 <= i < _U32:
        raise ValueError(f"{what} must be an integer in 0 .. 2^32 - 1, got {v!r}")
    return i


class Augment:
    """The augmentation of a ``[B, n, 3]`` batch (see the module docstring).

    ``yaw``: the rotation about z is uniform in ``[-yaw, yaw)`` radians.
    ``scale = (lo, hi)``: uniform in ``[lo, hi)``, ``0 < lo <= hi``.
    ``flip = (px, py)``: the probabilities of mirroring x and y (resolved to
    1 / 65536).  ``shift = (sx, sy, sz)``: a translation uniform in
    ``[-s, s)`` per axis.  ``jitter``: the standard deviation of the noise
    added to every coordinate (a sum of four uniforms, within 3.47 sigma).
    ``drop``: every cloud draws its own drop probability uniformly in
    ``[0, drop)``; point 0 of a cloud always survives.  ``seed`` and ``stream``
    are the two 32-bit words of the Philox key; ``stream=None`` becomes the
    rank of the process under ``torch.distributed``, else 0, when the
    augmentation first runs (or a ``Trainer`` takes it).

    All arguments are checked here, before any GPU work (``ValueError``).

    One ``Augment`` belongs to one stream at a time: its calls of one shape
    share a work buffer and all of them advance one counter, so they must be
    ordered by the stream (or by a graph captured from it).  Use one
    ``Augment`` per stream for concurrent work."""

    def __init__(self, yaw: float = math.pi, scale=(0.95, 1.05), flip=(0.0, 0.5), shift=(0.0, 0.0, 0.0),
                 jitter: float = 0.0, drop: float = 0.0, seed: int = 0, stream: Optional[int] = None) -> None:
        self.yaw = _amplitude(yaw, "yaw")
        try:
            lo, hi = (float(v) for v in scale)
        except (TypeError, ValueError):
            raise ValueError(f"scale must be a pair (lo, hi), got {scale!r}") from None
        if not (lo > 0.0 and lo <= hi):
            raise ValueError(f"scale must satisfy 0 < lo <= hi, got {(lo, hi)}")
        self.scale = (lo, hi)
        try:
            px, py = flip
        except (TypeError, ValueError):
            raise ValueError(f"flip must be a pair of probabilities, got {flip!r}") from None
        self.flip = (_probability(px, "flip[0]"), _probability(py, "flip[1]"))
        try:
            sx, sy, sz = shift
        except (TypeError, ValueError):
            raise ValueError(f"shift must hold three amplitudes, got {shift!r}") from None
        self.shift = tuple(_amplitude(v, f"shift[{a}]") for a, v in enumerate((sx, sy, sz)))
        self.jitter = _amplitude(jitter, "jitter")
        self.drop = _probability(drop, "drop")
        self.seed = _key_word(seed, "seed")
        self.stream = None if stream is None else _key_word(stream, "stream")
        self.xform: Optional[torch.Tensor] = None  # the last call's [B, 12] rows of [M | t]
        self._step0 = 0                            # the counter until it lives on a device
        self._step: Optional[torch.Tensor] = None  # one int64 on the device (the kernels' uint64)
        self._work: dict = {}

    # ---- the key and the counter

    def resolve_stream(self) -> int:
        """``stream`` as given, or -- decided on the first call of this -- the
        process's rank under ``torch.distributed``, else 0."""
        if self.stream is None:
            import torch.distributed as dist
            self.stream = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        return self.stream

    def step_tensor(self, device) -> torch.Tensor:
        """The counter on ``device``: one int64 that every call leaves one higher."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self._step is None:
            self._step = torch.tensor([self._step0], dtype=torch.int64, device=device)
        elif self._step.device != device:
            raise ValueError(f"this Augment's counter lives on {self._step.device}, not {device}")
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

    def config(self) -> "_lib.AugConfig":
        c = _lib.AugConfig()
        c.seed, c.stream = self.seed, self.resolve_stream()
        c.yaw_max, (c.scale_lo, c.scale_hi) = self.yaw, self.scale
        c.shift_max[0], c.shift_max[1], c.shift_max[2] = self.shift
        c.drop_max, c.jitter_sigma = self.drop, self.jitter
        c.flip_x_16, c.flip_y_16 = (int(round(p * 65536.0)) for p in self.flip)
        return c

    def state_dict(self) -> dict:
        """The configuration and the counter: a run resumed from it repeats the
        draws the original would have made."""
        return {"yaw": self.yaw, "scale": self.scale, "flip": self.flip, "shift": self.shift, "jitter": self.jitter,
                "drop": self.drop, "seed": self.seed, "stream": self.stream, "step": self.step}

    def load_state_dict(self, state: dict) -> None:
        fresh = Augment(**{k: v for k, v in state.items() if k != "step"})  # (validates)
        for k in ("yaw", "scale", "flip", "shift", "jitter", "drop", "seed", "stream"):
            setattr(self, k, getattr(fresh, k))
        self.step = state["step"]

    # ---- the call

    def _work_for(self, B: int, n: int, device) -> torch.Tensor:
        key = (B, n, device)
        w = self._work.get(key)
        if w is None:
            nbytes = _lib.lib().ndnet_aug_work_bytes(B, n)
            w = self._work[key] = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=device)
        return w

    def __call__(self, points: torch.Tensor, labels: Optional[torch.Tensor] = None, counts=None, *,
                 out_points: Optional[torch.Tensor] = None, out_labels: Optional[torch.Tensor] = None,
                 out_counts: Optional[torch.Tensor] = None
                 ) -> Tuple[torch.Tensor, Optional[torch.Tensor], torch.Tensor]:
        """``(points', labels', counts')``: the augmented batch.  ``points``
        ``[B, n, 3]`` on the GPU (converted to contiguous float32), ``labels``
        None or integer class ids ``[B, n]`` (converted to int32), ``counts``
        None or the ``[B]`` lengths of a ragged batch (converted to int32 on
        the device; the padding is never read).  ``counts'`` is int32 ``[B]``
        on the device; the rows of ``points'`` and ``labels'`` from
        ``counts'[b]`` on are not written.  ``out_*``: buffers to write into
        (contiguous, of the outputs' shapes and dtypes); with ``drop == 0``
        ``out_points`` may be ``points`` itself.  Stream ordered, no host
        synchronisation; the counter advances by one."""
        if not isinstance(points, torch.Tensor) or points.dim() != 3 or points.shape[-1] != 3:
            raise ValueError(f"points must be a [B, n, 3] tensor, got {tuple(getattr(points, 'shape', ()))}")
        B, n, _ = points.shape
        if B < 1 or n < 1:
            raise ValueError(f"points must hold at least one cloud and one point, got {tuple(points.shape)}")
        if labels is not None:
            if labels.is_floating_point() or labels.dtype == torch.bool or tuple(labels.shape) != (B, n):
                raise ValueError(f"labels must be integer class ids of shape {(B, n)}, got {labels.dtype} "
                                 f"{tuple(labels.shape)}")
        elif out_labels is not None:
            raise ValueError("out_labels goes with labels")
        _lib.require_gpu()
        if not points.is_cuda:
            raise RuntimeError("Augment needs its points on the GPU (there is no CPU fallback)")
        dev = points.device
        pts = points.to(torch.float32).contiguous()
        lab = labels.to(device=dev, dtype=torch.int32).contiguous() if labels is not None else None
        if counts is not None:
            counts = torch.as_tensor(counts).to(device=dev, dtype=torch.int32).contiguous()
            if counts.shape != (B,):
                raise ValueError(f"counts must have shape ({B},), got {tuple(counts.shape)}")
        if out_points is None:
            out_points = torch.empty_like(pts)
        if out_labels is None and lab is not None:
            out_labels = torch.empty_like(lab)
        if out_counts is None:
            out_counts = torch.empty((B,), dtype=torch.int32, device=dev)
        for t, shape, dtype in ((out_points, (B, n, 3), torch.float32), (out_labels, (B, n), torch.int32),
                                (out_counts, (B,), torch.int32)):
            if t is not None and not (t.is_contiguous() and t.dtype == dtype and t.device == dev
                                      and tuple(t.shape) == shape):
                raise ValueError(f"an output buffer must be contiguous {dtype} {shape} on {dev}")
        xform = torch.empty((B, 12), dtype=torch.float32, device=dev)
        cfg = self.config()
        rc = _lib.lib().ndnet_aug_run(
            ctypes.byref(cfg), pts.data_ptr(), lab.data_ptr() if lab is not None else None,
            counts.data_ptr() if counts is not None else None, B, n, self.step_tensor(dev).data_ptr(),
            self._work_for(B, n, dev).data_ptr(), out_points.data_ptr(),
            out_labels.data_ptr() if out_labels is not None else None, out_counts.data_ptr(), xform.data_ptr(),
            _lib.stream_ptr(dev))
        _lib.check(rc, "ndnet_aug_run")
        self.xform = xform
        return out_points, out_labels, out_counts
