"""Nearest-sample rows: which sample speaks for every point of a scan.

The PointNet-on-FPS baseline scores ``S`` farthest-point samples per cloud;
``nearest_sample`` gives every one of the ``n`` points of the scan the index of
its nearest sample, the baseline's counterpart of ``segment.point_rows``.  The
rows go unchanged into ``segment.point_labels``, ``segment.confusion``,
``segment.row_histogram`` and ``training.point_loss``.

    pts, = fps_downsample(points, 4096, counts=counts)            # [B, S, 3]
    rows = nearest_sample(points, pts, counts=counts)             # [B, n] int32

One HIP kernel (``ndnet_nearest_sample_run``, include/ndnet_nearest.h), an
exhaustive search in float32 with the distance expression of the FPS kernel,
``(dx*dx + dy*dy) + dz*dz`` with every operation rounded; ties go to the
smaller sample index.
"""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib
from .fps import _per_cloud


def nearest_sample(points: torch.Tensor, samples: torch.Tensor, counts=None, sample_counts=None,
                   out: Optional[torch.Tensor] = None, dist: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``rows[b, i]``: the index of the sample of cloud ``b`` nearest to its
    point ``i``, int32 ``[B, n]``.

    ``points`` ``[B, n, 3]`` and ``samples`` ``[B, S, 3]`` float32 on the GPU
    (a non-contiguous tensor is copied).  ``counts`` ``[B]``: only the first
    ``counts[b]`` points of cloud ``b`` exist; the others get -1 and are never
    read.  ``sample_counts`` ``[B]``: the same for the samples.  A point with a
    non-finite coordinate gets -1, a non-finite sample is never chosen, and a
    point that is itself a sample gets the smallest index at distance 0.
    ``out`` (int32 ``[B, n]``) and ``dist`` (float32 ``[B, n]``: the squared
    distance to the chosen sample, +inf with row -1, not written past
    ``counts[b]``) let a graph capture run without allocating.  Stream
    ordered, no host synchronisation."""
    for t, what in ((points, "points"), (samples, "samples")):
        if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.shape[-1] != 3:
            raise ValueError(f"{what} must be a [B, n, 3] tensor, got {tuple(getattr(t, 'shape', ()))}")
        if t.dtype != torch.float32:
            raise ValueError(f"{what} must be float32, got {t.dtype}")
    B, n, _ = points.shape
    S = samples.shape[1]
    if samples.shape[0] != B:
        raise ValueError(f"samples must hold the points' {B} clouds, got {samples.shape[0]}")
    if B < 1 or n < 1 or S < 1:
        raise ValueError(f"points and samples must hold at least one cloud and one point, got {tuple(points.shape)} "
                         f"and {tuple(samples.shape)}")
    if samples.device != points.device:
        raise ValueError(f"samples must be on the points' device {points.device}, got {samples.device}")
    for t, what in ((out, "out"), (dist, "dist")):
        dtype = torch.int32 if what == "out" else torch.float32
        if t is not None and not (isinstance(t, torch.Tensor) and t.dtype == dtype and tuple(t.shape) == (B, n)
                                  and t.device == points.device and t.is_contiguous()):
            raise ValueError(f"{what} must be contiguous {dtype} {(B, n)} on {points.device}")
    for t, what in ((counts, "counts"), (sample_counts, "sample_counts")):
        if t is not None and tuple(torch.as_tensor(t).shape) != (B,):
            raise ValueError(f"{what} must have shape ({B},), got {tuple(torch.as_tensor(t).shape)}")
    _lib.require_gpu()
    if not points.is_cuda:
        raise RuntimeError("nearest_sample needs its points on the GPU (there is no CPU fallback)")
    pts, smp = points.contiguous(), samples.contiguous()
    dev = pts.device
    counts = _per_cloud(counts, B, dev, "counts")
    sample_counts = _per_cloud(sample_counts, B, dev, "sample_counts")
    if out is None:
        out = torch.empty((B, n), dtype=torch.int32, device=dev)
    rc = _lib.lib().ndnet_nearest_sample_run(
        pts.data_ptr(), B, n, counts.data_ptr() if counts is not None else None, smp.data_ptr(), S,
        sample_counts.data_ptr() if sample_counts is not None else None, out.data_ptr(),
        dist.data_ptr() if dist is not None else None, _lib.stream_ptr(dev))
    _lib.check(rc, "ndnet_nearest_sample_run")
    return out
