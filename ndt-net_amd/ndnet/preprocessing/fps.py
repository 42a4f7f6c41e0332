"""Farthest point sampling on the GPU: fixed-size batches from ragged scans.

``Trainer.step`` and ``PipelinedSegmentation`` take ``[B, n, 3]`` with one
``n`` for all clouds; real scans have their own lengths.  (The NDT path --
``ndt_preprocessing``, ``segment.segment_points``, ``GraphedSegmentation`` --
also takes a padded batch with per-cloud ``counts`` and needs no cut.)
``farthest_point_sample`` picks
``n_samples`` evenly spread points of every cloud in one HIP kernel
(``ndnet_fps_run``, include/ndnet_fps.h: one workgroup per cloud, no launch
and no host round trip inside the selection), ``fps_downsample`` gathers the
points and their per-point tensors by the picked indices.

    points, classes, counts = collate_padded(scans)               # ragged -> [B, n_max, ...]
    pts, cls = fps_downsample(points.cuda(), 4096, classes.cuda(), counts=counts.cuda())
    gt = torch.nn.functional.one_hot(cls, n_classes + 1).float()  # for Trainer.step

The order is the usual one -- start point first (index 0 by default), then
always the point farthest from those picked, the lowest index among equals --
which is also open3d's ``farthest_point_down_sample`` rule.  Squared distances
are computed in the points' own dtype, ``(dx*dx + dy*dy) + dz*dz`` with every
operation rounded; open3d compares square roots in double, so near-ties can
fall differently and bit-equality with open3d is not claimed.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from .. import _lib


def _per_cloud(t, B: int, device, what: str) -> Optional[torch.Tensor]:
    if t is None:
        return None
    t = torch.as_tensor(t).to(device=device, dtype=torch.int32).contiguous()
    if t.shape != (B,):
        raise ValueError(f"{what} must have shape ({B},), got {tuple(t.shape)}")
    return t


def farthest_point_sample(points: torch.Tensor, n_samples: int, counts=None, start=None,
                          out: Optional[torch.Tensor] = None, min_dist: Optional[torch.Tensor] = None
                          ) -> torch.Tensor:
    """Indices of ``n_samples`` farthest-point samples of every cloud, int32
    ``[B, n_samples]``.

    ``points`` ``[B, n, 3]`` on the GPU, float32 or float64 (the dtype picks
    the kernel; a non-contiguous tensor is copied).  ``counts`` ``[B]``: only
    the first ``counts[b]`` points of cloud ``b`` exist (``1 <= counts[b] <=
    n``; the others are never read) and a cloud with fewer than ``n_samples``
    points has -1 in its tail.  ``start`` ``[B]``: the first sample of every
    cloud (default index 0).  Both are converted to int32 on the device.
    ``out`` (int32 ``[B, n_samples]``) and ``min_dist`` (``[B, n]`` of the
    points' dtype) let a graph capture run without allocating; ``min_dist``
    receives every existing point's final squared distance to the picked set,
    -1 for a picked point.  Stream ordered, no host synchronisation."""
    if not isinstance(points, torch.Tensor) or points.dim() != 3 or points.shape[-1] != 3:
        raise ValueError(f"points must be a [B, n, 3] tensor, got {tuple(getattr(points, 'shape', ()))}")
    if points.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"points must be float32 or float64, got {points.dtype}")
    B, n, _ = points.shape
    n_samples = int(n_samples)
    if B < 1 or n < 1:
        raise ValueError(f"points must hold at least one cloud and one point, got {tuple(points.shape)}")
    if n_samples < 1 or n_samples > n:
        raise ValueError(f"n_samples must lie in 1 .. n = {n}, got {n_samples}")
    _lib.require_gpu()
    if not points.is_cuda:
        raise RuntimeError("farthest_point_sample needs its points on the GPU (there is no CPU fallback)")
    pts = points.contiguous()
    dev = pts.device
    counts = _per_cloud(counts, B, dev, "counts")
    start = _per_cloud(start, B, dev, "start")
    if out is None:
        out = torch.empty((B, n_samples), dtype=torch.int32, device=dev)
    if min_dist is None:
        min_dist = torch.empty((B, n), dtype=pts.dtype, device=dev)
    for t, shape, dtype in ((out, (B, n_samples), torch.int32), (min_dist, (B, n), pts.dtype)):
        if not (t.is_contiguous() and t.dtype == dtype and t.device == dev and tuple(t.shape) == shape):
            raise ValueError(f"out / min_dist must be contiguous {dtype} {shape} on {dev}")
    run = _lib.lib().ndnet_fps_run if pts.dtype == torch.float32 else _lib.lib().ndnet_fps_run_f64
    rc = run(pts.data_ptr(), B, n, n_samples, counts.data_ptr() if counts is not None else None,
             start.data_ptr() if start is not None else None, min_dist.data_ptr(), out.data_ptr(),
             _lib.stream_ptr(dev))
    _lib.check(rc, "ndnet_fps_run")
    return out


def fps_downsample(points: torch.Tensor, n_samples: int, *per_point: torch.Tensor, counts=None, start=None
                   ) -> Tuple[torch.Tensor, ...]:
    """``(points [B, n_samples, 3], *gathered)``: the farthest-point samples of
    every cloud and the rows of any number of per-point tensors ``[B, n, ...]``
    (one-hot ground truth ``[B, n, C + 1]``, class ids ``[B, n]``, ...) at the
    same indices.  The selection is the HIP kernel; the gather is torch
    indexing.

    Every ``counts[b]`` must be at least ``n_samples`` (a shorter cloud has no
    ``n_samples`` distinct points to give).  This is checked only when
    ``counts`` arrives as a CPU tensor or a sequence -- checking a device
    tensor would need a host synchronisation."""
    if counts is not None and not (isinstance(counts, torch.Tensor) and counts.is_cuda):
        if int(torch.as_tensor(counts).min()) < int(n_samples):
            raise ValueError(f"every cloud needs at least n_samples = {int(n_samples)} points, "
                             f"got counts down to {int(torch.as_tensor(counts).min())}")
    idx = farthest_point_sample(points, n_samples, counts=counts, start=start).long()
    B = points.shape[0]
    rows = torch.arange(B, device=idx.device)[:, None]
    gathered = []
    for t in per_point:
        if t.dim() < 2 or t.shape[0] != B or t.shape[1] != points.shape[1]:
            raise ValueError(f"a per-point tensor must be [B, n, ...] = [{B}, {points.shape[1]}, ...], "
                             f"got {tuple(t.shape)}")
        gathered.append(t.to(idx.device)[rows, idx])
    return (points[rows, idx], *gathered)
