"""Per-point segmentation labels: the ND predictions mapped back to the points.

``ndt_preprocessing`` folds ``[B, N, 3]`` points into ``[B, k, 12]`` normal
distributions and ``NDTNetSegmentation`` scores one row per ND.  The row every
point was folded into comes from the NDT plan itself (``ndnet_ndt_point_rows``,
include/ndnet_amd.h: the kernels' own voxel keys, dense ids and survivor
numbering), the class of every row and the gather to the points from
include/ndnet_segment.h.  All of it runs on the GPU in HIP kernels; ``iou`` is
plain torch.

    labels, log_probs = segment_points(model, 1000, points)       # [B, N] int32
    conf = confusion(labels, gt, model.num_classes)               # [C + 1, C + 1]
    per_class, mean = iou(conf)

The PointNet-on-FPS baseline (``ndnet.models.pointnet``) is scored the same
way: ``segment_points_fps`` labels ``n_samples`` farthest-point samples per
cloud and gives every point the class of its nearest sample.

    labels, log_probs = segment_points_fps(baseline, 4096, points, counts=counts)

``row_histogram`` goes the other way for training: the points' rows and labels
give every ND row its class histogram, the target of the point-level loss
(``ndnet.training.point_loss``).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib
from .preprocessing.fps import _per_cloud, farthest_point_sample
from .preprocessing.nearest import nearest_sample
from .preprocessing.ndtnet_preprocessing import NdtPlan, check_counts, ndt_preprocessing


def point_rows(points: torch.Tensor, fill: str = "none", plan: Optional[NdtPlan] = None,
               rows_block: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
               counts=None) -> torch.Tensor:
    """The output row of every point of ``points`` ``[B, N, 3]``, int32
    ``[B, N]``: -1 (``fill="none"``) or the nearest row (``fill="nearest"``)
    for a point that contributed to no surviving ND.  ``plan`` defaults to the
    plan of the last ``ndt_preprocessing`` / ``ndt_multiscale`` call and
    ``rows_block`` to the ``[B, k, 12]`` block it returned (its last level's);
    ``points`` must be the points that call ran on.  ``counts``: the per-cloud
    point counts that run took (a ``[B]`` tensor or sequence; with the
    defaulted plan, the last call's); padding points get -1."""
    if counts is not None and points.dim() == 3:
        check_counts(counts, points.shape[0], points.shape[1])
    _lib.require_gpu()
    if plan is None:
        plan = ndt_preprocessing.last_plan
        if plan is None:
            raise RuntimeError("point_rows needs a plan: call ndt_preprocessing first")
        if rows_block is None:
            rows_block = ndt_preprocessing.last_rows
        if counts is None:
            counts = ndt_preprocessing.last_counts
    pts = points.to(device=plan.device, dtype=torch.float32).contiguous()
    k = rows_block.shape[1] if rows_block is not None else None
    counts = _per_cloud(counts, pts.shape[0], plan.device, "counts")
    return plan.point_rows(pts, rows_block, k, fill, out, counts=counts)


def _label_args(cols: int, unassigned: Optional[int], out: Optional[torch.Tensor], dtype) -> Tuple[torch.dtype, int]:
    """The label dtype (``out``'s when given) and the unassigned marker of
    ``point_labels``, checked on the host (``ValueError``)."""
    if out is not None:
        dtype = out.dtype
    if dtype not in (torch.int32, torch.uint8):
        raise ValueError(f"point labels are int32 or uint8, got {dtype}")
    if dtype == torch.int32:
        return dtype, -1 if unassigned is None else int(unassigned)
    if cols > 255:
        raise ValueError(f"uint8 labels hold at most 255 columns, got {cols}")
    unassigned = 255 if unassigned is None else int(unassigned)
    if not cols <= unassigned <= 255:
        raise ValueError(f"the uint8 unassigned marker must lie in {cols} .. 255 (no class), got {unassigned}")
    return dtype, unassigned


def point_labels(scores: torch.Tensor, rows: torch.Tensor, unassigned: Optional[int] = None,
                 out: Optional[torch.Tensor] = None, nd_labels: Optional[torch.Tensor] = None,
                 dtype: torch.dtype = torch.int32) -> torch.Tensor:
    """``labels[b, i] = argmax(scores[b, rows[b, i]])``, int32 ``[B, N]``;
    ``unassigned`` where ``rows[b, i] < 0``.  ``scores`` ``[B, k, C + 1]``
    float32 (log-probs or any per-ND scores), ``rows`` ``[B, N]`` int32.  The
    argmax runs once per ND (first maximum, NaN as a maximum, as
    ``torch.argmax``); ``nd_labels`` ``[B, k]`` int32 receives it.

    ``dtype=torch.uint8`` (or a uint8 ``out``, whose dtype wins): one byte per
    point, a quarter of the bytes to copy back to the host.  ``unassigned``
    defaults to -1 for int32 and to 255 for uint8, where it must be no class:
    more than 255 columns or a marker below the column count is a
    ``ValueError``, raised before any GPU work."""
    dtype, unassigned = _label_args(scores.shape[-1], unassigned, out, dtype)
    _lib.require_gpu()
    assert scores.is_cuda and scores.dtype == torch.float32 and scores.dim() == 3
    assert rows.dtype == torch.int32 and rows.dim() == 2 and rows.device == scores.device
    assert rows.shape[0] == scores.shape[0]
    scores, rows = scores.contiguous(), rows.contiguous()
    B, k, cols = scores.shape
    n = rows.shape[1]
    if out is None:
        out = torch.empty((B, n), dtype=dtype, device=scores.device)
    if nd_labels is None:
        nd_labels = torch.empty((B, k), dtype=torch.int32, device=scores.device)
    for t, shape, dt in ((out, (B, n), dtype), (nd_labels, (B, k), torch.int32)):
        assert t.is_contiguous() and t.dtype == dt and t.device == scores.device and t.shape == shape
    name = "ndnet_seg_point_labels" if dtype == torch.int32 else "ndnet_seg_point_labels_u8"
    rc = getattr(_lib.lib(), name)(scores.data_ptr(), rows.data_ptr(), B, n, k, cols, unassigned,
                                   nd_labels.data_ptr(), out.data_ptr(), _lib.stream_ptr(scores.device))
    _lib.check(rc, name)
    return out


def segment_points(model, num_nds: int, points: torch.Tensor, fill: str = "nearest", counts=None
                   ) -> Tuple[torch.Tensor, torch.Tensor]:
    """A class for every point of ``points`` ``[B, N, 3]``: ``ndt_preprocessing``,
    ``model`` (an eval-mode ``NDTNetSegmentation``), the points' rows and the
    rows' classes, eagerly under ``torch.no_grad()``.

    Returns ``(labels [B, N] int32, log_probs [B, num_nds, C + 1])``.  With
    ``fill="nearest"`` (default) a point that fell into a pruned ND or the
    ``N % 8`` tail takes the class of the nearest surviving ND; with
    ``fill="none"`` it gets -1.  Every point of a cloud whose NDT failed gets
    -1 either way.

    ``counts`` (a ``[B]`` tensor or sequence): a ragged batch, ``points``
    padded to ``[B, n_max, 3]`` (``collate_padded``); cloud ``b`` is its first
    ``counts[b]`` points, labelled as when it is run alone, and the padding
    points get -1 (``confusion`` leaves them out)."""
    with torch.no_grad():
        p, c, _ = ndt_preprocessing(int(num_nds), points, counts=counts)
        plan, block = ndt_preprocessing.last_plan, ndt_preprocessing.last_rows
        log_probs = model(p.to(plan.device), c.to(plan.device))
        rows = point_rows(points, fill, plan, block, counts=ndt_preprocessing.last_counts)
        return point_labels(log_probs, rows), log_probs


class FpsSegmentBuffers:
    """Every intermediate of ``segment_points_fps`` for one batch shape,
    allocated once: with these the whole sequence allocates nothing but the
    model's output and can be captured in one ``torch.cuda.graph`` on one
    stream.  ``indices`` ``[B, S]`` int32 (the FPS picks, -1 past a short
    cloud's count), ``samples`` ``[B, S, 3]``, ``rows`` ``[B, n]`` int32 (the
    nearest sample of every point), ``labels`` ``[B, n]`` int32."""

    def __init__(self, B: int, n: int, n_samples: int, device) -> None:
        S = int(n_samples)
        i32 = dict(dtype=torch.int32, device=device)
        self.shape = (int(B), int(n), S)
        self.indices = torch.empty((B, S), **i32)
        self.min_dist = torch.empty((B, n), dtype=torch.float32, device=device)
        self.gather_index = torch.empty((B, S, 3), dtype=torch.int64, device=device)
        self.samples = torch.empty((B, S, 3), dtype=torch.float32, device=device)
        self.sample_counts = torch.empty((B,), **i32)
        self.rows = torch.empty((B, n), **i32)
        self.nd_labels = torch.empty((B, S), **i32)
        self.labels = torch.empty((B, n), **i32)


def segment_points_fps(model, n_samples: int, points: torch.Tensor, counts=None, start=None,
                       buffers: Optional[FpsSegmentBuffers] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """A class for every point of ``points`` ``[B, n, 3]`` (float32, on the
    GPU) from the PointNet baseline: ``farthest_point_sample`` picks
    ``n_samples`` points per cloud, ``model`` (an eval-mode
    ``PointNetSegmentation``) scores them, ``nearest_sample`` gives every point
    its nearest sample and ``point_labels`` that sample's class, under
    ``torch.no_grad()``.

    Returns ``(labels [B, n] int32, log_probs [B, n_samples, C + 1])``.

    ``counts`` (a ``[B]`` tensor or sequence): a ragged batch padded to
    ``[B, n_max, 3]``; the padding points get -1 (``confusion`` leaves them
    out).  A cloud with fewer than ``n_samples`` points repeats its first point
    in the model's input; those copies stand for no point.  ``start``: the
    first sample of every cloud (``farthest_point_sample``).

    ``buffers`` (``FpsSegmentBuffers`` of this shape): every step writes into
    it -- the FPS indices, the gather (``torch.gather`` into ``samples``), the
    rows and the labels, which are then ``buffers.labels`` -- so the sequence
    is one straight line of launches on the current stream with no allocation
    but the model's output, and capturable; give ``counts`` / ``start`` as
    int32 tensors on the device then."""
    if not isinstance(points, torch.Tensor) or points.dim() != 3 or points.shape[-1] != 3:
        raise ValueError(f"points must be a [B, n, 3] tensor, got {tuple(getattr(points, 'shape', ()))}")
    if points.dtype != torch.float32:
        raise ValueError(f"points must be float32, got {points.dtype}")
    B, n, _ = points.shape
    S = int(n_samples)
    if buffers is not None and buffers.shape != (B, n, S):
        raise ValueError(f"buffers are for (B, n, n_samples) = {buffers.shape}, got {(B, n, S)}")
    with torch.no_grad():
        pts = points.contiguous()
        buf = buffers if buffers is not None else FpsSegmentBuffers(B, n, S, pts.device)
        dev = pts.device
        counts = _per_cloud(counts, B, dev, "counts")
        farthest_point_sample(pts, S, counts=counts, start=start, out=buf.indices, min_dist=buf.min_dist)
        # the gather by the picked indices (-1 past a short cloud's count reads point 0)
        buf.gather_index.copy_(buf.indices.unsqueeze(2).expand(B, S, 3))
        buf.gather_index.clamp_(min=0)
        torch.gather(pts, 1, buf.gather_index, out=buf.samples)
        log_probs = model(buf.samples)
        sample_counts = None
        if counts is not None:
            sample_counts = torch.clamp(counts, max=S, out=buf.sample_counts)
        nearest_sample(pts, buf.samples, counts=counts, sample_counts=sample_counts, out=buf.rows)
        labels = point_labels(log_probs, buf.rows, out=buf.labels, nd_labels=buf.nd_labels)
        return labels, log_probs


def confusion(pred: torch.Tensor, gt: torch.Tensor, num_classes: int) -> torch.Tensor:
    """Point-level confusion matrix ``[C + 1, C + 1]`` int64 (``[gt, pred]``)
    over every point whose ``pred`` and ``gt`` both lie in ``0 .. num_classes``;
    other points (unassigned, ignore labels) are left out."""
    _lib.require_gpu()
    cols = int(num_classes) + 1
    assert pred.is_cuda and gt.device == pred.device and pred.numel() == gt.numel() and pred.numel() > 0
    p = pred.to(torch.int32).contiguous()
    g = gt.to(torch.int32).contiguous()
    conf = torch.zeros(cols * cols + 1, dtype=torch.int64, device=pred.device)
    rc = _lib.lib().ndnet_seg_confusion(p.data_ptr(), g.data_ptr(), p.numel(), cols, conf.data_ptr(),
                                        _lib.stream_ptr(pred.device))
    _lib.check(rc, "ndnet_seg_confusion")
    return conf[:-1].view(cols, cols)


def row_histogram(rows: torch.Tensor, labels: torch.Tensor, num_nds: int, cols: int, ignore_label: int = -1,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The class histogram of every ND row, int32 ``[B, num_nds, cols]``:
    ``hist[b, r, c]`` = the number of points ``i`` with ``rows[b, i] == r`` and
    ``labels[b, i] == c`` (``rows`` and ``labels`` int32 ``[B, N]``).  A point
    whose row is outside ``0 .. num_nds - 1`` (-1: no row, padding) or whose
    label is outside ``0 .. cols - 1`` or equals ``ignore_label`` (-1: none)
    is left out.  The target of the point-level training loss
    (``ndnet.training.point_loss``).  ``out`` is overwritten whole."""
    _lib.require_gpu()
    assert rows.is_cuda and rows.dtype == torch.int32 and rows.dim() == 2
    assert labels.dtype == torch.int32 and labels.shape == rows.shape and labels.device == rows.device
    rows, labels = rows.contiguous(), labels.contiguous()
    B, n = rows.shape
    k, cols = int(num_nds), int(cols)
    if out is None:
        out = torch.empty((B, k, cols), dtype=torch.int32, device=rows.device)
    assert out.is_contiguous() and out.dtype == torch.int32 and out.device == rows.device and out.shape == (B, k, cols)
    rc = _lib.lib().ndnet_seg_row_hist(rows.data_ptr(), labels.data_ptr(), B, n, k, cols, int(ignore_label),
                                       out.data_ptr(), _lib.stream_ptr(rows.device))
    _lib.check(rc, "ndnet_seg_row_hist")
    return out


def iou(conf: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-class intersection over union of a ``[gt, pred]`` confusion matrix
    and its mean over the classes with a non-empty union (NaN for the others,
    and for the mean of an all-zero matrix).  Plain torch: any device."""
    c = conf.to(torch.float64)
    tp = c.diagonal()
    union = c.sum(0) + c.sum(1) - tp
    per_class = torch.where(union > 0, tp / union.clamp(min=1), torch.full_like(tp, float("nan")))
    seen = union > 0
    mean = per_class[seen].mean() if bool(seen.any()) else torch.tensor(float("nan"), dtype=torch.float64,
                                                                         device=conf.device)
    return per_class, mean
