"""Batched NDT preprocessing on the GPU.

Drop-in for ``ndnet.preprocessing.ndtnet_preprocessing.ndt_preprocessing``
(reference ndnet/preprocessing/ndtnet_preprocessing.py:6-73).  The reference
loops over the batch on the host, copies each cloud to the CPU as float64,
runs the C core and copies the result back; here the whole batch stays in HBM
and one call of ``ndnet_ndt_run`` (include/ndnet_amd.h) processes every cloud.
Results are bit-identical to the reference core's single-worker schedule
(SURVEY §8c), cast to float32 and passed through ``nan_to_num`` as the
reference does (ndtnet_preprocessing.py:66-69).
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Tuple

import torch

from .. import _lib
from .fps import _per_cloud


class NdtPlan:
    """Device workspace for one (batch, points, NDs, classes) shape."""

    def __init__(self, batch: int, num_points: int, num_nds: int, num_classes: int = -1,
                 voxel_capacity: int = 0, device: torch.device | None = None):
        _lib.require_gpu()
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.batch, self.num_points, self.num_nds, self.num_classes = batch, num_points, num_nds, num_classes
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            rc = _lib.lib().ndnet_ndt_plan_create(batch, num_points, num_nds, num_classes, voxel_capacity,
                                                  ctypes.byref(h))
        _lib.check(rc, "ndnet_ndt_plan_create")
        self.handle = h
        self.stats = torch.zeros((batch, _lib.STATS_BYTES), dtype=torch.uint8, device=self.device)

    def __del__(self):
        h = getattr(self, "handle", None)
        if h is not None and h.value:
            try:
                with torch.cuda.device(self.device):
                    _lib.lib().ndnet_ndt_plan_destroy(h)
            except Exception:
                pass
            self.handle = None

    def _counts_ptr(self, counts: Optional[torch.Tensor]):
        if counts is None:
            return None
        assert counts.is_contiguous() and counts.dtype == torch.int32 and counts.device == self.device
        assert counts.shape == (self.batch,)
        return counts.data_ptr()

    def run(self, points: torch.Tensor, labels: Optional[torch.Tensor], out: torch.Tensor,
            out_classes: Optional[torch.Tensor], part: int = 0, counts: Optional[torch.Tensor] = None) -> None:
        """part: 0 the whole run; 1 the front only (k_front); 2 the rest, after a
        part-1 call with the same arguments in stream order
        (include/ndnet_amd.h ndnet_ndt_set_run_part).

        counts: int32 ``[B]`` on the plan's device, or None.  Cloud ``b`` is
        then its first ``counts[b]`` points alone -- ``points`` is the padded
        ``[B, num_points, 3]`` batch, whose padding may hold anything -- and its
        rows are those of that cloud run on its own.  A count outside
        ``1 .. num_points`` fails its cloud (stats rc -20, zero rows).  The
        kernels read the counts on the device: a captured run follows whatever
        the buffer holds at replay (include/ndnet_amd.h ndnet_ndt_run_counts)."""
        assert points.is_contiguous() and points.dtype == torch.float32 and points.device == self.device
        assert out.is_contiguous() and out.shape == (self.batch, self.num_nds, 12)
        self.raise_sync_failures()
        st = _lib.stream_ptr(self.device)
        _lib.check(_lib.lib().ndnet_ndt_set_run_part(self.handle, int(part)), "ndnet_ndt_set_run_part")
        rc = _lib.lib().ndnet_ndt_run_counts(
            self.handle, st, points.data_ptr(),
            labels.data_ptr() if labels is not None else None,
            self._counts_ptr(counts),
            out.data_ptr(),
            out_classes.data_ptr() if out_classes is not None else None,
            self.stats.data_ptr())
        if part:
            _lib.lib().ndnet_ndt_set_run_part(self.handle, 0)
        _lib.check(rc, "ndnet_ndt_run")

    def set_path(self, path: int) -> None:
        """1: one launch per stage; 2: the fused front kernel (k_front); 0: 2 where allowed."""
        _lib.check(_lib.lib().ndnet_ndt_set_path(self.handle, int(path)), "ndnet_ndt_set_path")

    def set_cu_share(self, front_share: int, welford_share: Optional[int] = None) -> None:
        """k_front on CUs / front_share, k_welford_q on CUs / welford_share
        (default: front_share) -- include/ndnet_amd.h ndnet_ndt_set_cu_share:
        leaves CUs to another stream; identical results."""
        ws = front_share if welford_share is None else welford_share
        _lib.check(_lib.lib().ndnet_ndt_set_cu_share(self.handle, int(front_share), int(ws)), "ndnet_ndt_set_cu_share")

    def set_exact_counts(self, on: bool) -> None:
        """Count every bisection grid, also those with fewer voxels than k
        (include/ndnet_amd.h ndnet_ndt_set_exact_counts; debug / parity)."""
        _lib.check(_lib.lib().ndnet_ndt_set_exact_counts(self.handle, 1 if on else 0), "ndnet_ndt_set_exact_counts")

    def set_front_staged(self, on: bool) -> None:
        """k_front's scatter through LDS records in ND order (default on;
        include/ndnet_amd.h ndnet_ndt_set_front_staged; identical results)."""
        _lib.check(_lib.lib().ndnet_ndt_set_front_staged(self.handle, 1 if on else 0), "ndnet_ndt_set_front_staged")

    @property
    def front_staged(self) -> bool:
        """Whether k_front's scatter runs staged for this plan's shapes (float input)."""
        rc = _lib.lib().ndnet_ndt_get_front_staged(self.handle)
        if rc < 0:
            _lib.check(rc, "ndnet_ndt_get_front_staged")
        return rc == 1

    def set_lazy_list(self, on: bool) -> None:
        """Defer the retained KL list of clouds whose level-1 prune cannot read
        it (num_nds <= k) until a prune or dump needs it (default on;
        include/ndnet_amd.h ndnet_ndt_set_lazy_list)."""
        _lib.check(_lib.lib().ndnet_ndt_set_lazy_list(self.handle, 1 if on else 0), "ndnet_ndt_set_lazy_list")

    def set_welford_form(self, form: str) -> None:
        """k_welford_q's light form: "light64" (one ND per lane), "quad" (a lane
        quad per ND) or "auto" (quad at CU share 1, light64 above: the default);
        identical results (include/ndnet_amd.h ndnet_ndt_set_welford_form)."""
        code = {"auto": 0, "light64": 1, "quad": 2}[form]
        _lib.check(_lib.lib().ndnet_ndt_set_welford_form(self.handle, code), "ndnet_ndt_set_welford_form")

    @property
    def welford_form(self) -> str:
        return {1: "light64", 2: "quad"}[_lib.lib().ndnet_ndt_get_welford_form(self.handle)]

    def set_heavy_threshold(self, min_samples: int) -> None:
        """NDs with at least ``min_samples`` points get a whole wave in
        k_welford_q (include/ndnet_amd.h ndnet_ndt_set_heavy_threshold;
        identical results, default 256)."""
        _lib.check(_lib.lib().ndnet_ndt_set_heavy_threshold(self.handle, int(min_samples)),
                   "ndnet_ndt_set_heavy_threshold")

    @property
    def path(self) -> int:
        return int(_lib.lib().ndnet_ndt_get_path(self.handle))

    @property
    def front_lanes(self) -> Tuple[int, int]:
        """(first lane, lane count) of the device's front lanes this plan's
        k_front occupies (include/ndnet_amd.h ndnet_ndt_get_front_lanes;
        count 0 on the one-launch-per-stage path)."""
        l0, nl = ctypes.c_int(0), ctypes.c_int(0)
        _lib.check(_lib.lib().ndnet_ndt_get_front_lanes(self.handle, ctypes.byref(l0), ctypes.byref(nl)),
                   "ndnet_ndt_get_front_lanes")
        return l0.value, nl.value

    def raise_sync_failures(self) -> None:
        """Raises ``NdtCloudError`` (rc -22) if a k_front cloud barrier of an
        earlier run of this plan timed out -- read from mapped host memory,
        without synchronising (include/ndnet_amd.h
        ndnet_ndt_take_sync_failures).  Every ``run``, ``ndt_preprocessing``
        call and pipeline replay checks it, whatever ``check`` says."""
        rc = _lib.lib().ndnet_ndt_take_sync_failures(self.handle)
        if rc < 0:
            _lib.check(rc, "ndnet_ndt_take_sync_failures")
        if rc:
            raise NdtCloudError([_lib.NDNET_ERR_SYNC], sync=True)

    def prune(self, num_nds: int, out: torch.Tensor, out_classes: Optional[torch.Tensor] = None) -> None:
        st = _lib.stream_ptr(self.device)
        rc = _lib.lib().ndnet_ndt_prune(self.handle, st, num_nds, out.data_ptr(),
                                        out_classes.data_ptr() if out_classes is not None else None,
                                        None, None, None, self.stats.data_ptr())
        _lib.check(rc, "ndnet_ndt_prune")

    def point_rows(self, points: torch.Tensor, rows_block: Optional[torch.Tensor] = None,
                   num_nds: Optional[int] = None, fill: str = "none",
                   out: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The output row of every input point, int32 ``[B, N]``, after the last
        ``run`` / ``prune`` of this plan on the same ``points`` (stream
        ordered; include/ndnet_amd.h ndnet_ndt_point_rows).  A point that
        contributed to no surviving row gets -1 (``fill="none"``) or the row
        whose mean is nearest (``fill="nearest"``: ``rows_block`` is the
        ``[B, num_nds, 12]`` block that level wrote).  ``num_nds``: the NDs of
        the level last run (default: the plan's).  ``counts``: the int32
        ``[B]`` device tensor of the run it follows (None for a fixed-size
        run); a padding point (``i >= counts[b]``) gets -1 under both fills."""
        assert points.is_contiguous() and points.dtype == torch.float32 and points.device == self.device
        assert points.shape == (self.batch, self.num_points, 3)
        if fill not in _lib.POINT_FILL:
            raise ValueError(f"fill must be 'none' or 'nearest', got {fill!r}")
        k = self.num_nds if num_nds is None else int(num_nds)
        if rows_block is not None:
            assert rows_block.is_contiguous() and rows_block.dtype == torch.float32
            assert rows_block.device == self.device and rows_block.shape == (self.batch, k, 12)
        elif fill == "nearest":
            raise ValueError("fill='nearest' needs the rows block of the level last run")
        if out is None:
            out = torch.empty((self.batch, self.num_points), dtype=torch.int32, device=self.device)
        assert out.is_contiguous() and out.dtype == torch.int32 and out.device == self.device
        assert out.shape == (self.batch, self.num_points)
        rc = _lib.lib().ndnet_ndt_point_rows_counts(self.handle, _lib.stream_ptr(self.device), points.data_ptr(),
                                                    rows_block.data_ptr() if rows_block is not None else None, k,
                                                    _lib.POINT_FILL[fill], out.data_ptr(), self._counts_ptr(counts))
        _lib.check(rc, "ndnet_ndt_point_rows")
        return out

    def host_stats(self) -> list:
        raw = self.stats.cpu().numpy().tobytes()
        return [_lib.NdtStats.from_buffer_copy(raw, i * _lib.STATS_BYTES) for i in range(self.batch)]


_plans: dict = {}


def get_plan(batch: int, num_points: int, num_nds: int, num_classes: int, device: torch.device) -> NdtPlan:
    key = (batch, num_points, num_nds, num_classes, device)
    p = _plans.get(key)
    if p is None:
        p = NdtPlan(batch, num_points, num_nds, num_classes, device=device)
        _plans[key] = p
    return p


# opt-in failure check of every eager ndt_preprocessing call (see its docstring)
CHECK_RC = os.environ.get("NDNET_CHECK_RC", "0") == "1"


class NdtCloudError(RuntimeError):
    """A cloud of the batch failed (``rcs``: per-cloud return codes)."""

    def __init__(self, rcs, sync: bool = False):
        self.rcs = list(rcs)
        if sync:
            super().__init__("an earlier ndt_downsample run failed: a k_front cloud barrier timed out (rc -22, "
                             "NDNET_ERR_SYNC); its clouds hold zero rows")
            return
        bad = {b: rc for b, rc in enumerate(self.rcs) if rc != 0}
        super().__init__(f"ndt_downsample failed for clouds {bad} (rc -3: search hit 15 iterations, "
                         f"-1: grid above the voxel capacity, -22: front barrier timeout)")


def check_stats(plan: "NdtPlan") -> None:
    """Raises ``NdtCloudError`` if any cloud of the plan's last run failed
    (synchronises with the plan's stream)."""
    rcs = [s.rc for s in plan.host_stats()]
    plan.raise_sync_failures()  # consumed here: the per-cloud codes below carry it
    if any(rc != 0 for rc in rcs):
        raise NdtCloudError(rcs)


def check_counts(counts, batch: int, num_points: int) -> None:
    """The host's check of per-cloud point counts: shape ``[batch]`` and, when
    they arrive as a CPU tensor or a sequence, every value in
    ``1 .. num_points`` (``ValueError``).  A device tensor's values are not
    read -- that would synchronise; the kernels fail such a cloud with rc -20."""
    if counts is None:
        return
    on_device = isinstance(counts, torch.Tensor) and counts.is_cuda
    t = counts if on_device else torch.as_tensor(counts)
    if tuple(t.shape) != (batch,):
        raise ValueError(f"counts must have shape ({batch},), got {tuple(t.shape)}")
    if not on_device and (int(t.min()) < 1 or int(t.max()) > num_points):
        raise ValueError(f"every count must lie in 1 .. n = {num_points}, got {int(t.min())} .. {int(t.max())}")


def check_class_ids(classes: Optional[torch.Tensor], points: torch.Tensor) -> None:
    """The host's check of labels given as class ids: a 2-D ``classes`` must be
    an integer tensor of shape ``points.shape[:2]`` (``ValueError``).  One-hot
    labels (3-D) and ``None`` pass."""
    if classes is None or classes.dim() != 2:
        return
    if classes.is_floating_point() or classes.is_complex() or classes.dtype == torch.bool:
        raise ValueError(f"classes [B, N] must hold integer class ids, got {classes.dtype} "
                         "(one-hot labels are [B, N, num_classes + 1])")
    if tuple(classes.shape) != tuple(points.shape[:2]):
        raise ValueError(f"integer classes must have shape {tuple(points.shape[:2])}, got {tuple(classes.shape)}")


def class_ids(classes: torch.Tensor, dev: torch.device) -> torch.Tensor:
    """The plan's int32 ``[B, N]`` labels on ``dev``: integer class ids
    ``[B, N]`` as they come, or the first-max argmax of one-hot labels
    ``[B, N, num_classes + 1]``, as ndtnet_preprocessing.py:34 does per cloud."""
    oh = classes.to(dev)
    if oh.dim() == 2:
        return oh.to(torch.int32).contiguous()
    if oh.dtype == torch.float32:  # one HIP pass (torch's argmax + int cast: ~160 us at 16 x 100k x 29)
        oh = oh.contiguous()
        labels = torch.empty(oh.shape[:2], dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().ndnet_row_argmax(oh.data_ptr(), oh.shape[0] * oh.shape[1], oh.shape[2],
                                               labels.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
                   "ndnet_row_argmax")
        return labels
    return torch.argmax(oh, dim=2).to(torch.int32).contiguous()


def ndt_preprocessing(num_nds: int, points: torch.Tensor, classes: torch.Tensor = None,
                      num_classes: int = None, *, counts=None, check: Optional[bool] = None
                      ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """Downsample a batch of clouds to ``num_nds`` normal distributions.

    Args:
        num_nds: NDs per cloud (the reference's ``n_desired_nds``).
        points: ``[B, N, 3]`` float tensor (any device; computed on the GPU).
        classes: optional ``[B, N, num_classes + 1]`` one-hot labels, or an
            integer tensor ``[B, N]`` of class ids (``CARLA_Seg`` /
            ``collate_padded`` deliver these): the ids go to the plan as its
            int32 labels, with no one-hot and no argmax pass.  An id outside
            ``0 .. num_classes`` is left out of its voxel's histogram.  A
            floating-point ``[B, N]`` tensor or another shape is a
            ``ValueError``.
        num_classes: number of classes (labels take ``num_classes + 1`` values).
        counts: optional ``[B]`` tensor or sequence (converted to int32 on the
            device) for a ragged batch: ``points`` is then padded to
            ``[B, n_max, 3]`` (``collate_padded``), cloud ``b`` consists of its
            first ``counts[b]`` points, and its rows are, bit for bit, those
            of that cloud run alone; the padding (points and classes) may
            hold anything.  Counts given as a CPU tensor or a sequence are
            range-checked here (``ValueError`` outside ``1 .. N``); a device
            tensor is not read on the host -- a bad count fails its cloud
            with rc -20 and zero rows.

    Returns:
        ``(points [B, num_nds, 3], covariances [B, num_nds, 9], classes one-hot
        [B, num_nds, num_classes + 1] or None)`` float32 on ``points.device``.
        The first two are views of one ``[B, num_nds, 12]`` block, the layout
        the NDTNet kernels read.

    Failures: like the reference (ndt_legacy.py:153 ignores the return code;
    the zero-filled outputs of ndt_legacy.py:126-143 pass through), a failed
    cloud yields all-zero rows and a class-0 one-hot.  Failure modes are the
    reference's (-3: the bisection reached 15 iterations, ndt.c:191-194) plus
    this build's capacities: a bisection grid above the plan's voxel capacity
    (default 2^22 voxels per cloud) fails the cloud with -1 where the
    reference would malloc it.  ``check=True`` (or ``NDNET_CHECK_RC=1``)
    synchronises and raises ``NdtCloudError`` instead; it is skipped while a
    HIP graph is being captured.  Per-cloud codes: ``last_stats()``.  A
    k_front barrier timeout (-22, no reference code) is never silent: it sets
    a flag in host memory and the plan's next call raises ``NdtCloudError``
    whatever ``check`` is (``NdtPlan.raise_sync_failures``).
    """
    if counts is not None:  # (before any GPU work)
        if points.dim() != 3 or points.shape[2] != 3:
            raise ValueError(f"points must be [B, N, 3], got {tuple(points.shape)}")
        check_counts(counts, points.shape[0], points.shape[1])
    check_class_ids(classes, points)
    _lib.require_gpu()
    src_device = points.device
    dev = src_device if src_device.type == "cuda" else torch.device("cuda", torch.cuda.current_device())
    pts = points.to(device=dev, dtype=torch.float32).contiguous()
    B, N, D = pts.shape
    if D != 3:
        raise ValueError(f"points must be [B, N, 3], got {tuple(pts.shape)}")
    counts = _per_cloud(counts, B, dev, "counts")
    labelled = classes is not None
    if labelled and num_classes is None:
        raise ValueError("num_classes is required with classes")
    ncls = int(num_classes) if labelled else -1
    plan = get_plan(B, N, int(num_nds), ncls, dev)
    out = torch.empty((B, num_nds, 12), dtype=torch.float32, device=dev)
    out_cls = None
    labels = None
    if labelled:
        labels = class_ids(classes, dev)
        out_cls = torch.empty((B, num_nds, ncls + 1), dtype=torch.float32, device=dev)
    plan.run(pts, labels, out, out_cls, counts=counts)
    ndt_preprocessing.last_plan = plan
    ndt_preprocessing.last_rows = out  # the device block (ndnet.segment.point_rows reads it)
    ndt_preprocessing.last_counts = counts  # ... and the run's counts on the device, or None
    if (CHECK_RC if check is None else check) and not torch.cuda.is_current_stream_capturing():
        check_stats(plan)
    if src_device != dev:
        out = out.to(src_device)
        out_cls = out_cls.to(src_device) if out_cls is not None else None
    return out[..., :3], out[..., 3:], out_cls


ndt_preprocessing.last_plan = None
ndt_preprocessing.last_rows = None
ndt_preprocessing.last_counts = None


def ndt_multiscale(levels, points: torch.Tensor, classes: torch.Tensor = None, num_classes: int = None, *,
                   counts=None) -> list:
    """Multi-level NDT of a batch (config C5, tools/train_multiscale.py's
    levels): ``downsample(levels[0])`` then ``prune(levels[i])`` for each
    further, smaller level on the retained KL list -- NDT_Sampler.downsample /
    .prune (ndt_legacy.py:111-240) for every cloud at once, all on the GPU.

    Returns one ``(points [B,k,3], covariances [B,k,9], classes or None)`` per
    level, as ndt_preprocessing does for one level.  ``counts``: per-cloud
    point counts of a ragged batch, as ndt_preprocessing takes them (the prune
    levels read the plan's state only)."""
    levels = [int(k) for k in levels]
    if not levels or any(b >= a for a, b in zip(levels, levels[1:])):
        raise ValueError(f"levels must be strictly decreasing, got {levels}")
    p, c, cls = ndt_preprocessing(levels[0], points, classes, num_classes, counts=counts)
    out = [(p, c, cls)]
    plan = ndt_preprocessing.last_plan
    dev = plan.device
    B = p.shape[0]
    for k in levels[1:]:
        blk = torch.empty((B, k, 12), dtype=torch.float32, device=dev)
        blk_cls = torch.empty((B, k, cls.shape[2]), dtype=torch.float32, device=dev) if cls is not None else None
        plan.prune(k, blk, blk_cls)
        ndt_preprocessing.last_rows = blk  # the last level's block, as ndt_preprocessing keeps its own
        if points.device != dev:
            blk = blk.to(points.device)
            blk_cls = blk_cls.to(points.device) if blk_cls is not None else None
        out.append((blk[..., :3], blk[..., 3:], blk_cls))
    return out


def ndt_preprocessing_packed(num_nds: int, points: torch.Tensor) -> torch.Tensor:
    """The unlabelled path returning the ``[B, num_nds, 12]`` block itself."""
    p, _, _ = ndt_preprocessing(num_nds, points)
    return p.as_strided((p.shape[0], p.shape[1], 12), (p.shape[1] * 12, 12, 1))


def last_stats() -> list:
    """Per-cloud ``ndnet_ndt_stats`` of the last ``ndt_preprocessing`` call."""
    plan = ndt_preprocessing.last_plan
    return plan.host_stats() if plan is not None else []
