"""Packed int16 point input: half the bytes of a scan on its way to the GPU.

A packed batch is ``q`` ``[B, n, 3]`` int16 and ``qparams`` ``[B, 4]`` float32,
``(ox, oy, oz, step)`` per cloud (include/ndnet_packed.h).  The cloud is, by
definition, the decoded float32 cloud

    x[b, i, a] = RN(RN(float32(q[b, i, a]) * step[b]) + o[b, a])

-- two float32 roundings, never a fused multiply-add; in numpy
``q.astype(np.float32) * step + origin`` on float32 arrays -- so everything
downstream is as exact on it as on any other float32 cloud.  At the default
step a +-100 m scan resolves 3 mm.

``pack_points`` is host code (a ``DataLoader``'s workers run it through
``datasets.collate_packed``); ``unpack`` is the HIP decode, which
``GraphedSegmentation(packed=True)`` and ``PipelinedSegmentation(packed=True)``
launch at the head of their NDT stage.

    q, qparams = pack_points(points)             # CPU, [B, n, 3] float32 / float64
    x = unpack(q.cuda(), qparams.cuda())         # GPU, [B, n, 3] float32
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from .preprocessing.ndtnet_preprocessing import check_counts

Q_MIN, Q_MAX = -32768, 32767


def _default_step(half: float) -> np.float32:
    """The smallest float32 ``s`` with ``s * 32767 >= half`` (the product is
    exact in float64); 1 for a cloud of zero extent."""
    if half == 0.0:
        return np.float32(1.0)
    s = np.float32(half / Q_MAX)
    up, down = np.float32(np.inf), np.float32(0.0)
    while float(s) * Q_MAX < half:
        s = np.nextafter(s, up)
    while True:
        t = np.nextafter(s, down)
        if t <= 0 or float(t) * Q_MAX < half:
            return s
        s = t


def pack_points(points, counts=None, step=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``points`` ``[B, n, 3]`` (a CPU tensor or numpy array, float32 or
    float64) as ``(q [B, n, 3] int16, qparams [B, 4] float32)``, on the host.

    ``counts`` ``[B]``: only the first ``counts[b]`` points of cloud ``b``
    exist (``1 .. n``, ``ValueError`` otherwise); the padding is not read and
    packs to 0.  Every existing point must be finite (``ValueError`` naming
    the cloud).

    Per cloud, the origin is the float32 midpoint of the bounding box,
    ``o_a = float32((lo_a + hi_a) / 2)``, and the default ``step`` the smallest
    float32 with ``step * 32767 >= max_a max(hi_a - o_a, o_a - lo_a)`` (taken
    in float64; 1 for a cloud of zero extent, ``hi == lo`` on every axis), so
    every ``q`` lies within +-32767.  A given ``step`` (a scalar or ``[B]``) must be positive and
    finite, and large enough for every point of every cloud: a point whose
    ``q`` would leave ``-32768 .. 32767`` is a ``ValueError`` naming the cloud,
    never clamped.  ``q = rint((x - o) / step)`` in float64, ties to even."""
    if isinstance(points, torch.Tensor):
        if points.is_cuda:
            raise ValueError("pack_points packs on the host: give it a CPU tensor or a numpy array")
        points = points.detach().numpy()
    x = np.asarray(points)
    if x.ndim != 3 or x.shape[-1] != 3 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"points must have shape [B, n, 3] with B, n >= 1, got {tuple(x.shape)}")
    if x.dtype not in (np.float32, np.float64):
        raise ValueError(f"points must be float32 or float64, got {x.dtype}")
    B, n, _ = x.shape
    if counts is not None:
        if isinstance(counts, torch.Tensor) and counts.is_cuda:
            raise ValueError("pack_points packs on the host: give it the counts as a CPU tensor or a sequence")
        check_counts(counts, B, n)
        m = [int(c) for c in torch.as_tensor(counts).tolist()]
    else:
        m = [n] * B
    if step is not None:
        if isinstance(step, torch.Tensor):
            step = step.detach().cpu().numpy()
        st = np.asarray(step, dtype=np.float64)
        if st.ndim == 0:
            st = np.full(B, float(st))
        if st.shape != (B,):
            raise ValueError(f"step must be a scalar or have shape ({B},), got {tuple(st.shape)}")
        if not bool(np.all(np.isfinite(st) & (st > 0))):
            raise ValueError(f"every step must be positive and finite, got {st.tolist()}")
        st = st.astype(np.float32)
        if not bool(np.all(np.isfinite(st) & (st > 0))):
            raise ValueError(f"every step must be positive and finite as float32, got {st.tolist()}")
    q = np.zeros((B, n, 3), dtype=np.int16)
    qparams = np.zeros((B, 4), dtype=np.float32)
    for b in range(B):
        xb = x[b, :m[b]].astype(np.float64)
        if not bool(np.isfinite(xb).all()):
            raise ValueError(f"cloud {b} holds a point that is not finite")
        lo, hi = xb.min(axis=0), xb.max(axis=0)
        o = ((lo + hi) / 2).astype(np.float32)
        if not bool(np.isfinite(o).all()):
            raise ValueError(f"cloud {b} has an origin outside float32")
        o64 = o.astype(np.float64)
        if step is None:
            # (zero extent is hi == lo: a float64 point still lies a rounding away from its float32 origin)
            s = _default_step(float(np.maximum(hi - o64, o64 - lo).max()) if bool((hi > lo).any()) else 0.0)
            if not np.isfinite(s):
                raise ValueError(f"cloud {b} has an extent outside float32")
        else:
            s = st[b]
        r = np.rint((xb - o64) / float(s))
        if r.size and (r.min() < Q_MIN or r.max() > Q_MAX):
            raise ValueError(f"cloud {b}: step {float(s)!r} is too small, a point needs q = "
                             f"{int(r.min() if r.min() < Q_MIN else r.max())} outside {Q_MIN} .. {Q_MAX}")
        q[b, :m[b]] = r.astype(np.int16)
        qparams[b, :3], qparams[b, 3] = o, s
    return torch.from_numpy(q), torch.from_numpy(qparams)


def check_packed(q, qparams) -> None:
    """The host's check of a packed batch's shapes and dtypes (``ValueError``):
    ``q`` int16 ``[B, n, 3]`` and ``qparams`` float32 ``[B, 4]``.  No value is read."""
    if not isinstance(q, torch.Tensor) or q.dtype != torch.int16 or q.dim() != 3 or q.shape[-1] != 3:
        raise ValueError(f"packed points must be an int16 [B, n, 3] tensor, got {getattr(q, 'dtype', type(q))} "
                         f"{tuple(getattr(q, 'shape', ()))}")
    if q.shape[0] < 1 or q.shape[1] < 1:
        raise ValueError(f"packed points must hold at least one cloud and one point, got {tuple(q.shape)}")
    if qparams is None:
        raise ValueError("packed points need their qparams")
    if not isinstance(qparams, torch.Tensor) or qparams.dtype != torch.float32 or \
            tuple(qparams.shape) != (q.shape[0], 4):
        raise ValueError(f"qparams must be a float32 tensor of shape ({q.shape[0]}, 4), got "
                         f"{getattr(qparams, 'dtype', type(qparams))} {tuple(getattr(qparams, 'shape', ()))}")


def unpack(q: torch.Tensor, qparams: torch.Tensor, counts=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The decoded float32 ``[B, n, 3]`` cloud of a packed batch on the GPU
    (``ndnet_pts_unpack_i16``): stream ordered, no synchronisation, no
    allocation when ``out`` is given (capturable).

    ``counts`` ``[B]``: only the first ``counts[b]`` points of cloud ``b`` are
    read and written; the rest of ``out`` keeps what it held (of a fresh
    output: anything).  Given as a CPU tensor or a sequence they are
    range-checked as ``check_counts`` does (``ValueError``); a device tensor
    is not.  ``out`` must not overlap ``q``."""
    check_packed(q, qparams)
    B, n, _ = q.shape
    check_counts(counts, B, n)
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float32
                            or tuple(out.shape) != (B, n, 3) or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous float32 tensor of shape ({B}, {n}, 3)")
    _lib.require_gpu()
    if not q.is_cuda:
        raise RuntimeError("unpack needs the packed points on the GPU (there is no CPU fallback)")
    dev = q.device
    q = q.contiguous()
    qparams = qparams.to(dev).contiguous()
    if counts is not None:
        counts = torch.as_tensor(counts).to(device=dev, dtype=torch.int32).contiguous()
    if out is None:
        out = torch.empty((B, n, 3), dtype=torch.float32, device=dev)
    elif out.device != dev:
        raise ValueError(f"out must be on {dev}, got {out.device}")
    rc = _lib.lib().ndnet_pts_unpack_i16(q.data_ptr(), qparams.data_ptr(), B, n,
                                         counts.data_ptr() if counts is not None else None, out.data_ptr(),
                                         _lib.stream_ptr(dev))
    _lib.check(rc, "ndnet_pts_unpack_i16")
    return out
