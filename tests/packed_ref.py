"""The numpy oracle of the packed int16 point format (include/ndnet_packed.h,
ndnet/packed.py), written from the format's definition alone.

Decode: ``x = RN(RN(float32(q) * step) + o)``, element-wise in float32 -- numpy
rounds every float32 operation separately, so ``q.astype(np.float32) * step +
origin`` on float32 arrays is that, exactly.  ``decode_fused`` is what a fused
multiply-add would give (one rounding), the form the kernel must NOT compute:
the two differ only when the step is no power of two and the origin is not 0.

Pack: an independent transcription of the rules (midpoint origin in float32,
the smallest float32 step that reaches the half extent in 32767 steps, ``rint``
in float64), with exact rational arithmetic where the rule says "smallest".
"""
from fractions import Fraction

import numpy as np

STEPS = (np.float32(0.00313), np.float32(0.0217))            # not powers of two
ORIGINS = ((12.7, -340.2, 1.9), (-55.3, -7.25, -0.6), (301.1, 42.42, -3.3))  # non-zero; cloud 1 negative


def decode(q, qparams):
    """float32 ``[B, n, 3]``: two float32 roundings per element."""
    q = np.asarray(q)
    p = np.asarray(qparams, dtype=np.float32)
    assert q.dtype == np.int16 and q.ndim == 3 and p.shape == (q.shape[0], 4)
    prod = q.astype(np.float32) * p[:, None, 3:4]
    assert prod.dtype == np.float32
    out = prod + p[:, None, 0:3]
    assert out.dtype == np.float32
    return out


def decode_fused(q, qparams):
    """What ``fmaf(float(q), step, o)`` gives: the product is exact in float64
    (16 x 24 bits), the sum rounds once to float64 and once to float32."""
    p = np.asarray(qparams, dtype=np.float32).astype(np.float64)
    return (np.asarray(q).astype(np.float64) * p[:, None, 3:4] + p[:, None, 0:3]).astype(np.float32)


def default_step(half):
    """The smallest float32 ``s`` with ``s * 32767 >= half``, by exact
    rationals over the float32 neighbours of ``half / 32767``; 1 for 0."""
    if half == 0:
        return np.float32(1.0)
    guess = np.array([half / 32767.0], dtype=np.float32)
    bits = int(guess.view(np.uint32)[0])
    ok = [c for c in (np.array([b], dtype=np.uint32).view(np.float32)[0] for b in range(bits - 4, bits + 5))
          if Fraction(float(c)) * 32767 >= Fraction(float(half))]
    assert ok and len(ok) < 9  # the answer lies strictly inside the window
    return min(ok)


def pack(points, counts=None, step=None):
    """``(q int16 [B, n, 3], qparams float32 [B, 4])`` by the rules; raises
    ``OverflowError`` where a given step is too small (the oracle never clamps)."""
    x = np.asarray(points, dtype=np.float64)
    B, n, _ = x.shape
    q = np.zeros((B, n, 3), np.int16)
    qparams = np.zeros((B, 4), np.float32)
    for b in range(B):
        m = n if counts is None else int(counts[b])
        o = np.zeros(3, np.float32)
        half, extent = 0.0, 0.0
        for a in range(3):
            lo, hi = float(x[b, :m, a].min()), float(x[b, :m, a].max())
            o[a] = np.float32((lo + hi) / 2)
            half = max(half, hi - float(o[a]), float(o[a]) - lo)
            extent = max(extent, hi - lo)
        if extent == 0:  # a cloud of zero extent: step 1, whatever its points' distance to the float32 origin
            half = 0
        s = default_step(half) if step is None else np.float32(np.broadcast_to(np.asarray(step), (B,))[b])
        r = np.rint((x[b, :m] - o.astype(np.float64)) / float(s))
        if r.min() < -32768 or r.max() > 32767:
            raise OverflowError(b)
        q[b, :m] = r.astype(np.int16)
        qparams[b, :3], qparams[b, 3] = o, s
    return q, qparams


def kernel_case(B, n, seed=0):
    """The kernel tests' input: random ``q`` holding -32768, 32767 and 0 (as far
    as ``3 n`` elements allow), steps 0.00313 / 0.0217 and non-zero origins
    (cloud 1's negative on every axis).  ``|q * step|`` is 0 or >= 0.003: no
    subnormal arises."""
    rng = np.random.default_rng(1000 * B + n + 7919 * seed)
    q = rng.integers(-32768, 32768, (B, n, 3), dtype=np.int64).astype(np.int16)
    flat = q.reshape(B, -1)
    for b in range(B):
        for v, at in zip((-32768, 32767, 0), rng.permutation(3 * n)[:3]):
            flat[b, at] = v
    qparams = np.zeros((B, 4), np.float32)
    for b in range(B):
        qparams[b, :3] = ORIGINS[1] if B < 3 else ORIGINS[(b + seed) % len(ORIGINS)]
        qparams[b, 3] = STEPS[(b + seed) % 2]
    return q, qparams
