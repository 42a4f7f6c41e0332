"""The numpy oracle of the augmentation (include/ndnet_augment.h): Philox4x32-10
from its definition, the per-cloud parameters in float64, the per-point chain
in float32 with one numpy operation per rounding."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
K = np.float32(np.sqrt(3.0) / 65536.0)


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of the counters (arrays or ints, broadcast together) under
    the key (k0, k1): the four output words, uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(MASK) for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & MASK, int(k1) & MASK
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(MASK),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(MASK)]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return [v.astype(np.uint32) for v in c]


def counter(i, b, step, purpose):
    """(i, b, uint32(step), (uint32(step >> 32) << 2) | purpose)."""
    step = int(step)
    assert 0 <= step < 1 << 62 and 0 <= purpose < 4
    return i, b, step & MASK, (((step >> 32) << 2) | purpose) & MASK


def u24(w):
    return (np.asarray(w, dtype=np.uint32) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


class Config:
    """The fields of ndnet_aug_config."""

    def __init__(self, seed=0, stream=0, yaw_max=0.0, scale_lo=1.0, scale_hi=1.0, shift_max=(0.0, 0.0, 0.0),
                 drop_max=0.0, jitter_sigma=0.0, flip_x_16=0, flip_y_16=0):
        self.seed, self.stream = int(seed), int(stream)
        self.yaw_max, self.scale_lo, self.scale_hi = float(yaw_max), float(scale_lo), float(scale_hi)
        self.shift_max = tuple(float(v) for v in shift_max)
        self.drop_max, self.jitter_sigma = float(drop_max), float(jitter_sigma)
        self.flip_x_16, self.flip_y_16 = int(flip_x_16), int(flip_y_16)

    @classmethod
    def of(cls, aug):
        """The config an ndnet.augment.Augment passes to the kernels."""
        c = aug.config()
        return cls(c.seed, c.stream, c.yaw_max, c.scale_lo, c.scale_hi, tuple(c.shift_max), c.drop_max,
                   c.jitter_sigma, c.flip_x_16, c.flip_y_16)


def cloud_params(cfg, B, step):
    """(xform [B, 12] float32, T [B] uint32, flips [B, 2] of +-1): each entry of
    [M | t] computed in float64 and rounded once."""
    b = np.arange(B)
    P = philox(*counter(0, b, step, 0), cfg.seed, cfg.stream)
    Q = philox(*counter(1, b, step, 0), cfg.seed, cfg.stream)
    theta = (2.0 * u24(P[0]) - 1.0) * cfg.yaw_max
    s = cfg.scale_lo + u24(P[1]) * (cfg.scale_hi - cfg.scale_lo)
    fx = np.where((P[2] & np.uint32(0xFFFF)) < cfg.flip_x_16, -1.0, 1.0)
    fy = np.where((P[2] >> np.uint32(16)) < cfg.flip_y_16, -1.0, 1.0)
    T = np.floor(u24(P[3]) * cfg.drop_max * 2.0 ** 32).astype(np.uint64).astype(np.uint32)
    c, z = np.cos(theta), np.sin(theta)
    sc, sz = s * c, s * z
    t = [(2.0 * u24(Q[a]) - 1.0) * cfg.shift_max[a] for a in range(3)]
    zero = np.zeros(B)
    X = np.stack([fx * sc, fx * -sz, zero, t[0], fy * sz, fy * sc, zero, t[1], zero, zero, s, t[2]], axis=1)
    return X.astype(np.float32), T, np.stack([fx, fy], axis=1)


def point_words(cfg, b, m, step):
    """W0 .. W7 of the points 0 .. m - 1 of cloud b: [8, m] uint32."""
    i = np.arange(m)
    return np.stack(philox(*counter(i, b, step, 1), cfg.seed, cfg.stream) +
                    philox(*counter(i, b, step, 2), cfg.seed, cfg.stream))


def jitter_z(W, a):
    """z of axis a from the words [8, m]: float(S - 131070) * K in float32."""
    lo, hi = np.uint32(0xFFFF), np.uint32(16)
    S = ((W[2 * a] & lo).astype(np.int64) + (W[2 * a] >> hi) + (W[2 * a + 1] & lo) + (W[2 * a + 1] >> hi))
    return (S - 131070).astype(np.float32) * K


def keep_mask(W, T):
    k = W[6] >= np.uint32(T)
    k[0] = True
    return k


def apply_cloud(cfg, b, pts, step, xform_row, T):
    """The kept indices of cloud b and their transformed points [m', 3]:
    pts [m, 3] float32 (the cloud's existing points), xform_row its 12 float32."""
    pts = np.asarray(pts, dtype=np.float32)
    m = pts.shape[0]
    W = point_words(cfg, b, m, step)
    keep = keep_mask(W, T) if cfg.drop_max > 0 else np.ones(m, bool)
    X = np.asarray(xform_row, dtype=np.float32).reshape(3, 4)
    sigma = np.float32(cfg.jitter_sigma)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    out = np.empty((m, 3), np.float32)
    with np.errstate(all="ignore"):
        for a in range(3):
            j = sigma * jitter_z(W, a)
            v = X[a, 0] * x
            v = v + X[a, 1] * y
            v = v + X[a, 2] * z
            v = v + X[a, 3]
            out[:, a] = v + j
    idx = np.nonzero(keep)[0]
    return idx, out[idx]


def augment(cfg, points, labels, counts, step, xform=None):
    """The whole call on a [B, n, 3] batch: (xform, T, per-cloud lists of kept
    indices, points and labels).  `xform`: the matrices to apply (the kernel's
    own, to compare the points bit for bit), default the oracle's."""
    B, n, _ = points.shape
    X, T, _ = cloud_params(cfg, B, step)
    use = X if xform is None else np.asarray(xform, np.float32).reshape(B, 12)
    idx, pts, lab = [], [], []
    for b in range(B):
        m = n if counts is None else min(max(int(counts[b]), 1), n)
        i, p = apply_cloud(cfg, b, points[b, :m], step, use[b], T[b])
        idx.append(i)
        pts.append(p)
        lab.append(None if labels is None else labels[b, i])
    return X, T, idx, pts, lab
