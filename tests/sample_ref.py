"""The numpy oracle of the random subsample (include/ndnet_sample.h): the keys
from the augmentation oracle's Philox with purpose 3, the selection as a
lexicographic sort, the filler rows, and the gather by given indices."""
import numpy as np

from aug_ref import counter, philox

PURPOSE = 3
TILE = 1024  # NDNET_SAMPLE_TILE
LIST = 1024  # NDNET_SAMPLE_LIST


def keys(seed, stream, b, m, step, key_bits=32):
    """key[i] of the points 0 .. m - 1 of cloud b: word 0 >> (32 - key_bits), uint32 [m]."""
    assert 1 <= key_bits <= 32
    w0 = philox(*counter(np.arange(m), b, step, PURPOSE), seed, stream)[0]
    return w0 >> np.uint32(32 - key_bits)


def choose(key, S):
    """The chosen indices, ascending: all of them if there are at most S, else
    the S smallest in (key, index)."""
    m = len(key)
    if m <= S:
        return np.arange(m)
    return np.sort(np.lexsort((np.arange(m), key))[:S])


def choose_threshold(key, S):
    """The same set in the threshold form: tau the S-th smallest key, every key
    below it and the first S - #{key < tau} indices among the keys equal to it.
    Returns (indices, tau, #{key < tau}, #{key == tau}); tau None for m <= S."""
    m = len(key)
    if m <= S:
        return np.arange(m), None, 0, 0
    tau = np.sort(key)[S - 1]
    below = np.nonzero(key < tau)[0]
    ties = np.nonzero(key == tau)[0]
    quota = S - len(below)
    assert 1 <= quota <= len(ties)
    return np.sort(np.concatenate([below, ties[:quota]])), tau, len(below), len(ties)


def cloud_len(counts, b, n):
    return n if counts is None else min(max(int(counts[b]), 1), n)


def sample(seed, stream, points, labels, counts, S, step, key_bits=32, fill_label=-1):
    """The whole call on a [B, n, 3] batch: (points [B, S, 3], labels [B, S]
    int32 | None, counts [B] int32, indices [B, S] int32).  Nothing past a
    cloud's count is read."""
    B, n, _ = points.shape
    out_p = np.empty((B, S, 3), np.float32)
    out_l = None if labels is None else np.empty((B, S), np.int32)
    out_c = np.empty(B, np.int32)
    out_i = np.empty((B, S), np.int32)
    for b in range(B):
        m = cloud_len(counts, b, n)
        idx = choose(keys(seed, stream, b, m, step, key_bits), S)
        k = len(idx)
        out_c[b] = k
        out_i[b, :k], out_i[b, k:] = idx, -1
        out_p[b, :k], out_p[b, k:] = points[b, idx], points[b, 0]
        if labels is not None:
            out_l[b, :k], out_l[b, k:] = labels[b, idx], fill_label
    return out_p, out_l, out_c, out_i


def gather(points, labels, indices, fill_label=-1):
    """ndnet_sample_gather_run: a row with 0 <= index < n takes that point and
    label, any other point 0 and fill_label; the counts are the valid rows."""
    B, n, _ = points.shape
    ok = (indices >= 0) & (indices < n)
    safe = np.where(ok, indices, 0)
    rows = np.arange(B)[:, None]
    out_p = points[rows, safe].astype(np.float32)
    out_l = None if labels is None else np.where(ok, labels[rows, safe], fill_label).astype(np.int32)
    return out_p, out_l, ok.sum(1).astype(np.int32)
