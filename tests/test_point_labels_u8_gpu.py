"""ndnet_seg_point_labels_u8 (include/ndnet_segment.h) against numpy, exactly:
the byte labels through every path of its gather -- the 16-byte row load and
4-byte label store, the four-scalar-load form for rows off a 16-byte boundary,
the byte-store head of a cloud whose output starts off a word boundary, the
tail, clouds whose base b * n is no multiple of four -- with the bytes around
the output left alone, and equal to the int32 entry's labels cast to bytes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

I32_MIN = -2 ** 31
SENTINEL = 0xA5
PAD = 32  # sentinel bytes on both sides of the output
# (byte offset of the output, int32 offset of the rows) from a 256-byte aligned
# allocation: (0, 0) takes the vector loads, (0, 2) and, for most n, the others
# the scalar loads; output offsets 1 .. 3 give every head length
OFFSETS = [(0, 0), (1, 0), (2, 1), (3, 3), (0, 2)]


def _case(B, n, k, cols, seed):
    rng = np.random.default_rng(seed)
    scores = rng.integers(-3, 4, (B, k, cols)).astype(np.float32)  # small integers: ties in every row
    scores[rng.random((B, k, cols)) < 0.1] = np.nan
    scores[:, 0, :] = 1.5                                          # an all-equal row
    special = np.array([-1, k, k + 7, I32_MIN], np.int64)
    rows = rng.integers(0, k, (B, n))
    pick = rng.random((B, n)) < 0.3
    rows[pick] = special[rng.integers(0, 4, int(pick.sum()))]
    if n >= 4:
        rows[:, rng.permutation(n)[:4]] = special                  # each of them in every cloud
    nd = np.argmax(scores, axis=2).astype(np.int32)                # first maximum, NaN as a maximum
    ok = (rows >= 0) & (rows < k)
    gathered = np.take_along_axis(nd, np.where(ok, rows, 0), axis=1)
    return scores, rows.astype(np.int32), nd, ok, gathered


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 255, 256, 257, 1023, 1025])
def test_u8_labels_match_numpy_at_every_alignment(n):
    import torch
    from ndnet import segment
    dev = torch.device("cuda", 0)
    for B in (1, 3):
        for k in (1, 5, 400):
            for cols in (1, 6, 255):
                scores, rows, nd, ok, gathered = _case(B, n, k, cols, seed=1000 * n + 100 * B + k + cols)
                d_scores = torch.from_numpy(scores).to(dev)
                ref32 = segment.point_labels(d_scores, torch.from_numpy(rows).to(dev), unassigned=-1)
                assert np.array_equal(ref32.cpu().numpy(), np.where(ok, gathered, -1))
                rows_buf = torch.zeros(B * n + 8, dtype=torch.int32, device=dev)
                for unassigned in (255, cols):
                    expect = np.where(ok, gathered, unassigned).astype(np.uint8)
                    for out_off, row_off in OFFSETS:
                        d_rows = rows_buf[row_off:row_off + B * n].view(B, n)
                        d_rows.copy_(torch.from_numpy(rows))
                        buf = torch.full((PAD + 3 + B * n + PAD,), SENTINEL, dtype=torch.uint8, device=dev)
                        out = buf[PAD + out_off:PAD + out_off + B * n].view(B, n)
                        assert out.data_ptr() % 4 == out_off and d_rows.data_ptr() % 16 == 4 * row_off
                        d_nd = torch.full((B, k), -7, dtype=torch.int32, device=dev)
                        got = segment.point_labels(d_scores, d_rows, unassigned=unassigned, out=out, nd_labels=d_nd)
                        assert got.data_ptr() == out.data_ptr() and got.dtype == torch.uint8
                        where = (B, k, cols, unassigned, out_off, row_off)
                        h = buf.cpu().numpy()
                        assert np.array_equal(h[PAD + out_off:PAD + out_off + B * n].reshape(B, n), expect), where
                        assert (h[:PAD + out_off] == SENTINEL).all(), where
                        assert (h[PAD + out_off + B * n:] == SENTINEL).all(), where
                        assert np.array_equal(d_nd.cpu().numpy(), nd), where
                # the int32 entry's labels, cast: -1 becomes 255
                assert np.array_equal(ref32.cpu().numpy().astype(np.uint8), np.where(ok, gathered, 255).astype(np.uint8))


def test_u8_defaults_and_dtype_argument():
    """dtype=torch.uint8 without out: a new uint8 tensor with 255 for a point
    without a row; the default call stays int32 with -1."""
    import torch
    from ndnet import segment
    dev = torch.device("cuda", 0)
    scores, rows, nd, ok, gathered = _case(2, 1001, 37, 6, seed=5)
    d_scores, d_rows = torch.from_numpy(scores).to(dev), torch.from_numpy(rows).to(dev)
    a = segment.point_labels(d_scores, d_rows, dtype=torch.uint8)
    b = segment.point_labels(d_scores, d_rows)
    assert a.dtype == torch.uint8 and b.dtype == torch.int32
    assert np.array_equal(a.cpu().numpy(), np.where(ok, gathered, 255).astype(np.uint8))
    assert np.array_equal(b.cpu().numpy(), np.where(ok, gathered, -1))
