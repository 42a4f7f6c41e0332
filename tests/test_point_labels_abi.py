"""The point-label entry points reject misuse before any launch (CPU: the
arguments are host memory, nothing reaches a GPU), ndnet.segment.iou is plain
torch, and GraphedSegmentation's point_labels argument is checked before any
GPU work."""
import ctypes

import numpy as np
import pytest


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_seg_point_labels_rejects_bad_arguments():
    from ndnet import _lib
    f = _lib.lib().ndnet_seg_point_labels
    E = _lib.NDNET_ERR_ARG
    scores, rows = np.zeros((2, 4, 3), np.float32), np.zeros((2, 5), np.int32)
    nd, pl = np.full((2, 4), 7, np.int32), np.full((2, 5), 7, np.int32)
    good = [_p(scores), _p(rows), 2, 5, 4, 3, -1, _p(nd), _p(pl), None]
    for i in (0, 1, 7, 8):  # a NULL pointer
        a = list(good)
        a[i] = None
        assert f(*a) == E, i
    for i, bad in ((2, 0), (2, -1), (3, 0), (4, 0), (5, 0), (5, -3)):  # B, n, k, cols < 1
        a = list(good)
        a[i] = bad
        assert f(*a) == E, (i, bad)
    assert (nd == 7).all() and (pl == 7).all()


def test_seg_confusion_rejects_bad_arguments():
    from ndnet import _lib
    f = _lib.lib().ndnet_seg_confusion
    E = _lib.NDNET_ERR_ARG
    pred, gt, conf = np.zeros(8, np.int32), np.zeros(8, np.int32), np.full(10, 7, np.uint64)
    good = [_p(pred), _p(gt), 8, 3, _p(conf), None]
    for i in (0, 1, 4):
        a = list(good)
        a[i] = None
        assert f(*a) == E, i
    for i, bad in ((2, 0), (3, 0), (3, -1)):  # count == 0, cols < 1
        a = list(good)
        a[i] = bad
        assert f(*a) == E, (i, bad)
    assert (conf == 7).all()


def test_point_rows_rejects_a_null_plan():
    from ndnet import _lib
    pts, blk, out = np.zeros((1, 8, 3), np.float32), np.zeros((1, 2, 12), np.float32), np.full((1, 8), 7, np.int32)
    for fill in (0, 1):
        assert _lib.lib().ndnet_ndt_point_rows(None, None, _p(pts), _p(blk), 2, fill, _p(out)) == _lib.NDNET_ERR_ARG
    assert (out == 7).all()
    assert _lib.POINT_FILL == {"none": 0, "nearest": 1}


def test_iou_on_hand_made_matrices():
    import torch
    from ndnet import segment
    # [gt, pred]; class 2 never occurs and is never predicted: an empty union
    conf = torch.tensor([[3, 1, 0],
                         [1, 2, 0],
                         [0, 0, 0]])
    per, mean = segment.iou(conf)
    assert per.dtype == torch.float64 and per.shape == (3,)
    assert per[0].item() == 3 / 5 and per[1].item() == 2 / 4 and torch.isnan(per[2])
    assert mean.item() == pytest.approx((3 / 5 + 2 / 4) / 2, rel=1e-15)
    # predicted but absent from the ground truth: a non-empty union with IoU 0 counts in the mean
    conf = torch.tensor([[4, 0, 2],
                         [0, 6, 0],
                         [0, 0, 0]], dtype=torch.int64)
    per, mean = segment.iou(conf)
    assert per.tolist() == [4 / 6, 1.0, 0.0] and mean.item() == pytest.approx((4 / 6 + 1.0) / 3, rel=1e-15)
    per, mean = segment.iou(torch.eye(4, dtype=torch.int64) * 5)
    assert per.tolist() == [1.0] * 4 and mean.item() == 1.0
    per, mean = segment.iou(torch.zeros((2, 2), dtype=torch.int64))
    assert torch.isnan(per).all() and torch.isnan(mean)


def test_graphed_point_labels_argument_is_checked_first(monkeypatch):
    """The ValueErrors come before any GPU work: require_gpu is never reached."""
    from ndnet import _lib, pipeline
    from ndnet.models.ndtnet import NDTNetClassification, NDTNetSegmentation

    def no_gpu_work():
        raise AssertionError("GPU work before the argument check")

    monkeypatch.setattr(_lib, "require_gpu", no_gpu_work)
    seg = NDTNetSegmentation(3, 5, 64).eval()
    cls = NDTNetClassification(3, 5, 64).eval()
    with pytest.raises(ValueError, match="NDTNetSegmentation"):
        pipeline.GraphedSegmentation(cls, 8, 1, 64, point_labels="nearest")
    with pytest.raises(ValueError, match="levels"):
        pipeline.GraphedSegmentation(seg, 8, 1, 64, levels=(8, 4), point_labels="none")
    with pytest.raises(ValueError, match="point_labels"):
        pipeline.GraphedSegmentation(seg, 8, 1, 64, point_labels="mean")
    with pytest.raises(AssertionError):  # a valid argument goes on to the GPU work
        pipeline.GraphedSegmentation(seg, 8, 1, 64, point_labels="nearest")
