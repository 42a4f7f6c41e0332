"""The point-level loss (row histograms, ``point_loss``, the trainer's
``loss="points"``), the parts that need no GPU: the headers declare the four
entry points and the bindings cover them, bad arguments return NDNET_ERR_ARG
without a launch, the torch composition of the loss and the accuracy equals a
float64 numpy evaluation of their definitions, and the Python layer refuses bad
labels, losses and fills before any GPU work."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO

# entry point -> (header, number of arguments)
ENTRIES = {"ndnet_seg_row_hist": ("ndnet_segment.h", 9), "ndnet_tr_nll_hist": ("ndnet_train.h", 9),
           "ndnet_tr_nll_hist_bwd": ("ndnet_train.h", 8), "ndnet_tr_hist_match_cm": ("ndnet_train.h", 8)}


def _no_gpu(monkeypatch):
    """The calls below must raise before they reach the GPU: make reaching it an error of another type."""
    from ndnet import _lib

    def reached():
        raise AssertionError("the check did not come before the GPU call")

    monkeypatch.setattr(_lib, "require_gpu", reached)


def test_headers_declare_and_bindings_cover_the_entries():
    from ndnet import _lib
    lib = _lib.lib()
    tables = {"ndnet_segment.h": _lib.EXPORTS, "ndnet_train.h": _lib.TRAIN_EXPORTS}
    for name, (header, nargs) in ENTRIES.items():
        code = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", header)).read(), flags=re.S)
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", code)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name
        assert name in tables[header] and hasattr(lib, name), name
        assert len(tables[header][name][1]) == nargs, name
    hdr = open(os.path.join(REPO, "include", "ndnet_segment.h")).read()
    assert re.search(r"const int32_t \*d_point_rows, const int32_t \*d_point_labels, int B, uint64_t n, uint64_t k,\s+"
                     r"int cols, int32_t ignore_label, int32_t \*d_hist, void \*stream\)", hdr)


def test_bad_arguments_are_refused_without_a_launch():
    from ndnet import _lib
    L, E, P = _lib.lib(), _lib.NDNET_ERR_ARG, 0x1000  # (P is never dereferenced)
    hist = lambda rows=P, labels=P, B=1, n=1, k=1, cols=1, out=P: L.ndnet_seg_row_hist(  # noqa: E731
        rows, labels, B, n, k, cols, -1, out, None)
    assert hist(rows=None) == E and hist(labels=None) == E and hist(out=None) == E
    assert hist(B=0) == E and hist(n=0) == E and hist(k=0) == E and hist(cols=0) == E and hist(B=-1) == E
    nll = lambda logp=P, h=P, part=P, w=P, loss=P, B=1, C=1, N=1: L.ndnet_tr_nll_hist(  # noqa: E731
        logp, h, part, w, loss, B, C, N, None)
    assert nll(logp=None) == E and nll(h=None) == E and nll(part=None) == E and nll(w=None) == E
    assert nll(loss=None) == E and nll(B=0) == E and nll(C=0) == E and nll(N=0) == E and nll(C=33) == E
    bwd = lambda h=P, w=P, dl=P, out=P, B=1, C=1, N=1: L.ndnet_tr_nll_hist_bwd(h, w, dl, out, B, C, N, None)  # noqa: E731
    assert bwd(h=None) == E and bwd(w=None) == E and bwd(dl=None) == E and bwd(out=None) == E
    assert bwd(B=0) == E and bwd(C=0) == E and bwd(N=0) == E and bwd(C=33) == E
    match = lambda pred=P, h=P, ctr=P, B=1, C=1, N=1: L.ndnet_tr_hist_match_cm(  # noqa: E731
        pred, h, B, C, N, ctr, None, None)
    assert match(pred=None) == E and match(h=None) == E and match(ctr=None) == E
    assert match(B=0) == E and match(C=0) == E and match(N=0) == E and match(C=33) == E


def _np_loss(pred, hist):
    """-(1/W) sum h logp over the non-zero counts, in float64; 0 for W == 0."""
    p, h = pred.astype(np.float64), hist.astype(np.int64)
    W = int(h.sum())
    nz = h != 0
    return (-(h[nz] * p[nz]).sum() / W) if W else 0.0


def _np_first_argmax(pred):
    """First maximum of the last axis, NaN counting as a maximum (torch.argmax)."""
    out = np.zeros(pred.shape[:-1], np.int64)
    for idx in np.ndindex(*pred.shape[:-1]):
        row = pred[idx]
        nan = np.nonzero(np.isnan(row))[0]
        out[idx] = nan[0] if nan.size else int(np.argmax(row))
    return out


def _np_acc(pred, hist):
    h = hist.astype(np.int64)
    W = int(h.sum())
    m = int(np.take_along_axis(h, _np_first_argmax(pred)[..., None], -1).sum())
    return (np.float32(m) / np.float32(W)) if W else np.float32(0), m, W


def _case(seed, B=2, k=37, C=6):
    g = torch.Generator().manual_seed(seed)
    pred = torch.log_softmax(torch.randn(B, k, C, generator=g), -1)
    hist = torch.randint(0, 9, (B, k, C), generator=g, dtype=torch.int32)
    hist[torch.rand(B, k, C, generator=g) < 0.5] = 0
    hist[0, 3] = 0  # an empty row
    return pred, hist


def test_point_loss_and_accuracy_match_the_definitions_on_the_cpu():
    from ndnet import training
    pred, hist = _case(1)
    # -inf under a zero count contributes 0, not NaN
    hist[1, 5, 2] = 0
    pred[1, 5, 2] = float("-inf")
    loss = training.point_loss(pred, hist)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    want = _np_loss(pred.numpy(), hist.numpy())
    assert np.isfinite(loss.item()) and abs(loss.item() - want) <= 1e-5 * max(1.0, abs(want))
    # the accuracy's argmax: a NaN, an exact tie (first index wins) and an all-equal row (class 0)
    pa = pred.clone()
    pa[1, 5, 2] = -50.0
    pa[0, 0, 4] = float("nan")
    pa[0, 1, 5] = pa[0, 1].max()
    pa[1, 36, :] = 0.25
    hist[0, 0] = torch.tensor([1, 2, 3, 4, 5, 6])
    hist[1, 36] = torch.tensor([7, 0, 0, 0, 0, 9])
    acc = training.point_accuracy_tensor(pa, hist)
    want_acc, m, W = _np_acc(pa.numpy(), hist.numpy())
    assert acc.dtype == torch.float32 and acc.dim() == 0 and 0 < m < W
    assert acc.item() == float(want_acc)
    # the gradient of the definition: -h / W, zero (not NaN) under the masked -inf
    p = pred.clone().requires_grad_()
    training.point_loss(p, hist).backward()
    W = int(hist.sum())
    assert torch.allclose(p.grad, -hist.float() / W, rtol=1e-6, atol=0) and bool(torch.isfinite(p.grad).all())


def test_an_empty_histogram_gives_zero_loss_accuracy_and_gradient():
    from ndnet import training
    pred, hist = _case(2)
    hist.zero_()
    pred[0, 0, 0] = float("-inf")
    p = pred.clone().requires_grad_()
    loss = training.point_loss(p, hist)
    assert loss.item() == 0.0
    loss.backward()
    assert bool((p.grad == 0).all())
    assert training.point_accuracy_tensor(pred, hist).item() == 0.0


def test_point_loss_of_one_hot_counts_is_the_nd_loss():
    """With one point per row the point loss is segmentation_loss of the one-hot."""
    from ndnet import training
    pred, _ = _case(3)
    ids = torch.randint(0, 6, (2, 37), generator=torch.Generator().manual_seed(4))
    oh = torch.nn.functional.one_hot(ids, 6)
    a, b = training.point_loss(pred, oh.int()), training.segmentation_loss(pred, oh.float())
    assert abs(a.item() - b.item()) <= 1e-5 * abs(b.item())  # (two fp32 summation orders of 444 terms)
    assert training.point_accuracy_tensor(pred, oh.int()).item() == training.accuracy_tensor(pred, oh.float()).item()


@pytest.mark.parametrize("classes", [torch.zeros((2, 16)), torch.zeros((2, 16), dtype=torch.float64),
                                     torch.zeros((2, 15), dtype=torch.int64), torch.zeros((3, 16), dtype=torch.int32),
                                     torch.zeros((16, 2), dtype=torch.int64)])
def test_bad_class_ids_are_refused_before_the_gpu(monkeypatch, classes):
    from ndnet.preprocessing.ndtnet_preprocessing import ndt_multiscale, ndt_preprocessing
    from ndnet.training import Trainer
    _no_gpu(monkeypatch)
    pts = torch.zeros((2, 16, 3))
    with pytest.raises(ValueError, match="classes"):
        ndt_preprocessing(4, pts, classes, 5)
    with pytest.raises(ValueError, match="classes"):
        ndt_multiscale((4, 2), pts, classes, 5)
    for loss in ("nds", "points"):
        tr = Trainer(torch.nn.Linear(1, 1), 1e-3, 4, 5, torch.device("cpu"), ddp=False, loss=loss)
        with pytest.raises(ValueError, match="classes"):
            tr.step(pts, classes)


def test_integer_class_ids_pass_the_host_check(monkeypatch):
    """Ids of the points' shape go on to the GPU (here: the stand-in's error)."""
    from ndnet.preprocessing.ndtnet_preprocessing import ndt_preprocessing
    _no_gpu(monkeypatch)
    for dtype in (torch.int64, torch.int32, torch.uint8):
        with pytest.raises(AssertionError, match="did not come before"):
            ndt_preprocessing(4, torch.zeros((2, 16, 3)), torch.zeros((2, 16), dtype=dtype), 5)


@pytest.mark.parametrize("kw", [{"loss": "point"}, {"loss": None}, {"loss": "NDS"}, {"point_fill": "nearest "},
                                {"point_fill": True}, {"loss": "points", "point_fill": "mean"}])
def test_trainer_refuses_an_unknown_loss_or_fill_before_the_gpu(monkeypatch, kw):
    from ndnet.training import Trainer
    _no_gpu(monkeypatch)

    class Unmovable(torch.nn.Module):
        def to(self, *a, **k):
            raise AssertionError("the check did not come before the model was moved")

    with pytest.raises(ValueError, match="loss|point_fill"):
        Trainer(Unmovable(), 1e-3, 4, 5, torch.device("cuda", 0), ddp=False, **kw)
    # valid values go on
    for ok in ({}, {"loss": "points"}, {"loss": "points", "point_fill": "none", "ignore_label": 0}):
        with pytest.raises(AssertionError, match="model was moved"):
            Trainer(Unmovable(), 1e-3, 4, 5, torch.device("cuda", 0), ddp=False, **ok)


def test_signatures_carry_the_new_arguments():
    from ndnet import segment, training
    from ndnet.models import train_hip
    T = training.Trainer
    sig = lambda f: inspect.signature(f).parameters  # noqa: E731
    for f in (T.step, T.step_graphed, training.GraphedTrainStep.__call__):
        assert sig(f)["counts"].default is None, f
    assert list(sig(T.step))[:5] == ["self", "points", "gt_points", "train", "counts"]
    assert list(sig(T.step_graphed)) == ["self", "points", "gt_points", "counts"]
    init = sig(T.__init__)
    assert init["loss"].default == "nds" and init["point_fill"].default == "nearest"
    assert init["ignore_label"].default == -1
    assert sig(T.step_on_nds)["hist"].default is None
    assert list(sig(T.step_on_nds)) == ["self", "pcl", "covs", "gt", "train", "hist"]
    assert list(sig(segment.row_histogram)) == ["rows", "labels", "num_nds", "cols", "ignore_label", "out"]
    assert sig(segment.row_histogram)["ignore_label"].default == -1 and sig(segment.row_histogram)["out"].default is None
    assert list(sig(train_hip.nll_hist)) == ["logp", "hist"]
    assert list(sig(training.point_loss)) == ["pred", "hist"]
    assert list(sig(training.point_accuracy_tensor)) == ["pred", "hist"]
    assert "DDP" in T.__doc__ and "per-rank" in T.__doc__
