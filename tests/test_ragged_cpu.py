"""Ragged batches (per-cloud point counts), the parts that need no GPU: the
header declares the counts entry points and the bindings cover them, the host's
range check of counts given as a list or a CPU tensor raises before any GPU
call, and GraphedSegmentation refuses a bad ``ragged`` before any GPU work."""
import inspect
import os
import re

import pytest
import torch

from conftest import REPO

ENTRIES = ("ndnet_ndt_run_counts", "ndnet_ndt_run_f64_counts", "ndnet_ndt_point_rows_counts")


def _no_gpu(monkeypatch):
    """The calls below must raise before they reach the GPU: make reaching it an error of another type."""
    from ndnet import _lib

    def reached():
        raise AssertionError("the check did not come before the GPU call")

    monkeypatch.setattr(_lib, "require_gpu", reached)


def test_header_declares_and_bindings_cover_the_counts_entries():
    from ndnet import _lib
    hdr = open(os.path.join(REPO, "include", "ndnet_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.lib()
    for name in ENTRIES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", code)
        assert m, name
        assert re.search(r"const\s+int32_t\s*\*\s*d_counts", m.group(1)), name
        assert name in _lib.EXPORTS and hasattr(lib, name)
        # one argument more than the call it extends, every pointer as void *
        base = name.replace("_counts", "")
        assert len(_lib.EXPORTS[name][1]) == len(_lib.EXPORTS[base][1]) + 1
        assert len(_lib.EXPORTS[name][1]) == len(m.group(1).split(","))
    # the existing signatures are as they were
    assert re.search(r"int ndnet_ndt_run\(void \*plan, void \*stream, const float \*d_points, "
                     r"const int32_t \*d_labels, float \*d_out,\s+float \*d_out_classes, "
                     r"ndnet_ndt_stats \*d_stats\);", code)
    # the contract is written down where the entry points are declared
    for phrase in ("NDNET_ERR_ARG (-20)", "must not\n * change while a run that reads it is in flight",
                   "part 2 takes the same d_counts as part 1"):
        assert phrase in hdr, phrase


def test_null_plan_is_refused_without_a_launch():
    from ndnet import _lib
    L, E, P = _lib.lib(), _lib.NDNET_ERR_ARG, 0x1000  # (P is never dereferenced)
    assert L.ndnet_ndt_run_counts(None, None, P, None, P, P, None, None) == E
    assert L.ndnet_ndt_run_f64_counts(None, None, P, None, P, None, None, None, P, None) == E
    assert L.ndnet_ndt_point_rows_counts(None, None, P, None, 1, 0, P, P) == E


def test_python_signatures_take_counts():
    from ndnet import segment
    from ndnet.pipeline import GraphedSegmentation
    from ndnet.preprocessing.ndtnet_preprocessing import NdtPlan, ndt_multiscale, ndt_preprocessing
    for f in (NdtPlan.run, NdtPlan.point_rows, ndt_preprocessing, ndt_multiscale, segment.point_rows,
              segment.segment_points, GraphedSegmentation.__call__):
        p = inspect.signature(f).parameters
        assert "counts" in p and p["counts"].default is None, f
    assert inspect.signature(ndt_preprocessing).parameters["counts"].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(GraphedSegmentation.__init__).parameters["ragged"].default is False
    assert ndt_preprocessing.last_counts is None or isinstance(ndt_preprocessing.last_counts, torch.Tensor)


@pytest.mark.parametrize("counts", [[16, 0], [16, 17], [1, -3], torch.tensor([0, 16]), torch.tensor([16, 17]),
                                    [16], [16, 16, 16], torch.tensor([[16, 16]]), (17, 1)])
def test_host_check_of_counts_comes_before_the_gpu(monkeypatch, counts):
    from ndnet import segment
    from ndnet.preprocessing.ndtnet_preprocessing import ndt_multiscale, ndt_preprocessing
    _no_gpu(monkeypatch)
    pts = torch.zeros((2, 16, 3))
    with pytest.raises(ValueError, match="count"):
        ndt_preprocessing(4, pts, counts=counts)
    with pytest.raises(ValueError, match="count"):
        ndt_multiscale((4, 2), pts, counts=counts)
    with pytest.raises(ValueError, match="count"):
        segment.segment_points(lambda p, c: None, 4, pts, counts=counts)
    with pytest.raises(ValueError, match="count"):
        segment.point_rows(pts, counts=counts)


def test_valid_counts_pass_the_host_check(monkeypatch):
    """1 and n are both in range; the call then goes on to the GPU (here: the stand-in's error)."""
    from ndnet.preprocessing.ndtnet_preprocessing import check_counts, ndt_preprocessing
    check_counts([1, 16], 2, 16)
    check_counts(torch.tensor([16, 1]), 2, 16)
    check_counts(None, 2, 16)
    _no_gpu(monkeypatch)
    with pytest.raises(AssertionError, match="did not come before"):
        ndt_preprocessing(4, torch.zeros((2, 16, 3)), counts=[1, 16])


@pytest.mark.parametrize("ragged", ["yes", 1, None, 0])
def test_graphed_segmentation_refuses_a_bad_ragged_before_the_gpu(monkeypatch, ragged):
    from ndnet.pipeline import GraphedSegmentation
    _no_gpu(monkeypatch)
    with pytest.raises(ValueError, match="ragged"):
        GraphedSegmentation(torch.nn.Linear(1, 1), 4, 2, 16, ragged=ragged)
    # a valid ragged goes on to the other checks and then to the GPU
    with pytest.raises(ValueError, match="point_labels"):
        GraphedSegmentation(torch.nn.Linear(1, 1), 4, 2, 16, ragged=True, point_labels="mean")
    with pytest.raises(AssertionError, match="did not come before"):
        GraphedSegmentation(torch.nn.Linear(1, 1), 4, 2, 16, ragged=True)
