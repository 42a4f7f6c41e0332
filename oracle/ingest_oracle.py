"""TEST INFRASTRUCTURE ONLY (the checker, never the product): a restatement of
the reference's CARLA_Seg.get_data_pcl (ndnet/datasets/CARLA_Seg.py:97-175)
in plain Python, for the parity tests of the native PLY reader and of
ndnet.datasets.CARLA_Seg.  Parity pinned by construction: the reference's own
loop (readlines, strip().split(), float() of tokens 0-2, int() of the last
token, the class bound, np.random.choice without replacement, float32 points,
one-hot of n_classes + 1), minus open3d (imported but unused on that path).
"""
import io

import numpy as np


class LineError(Exception):
    """What the loop raised (``__cause__``) and where: ``index`` counts the data lines before it."""

    def __init__(self, index):
        super().__init__(index)
        self.index = index


def parse_lines(pcl, n_classes, num_header_lines=10, skip_blank=False):
    """The reference's loop over ``readlines()``: a list of ``[x, y, z]`` and the list of class
    tags (Python ints, before the uint16 cast).  ``skip_blank`` leaves out the lines whose
    ``strip().split()`` is empty, on which the loop raises IndexError (the native reader skips
    them, include/ndnet_ingest.h)."""
    points, classes = [], []
    for point in pcl[num_header_lines:]:                       # CARLA_Seg.py:118
        data = point.strip().split()                           # :120
        if skip_blank and not data:
            continue
        x, y, z = float(data[0]), float(data[1]), float(data[2])
        class_tag = int(data[-1])                              # :124
        if class_tag > n_classes:                              # :126-127
            raise ValueError(f"Class tag {class_tag} out of bounds")
        points.append([x, y, z])
        classes.append(class_tag)
    return points, classes


def parse_bytes(raw, n_classes, num_header_lines=10, errors="strict"):
    """``parse_lines`` of a file's bytes, blank lines skipped: the lines are those of
    ``open(path, "r").readlines()`` (UTF-8, universal newlines; ``errors`` as ``open``'s).
    Returns ``(xyz [n, 3] float64, tags: list of int)``; whatever the loop raises comes as the ``__cause__`` of a ``LineError``
    with the number of data lines read before it."""
    pcl = io.TextIOWrapper(io.BytesIO(raw), encoding="utf-8", errors=errors).readlines()
    data = [ln for ln in pcl[num_header_lines:] if ln.strip().split()]
    points, classes = [], []
    for i, ln in enumerate(data):
        try:
            p, c = parse_lines([ln], n_classes, 0)
        except Exception as exc:
            raise LineError(i) from exc
        points += p
        classes += c
    return np.asarray(points, np.float64).reshape(-1, 3), classes


def get_data_pcl(pcl_filename, n_classes, n_samples, num_header_lines=10):
    with open(pcl_filename, "r") as f:
        pcl = f.readlines()                                    # CARLA_Seg.py:113-115
    points, classes = parse_lines(pcl, n_classes, num_header_lines)
    points = [np.array(p) for p in points]
    np_points = np.asarray(points)
    point_indexes = np.random.choice(np_points.shape[0], n_samples, replace=False)  # :137-138
    np_points = np_points[point_indexes]
    np_classes = np.asarray(classes, dtype=np.uint16)[point_indexes]                # :142-143
    pts = np_points.astype(np.float32)                                              # :164 torch.tensor(...).float()
    gt = np.zeros((np_classes.shape[0], n_classes + 1), np.float32)                 # :167-170
    for i in range(np_classes.shape[0]):
        gt[i, int(np_classes[i])] = 1
    return pts, gt
